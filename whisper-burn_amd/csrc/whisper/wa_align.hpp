// wa_align.hpp -- launchers of the token-alignment kernels (wa_align.hip):
// cross-attention weights of chosen heads, their standardise + median-of-7 +
// head mean, and dynamic time warping.  Semantics: include/whisper_amd.h
// "Token alignment".
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace wa {

// Heads whose weights one pass holds: bounds the w scratch
// ([kAlignHeadsPerPass][B][P][Fld] f32); a layer with more heads takes several passes.
constexpr int kAlignHeadsPerPass = 4;
// the row stride of w and Msum for T encoder frames (16-byte rows)
inline int align_fld(int T) { return (T + 3) / 4 * 4; }

// w[hp][b][t][f] = softmax over f < F[b] of q_t . k_f / 8 for head heads[hp] of
// one layer (hp < n_heads <= kAlignHeadsPerPass): q [B*P, 64 H] f32, k
// head-major [B][H][T][64] f32, pad / F / heads device arrays (clip b's rows are
// [pad[b], P), 1 <= F[b] <= T).  Pad rows and frames >= F[b] are neither read
// nor written.  The operand treatment of the prefill's attention kernel.
hipError_t launch_align_weights(const float* q, const float* k, int B, int P, int T, int H, const int* pad,
                                const int* F, const int* heads, int n_heads, float* w, int Fld, int ns,
                                hipStream_t st);
// Per head of the pass, in order: z = (w - mean) / std per frame column over the
// clip's real rows (std == 0: z = 0), median of 7 along frames (reflect), added
// to msum [B][P][Fld] (first: the first head overwrites); last: the sums are
// then divided by total_heads.  F[b] >= 4.
hipError_t launch_align_filter(const float* w, int B, int P, const int* pad, const int* F, int n_heads, int Fld,
                               float* msum, bool first, bool last, int total_heads, hipStream_t st);
// DTW of clip b over cost[i][j] = (negate ? -x : x)[b * x_bs + (row0[b] + i) * x_ld + j],
// i < N[b] <= 447, j < F[b]: trace bytes [B][n_ld + 1][f_ld + 1] (row 0 = 2,
// column 0 = 1), jump[b * jump_ld + i] = the frame at which the path enters row i.
hipError_t launch_align_dtw(const float* x, long x_bs, int x_ld, const int* row0, const int* N, const int* F, int B,
                            bool negate, uint8_t* trace, int n_ld, int f_ld, int* jump, int jump_ld, hipStream_t st);

}  // namespace wa
