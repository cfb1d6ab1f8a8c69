// wa_kernels.hpp -- launchers of the Whisper model kernels around the Q4 path
// (LayerNorm, attention, conv front-end, embedding; the logits and the token
// pick: wa_pick.hpp).
// Reference semantics: src/model/{layers,attention,encoder,decoder,whisper}.rs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace wa {

// Device-resident decode state (read by kernels, advanced on the device so a
// captured step graph can be replayed without host involvement).
struct DecodeState {
  int position;  // positional-embedding index of the current token
  int kv_len;    // entries in the self-attention KV cache before this step
  int step;      // greedy-loop step index (whisper.rs:104)
  int n_done;    // clips that have emitted EOT
};

// Encoder self-attention (attention.rs:243-298, non-causal), flash-style,
// f32 MFMA.  qkv: [B*T, 3D] f32 (q | k | v).  Writes the A-tiled operand of
// the output projection (rows b*T + t, K = D) -- or, with out32 non-null
// (range tier 3, wa_model), f32 rows [B*T][D] there instead.  The same holds
// for every attention launcher below.
hipError_t launch_encoder_attention(const float* qkv, int B, int T, int H, _Float16* tiled, int ns,
                                    hipStream_t st, float* out32 = nullptr);

// Decoder self-attention with KV cache (attention.rs:62-125).  qkv [B*Tq, 3D];
// appends k, v of the Tq new tokens at cache index kv_len (+ kv_base_extra)
// and attends over kv_len + Tq entries, causal inside the new tokens when
// Tq > 1 (attention.rs:270-287).  cache_k/v: [B, ctx, D].
// pad (nullable; device [B]): clip b's entries start at cache slot pad[b] (a
// right-aligned prompt, launch_prefill_self_attention) -- keys [pad[b],
// kv_len + Tq), split over the waves from pad[b], so the clip's bits are those
// of an unpadded clip with kv_len - pad[b] entries.
hipError_t launch_decoder_self_attention(const float* qkv, float* cache_k, float* cache_v, int B, int Tq, int H,
                                         int ctx, const DecodeState* state, int kv_len_host, _Float16* tiled,
                                         int ns, hipStream_t st, float* out32 = nullptr, const int* pad = nullptr);

// The decoder's attention over whole prompts of P rows per clip, flash-style
// on f16-pair MFMAs (the encoder kernel's arithmetic).
// Self-attention: qkv [B*P, 3D]; clip b's prompt is right-aligned in rows
// [pad[b], P) (pad: device [B], each in [0, P)); row t attends keys [pad[b], t]
// and K / V of the real rows are copied into the head-major caches at slots
// pad[b] .. P - 1 (cache_k null: no copy).  Pad rows are written as zeros.
hipError_t launch_prefill_self_attention(const float* qkv, float* cache_k, float* cache_v, int B, int P, int H, int ctx,
                                         const int* pad, _Float16* tiled, int ns, hipStream_t st,
                                         float* out32 = nullptr);
// Cross-attention: q [B*P, D], k / v head-major [B][H][T][64] f32; every row
// attends all T keys (each clip's K / V are read once per 128 rows).
hipError_t launch_prefill_cross_attention(const float* q, const float* k, const float* v, int B, int P, int T, int H,
                                          _Float16* tiled, int ns, hipStream_t st, float* out32 = nullptr);

// Cross-attention over cached K / V (attention.rs:177-236, the reference's
// form; used for decode groups of a few clips): q [B*Tq, D] f32, k / v
// head-major [B][H][T][64] f32 (wq4_gemm_tiled_headmajor of the encoder
// output), Tq <= 4; part: cross_attention_kv_part_floats floats, counters:
// B * H ints zeroed once (re-armed by the kernel).  Writes the A-tiled
// operand of the output projection.
int cross_attention_kv_splits(int T);
size_t cross_attention_kv_part_floats(int B, int H, int T);
hipError_t launch_cross_attention_kv(const float* q, const float* k, const float* v, int B, int Tq, int T, int H,
                                     float* part, int* counters, _Float16* tiled, int ns, hipStream_t st,
                                     float* out32 = nullptr);

// Cross-attention over the encoder output (wa_xattn.hip; attention.rs:
// 204-298 restated without K/V caches): q [B*Tq, D] f32 (rows b*Tq + i),
// wk / wv: the layer's raw key / value weights [D, D] (wtype: Q4_0 blocks or
// f16), bv: value bias, enc: [B][T][ns][D] f16 planes (launch_enc_planes),
// qt: [B*Tq][ns][ceil16(H)][D] f16 scratch zeroed once, part:
// xattn_part_floats floats.  Writes the A-tiled operand of the output
// projection.  Needs D == 64 * H, D % 128 == 0, D <= 1280.
struct XattnPlan {
  int splits;  // frame ranges per query row (workgroups per row)
  int ch;      // 16-frame sub-chunks per range
};
// The frame split of a decode (wa_xattn.hip): rows = the rows of the largest
// concurrently decoding group, free_cus = the CUs the decode has while a
// CU-masked stream runs beside it (<= 0: nothing beside it, no bound).
// force_splits < 0: the product's rule (WA_XATTN_SPLITS_RT overrides it, A/B
// runs and tests only), 0: the rule alone, > 0: that many splits (normalised).
XattnPlan xattn_plan(int T, int rows = 1, int free_cus = 0, int force_splits = -1);
// sized for every plan of up to the maximum (8) splits
size_t xattn_part_floats(int R, int H, int D, int T);
// Q4_0 Wv repacked once at model load into the cross-attention
// projection's lane order (same bytes; wv_pack_words u32 words).
size_t wv_pack_words(int H, int D);
hipError_t launch_wv_pack(const uint8_t* wv, int H, int D, uint32_t* out, hipStream_t st);
// Infinity Cache residency of the encoder planes: of every kXattnResDen
// consecutive 16-frame sub-chunks of a clip, q load with the default cache
// policy (and stay on-die from one decoder layer to the next), the others
// nontemporal.  q = kXattnResDen: everything default.  Values never change.
constexpr int kXattnResDen = 64;
struct XattnResidency {
  int q = kXattnResDen;
};
// The one predicate of every kernel that reads the planes: a fixed function
// of the clip's sub-chunk index (never of step, layer, group or split), so a
// line always loads with the same policy.  Residents are evenly interleaved:
// any n consecutive sub-chunks hold floor or ceil(n q / 64) of them, so every
// (row, split) workgroup of a launch walks the same mix.
constexpr bool xattn_chunk_resident(int chunk, int q) { return ((chunk * q) & (kXattnResDen - 1)) + q >= kXattnResDen; }
// The share for a decode whose concurrently running groups stream the planes
// of live_clips clips in all ([T][ns][D] f16 each); budget_mb < 0: the
// product's rule, else a budget in MB (10^6 bytes) that replaces it.
XattnResidency xattn_residency(int live_clips, int T, int ns, int D, double budget_mb = -1.0);
// wvp: the launch_wv_pack words of wv (Q4 weights; ignored for f16 weights).
// plan: an xattn_plan of T (no empty split, at most the maximum splits).
hipError_t launch_xattn(const float* q, const uint8_t* wk, const uint8_t* wv, const uint32_t* wvp, const float* bv,
                        int wtype, const _Float16* enc, int B, int Tq, int T, int H, int D, _Float16* qt, float* part,
                        _Float16* tiled, int ns, XattnResidency res, XattnPlan plan, hipStream_t st,
                        float* out32 = nullptr);
// A-tiled operand [R][K] (hi + lo) -> f32 rows (diagnostics).
hipError_t launch_untile(const _Float16* tiled, int R, int K, int ns, float* out, hipStream_t st);
// f32 rows [rows][D] -> [rows][ns][D] f16 planes (hi | lo) for launch_xattn.
hipError_t launch_enc_planes(const float* x, int64_t rows, int D, int ns, _Float16* out, hipStream_t st);

// Conv1D (layers.rs:77-132) as an implicit-im2col f32 MFMA GEMM + bias +
// GELU (encoder.rs:89-94) (+ pos[t] if pos != nullptr).  Input element
// (b, c, t) at in[b*in_bs + c*in_cs + t*in_ts]; output [B, T_out, N].
// w_t: weights re-laid as [N][3*C] with k = kk*C + c.
hipError_t launch_conv_gelu(const float* in, long in_bs, long in_cs, long in_ts, int B, int C, int T_in,
                            int stride, const float* w_t, const float* bias, const float* pos, int N, float* out,
                            hipStream_t st);

// x[b*Tq + t] = tok_emb[tokens[b*Tq + t]] + pos_emb[pos0 + t]   (decoder.rs:326-343)
// pos0 = state ? state->position : pos0_host.  pad (nullable; device [B]): clip
// b's positions count from its first slot, pos0 + t - pad[b] (a right-aligned
// prompt; a pad row, where that is negative, gets position 0).
hipError_t launch_embed(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                        const DecodeState* state, int pos0_host, float* x, hipStream_t st, const int* pad = nullptr);

// launch_embed + the LayerNorm-fold producer for gamma (wq4_gemm_tiled_lnfold):
// also writes at = A-tiled x * gamma and stats [rows][D/16][2] (mean and sum
// of squared deviations of each 16-column tile of x); D % 32 == 0.
hipError_t launch_embed_fold(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                             const DecodeState* state, int pos0_host, float* x, const float* gamma, _Float16* at,
                             float* stats, int ns, hipStream_t st, const int* pad = nullptr);

}  // namespace wa

