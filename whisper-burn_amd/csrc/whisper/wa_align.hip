// wa_align.hip -- gfx950 kernels of the token alignment (wa_align): what
// OpenAI's timing.py find_alignment computes from the cross-attention weights
// of a few "alignment heads" of a teacher-forced decoder pass.
//   align_weights_kernel  w = softmax_f(q . k / 8) of chosen heads of one layer
//   align_filter_kernel   standardise over the token axis, median of 7 over
//                         frames, mean over heads
//   align_dtw_kernel      dynamic time warping over -M and the backtrace
// Semantics: include/whisper_amd.h "Token alignment"; numerics and scratch
// sizes: DESIGN.md section 5 "Token alignment (wa_align)".
#include <hip/hip_runtime.h>

#include <cmath>

#include "../wq4_device.hpp"
#include "wa_align.hpp"

namespace wa {

using wq4::floatx16;
using wq4::floatx4;
using wq4::half8;
using wq4::split_f16;

namespace {

// prefill_attention_kernel's constants (wa_kernels.hip): the scores in base 2,
// q and k as f16 pairs of x * 2^5, the scores x 2^10, the lazy reference maximum
constexpr float kAlQScale = 0.125f * 1.4426950408889634f;
constexpr float kAlOpScale = 32.0f, kAlSInv = 1.0f / 1024.0f, kAlLazyMax = 1024.0f;
constexpr int kAlKeys = 64, kAlLd = 72, kAlWaves = 4;

typedef _Float16 al_half2 __attribute__((ext_vector_type(2)));
typedef float al_float2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void al_split2(float a, float b, al_half2& hi, al_half2& lo) {
  hi = __builtin_convertvector((al_float2){a, b}, al_half2);
  const al_float2 r = (al_float2){a, b} - __builtin_convertvector(hi, al_float2);
  lo = __builtin_convertvector(r, al_half2);
}
__device__ __forceinline__ floatx16 al_mfma(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// ------------------------------------------------- attention weights --
// prefill_attention_kernel's score arithmetic (S^T = K Q^T on
// v_mfma_f32_32x32x16_f16, operands f16 pairs at two planes, hi alone at one;
// 32 queries per wave, 64-key tiles in two 32-key sub-tiles; the lazy
// reference maximum; l summed over the sub-tiles with compensated adds), run
// twice over the clip's first F[b] keys: the first walk leaves every query's
// reference m and sum l, the second forms the same scores again (the same
// instructions on the same operands: the same bits) and writes
// exp2(s - m) / l.  Workgroup = 4 waves x 32 rows of one (clip, head of the
// pass), grid (ceil(P / 128), heads, B).  A row's bits depend on its own q,
// the clip's K and F[b] only.
template <int NS>
__global__ __launch_bounds__(64 * kAlWaves, 2) void align_weights_kernel(
    const float* __restrict__ qp, const float* __restrict__ kp, int B, int P, int T, int H,
    const int* __restrict__ pad, const int* __restrict__ Fp, const int* __restrict__ heads, float* __restrict__ w,
    int Fld) {
  constexpr int NW = kAlWaves;
  __shared__ __attribute__((aligned(16))) _Float16 klsb[2][NS][kAlKeys * kAlLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int hp = blockIdx.y, head = heads[hp], b = blockIdx.z;
  const int D = H * 64;
  const int pad_b = pad[b], F = Fp[b];
  const int q0 = blockIdx.x * (32 * NW);
  if (q0 + 32 * NW <= pad_b || F < 1) return;  // pad rows only (workgroup-uniform)
  const int q = q0 + wave * 32 + l32;
  // a pad row or a row past P carries a real row's query (nothing is stored for it)
  const int qrow = min(max(q, pad_b), P - 1);
  const float* kbase = kp + ((size_t)b * H + head) * (size_t)T * 64;

  half8 qb[4][NS];
  {
    const float* qr = qp + ((size_t)b * P + qrow) * D + head * 64;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const floatx4 x0 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh);
      const floatx4 x1 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh + 4);
      half8 hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (j < 4 ? x0[j] : x1[j - 4]) * kAlQScale;
        _Float16 a, c;
        split_f16(v * kAlOpScale, a, c);
        hi[j] = a;
        lo[j] = c;
      }
      qb[ks][0] = hi;
      if constexpr (NS == 2) qb[ks][1] = lo;
    }
  }
  // staging: thread (key tid / 4, dims 16 (tid % 4) + 0..15) of K
  constexpr int EPT = 64 * kAlKeys / (64 * NW);
  constexpr int TPK = 64 / EPT;
  const int skey = tid / TPK, sd = (tid % TPK) * EPT;
  floatx4 kreg[EPT / 4];
  auto fetch = [&](int key0) {
    const int key = key0 + skey;
    const bool ok = key < F;
    const size_t ofs = (size_t)(ok ? key : 0) * 64 + sd;
#pragma unroll
    for (int i = 0; i < EPT / 4; ++i)
      kreg[i] = ok ? *reinterpret_cast<const floatx4*>(kbase + ofs + 4 * i) : floatx4{0.f, 0.f, 0.f, 0.f};
  };
  auto stage = [&](int buf) {
    _Float16(*kls)[kAlKeys * kAlLd] = klsb[buf];
    half8 kh[EPT / 8], kl[EPT / 8];
#pragma unroll
    for (int i = 0; i < EPT; i += 2) {
      al_half2 h2, l2;
      al_split2(kreg[i >> 2][i & 3] * kAlOpScale, kreg[i >> 2][(i & 3) + 1] * kAlOpScale, h2, l2);
      kh[i >> 3][i & 7] = h2[0];
      kh[i >> 3][(i & 7) + 1] = h2[1];
      kl[i >> 3][i & 7] = l2[0];
      kl[i >> 3][(i & 7) + 1] = l2[1];
    }
#pragma unroll
    for (int u = 0; u < EPT / 8; ++u) {
      *reinterpret_cast<half8*>(&kls[0][skey * kAlLd + sd + 8 * u]) = kh[u];
      if constexpr (NS == 2) *reinterpret_cast<half8*>(&kls[NS - 1][skey * kAlLd + sd + 8 * u]) = kl[u];
    }
  };
  // the scores of sub-tile `sub` of the staged tile, keys >= F at -inf
  auto scores = [&](const _Float16(*kls)[kAlKeys * kAlLd], int key0, int sub) {
    floatx16 st;
#pragma unroll
    for (int i = 0; i < 16; ++i) st[i] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int off = (sub * 32 + l32) * kAlLd + 16 * ks + 8 * lh;
      const half8 ah = *reinterpret_cast<const half8*>(&kls[0][off]);
      st = al_mfma(ah, qb[ks][0], st);
      if constexpr (NS == 2) {
        const half8 al = *reinterpret_cast<const half8*>(&kls[1][off]);
        st = al_mfma(al, qb[ks][0], st);
        st = al_mfma(ah, qb[ks][1], st);
      }
    }
    if (key0 + sub * 32 + 32 > F) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = key0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        if (key >= F) st[i] = -INFINITY;
      }
    }
    return st;
  };

  float m = -INFINITY, l = 0.0f, lc = 0.0f;
  float nmn = 0.0f, inv = 0.0f;
  const bool store = q >= pad_b && q < P;
  float* wrow = w + (((size_t)hp * B + b) * P + (store ? q : qrow)) * Fld;
  const int ntile = (F + kAlKeys - 1) / kAlKeys;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    fetch(0);
    stage(0);
    __syncthreads();
    if (ntile > 1) fetch(kAlKeys);
    for (int kt = 0; kt < ntile; ++kt) {
      const int key0 = kt * kAlKeys;
      const _Float16(*kls)[kAlKeys * kAlLd] = klsb[kt & 1];
#pragma unroll
      for (int sub = 0; sub < kAlKeys / 32; ++sub) {
        if (key0 + sub * 32 >= F) continue;  // no key of the clip (workgroup-uniform)
        floatx16 st = scores(kls, key0, sub);
        if (pass == 0) {
          float mx = -INFINITY;
#pragma unroll
          for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[i]);
          mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
          // lazy reference maximum: m moves only when a score exceeds it by more
          // than 1 in base 2, so p = exp2(s - m) lies in (0, 2]; key 0 is in the
          // first sub-tile, so mn is finite
          float mn = fmaxf(m, mx);
          if (m != -INFINITY && mn - m <= kAlLazyMax) mn = m;
          const float alpha = __builtin_amdgcn_exp2f((m - mn) * kAlSInv);
          const float nm = -mn * kAlSInv;
          float rs = 0.0f;
#pragma unroll
          for (int i = 0; i < 16; ++i) rs += __builtin_amdgcn_exp2f(fmaf(st[i], kAlSInv, nm));
          rs += __shfl_xor(rs, 32, 64);
          m = mn;
          l *= alpha;
          lc *= alpha;
          // compensated (two-sum) add of the sub-tile's part
          const float t = l + rs, bp = t - l;
          lc += (l - (t - bp)) + (rs - bp);
          l = t;
        } else if (store) {
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) {
            const int kb = key0 + sub * 32 + 8 * gg + 4 * lh;
            floatx4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_exp2f(fmaf(st[4 * gg + j], kAlSInv, nmn)) * inv;
            if (kb + 3 < F) {
              *reinterpret_cast<floatx4*>(wrow + kb) = o;
            } else {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (kb + j < F) wrow[kb + j] = o[j];
            }
          }
        }
      }
      if (kt + 1 < ntile) {
        stage((kt + 1) & 1);
        if (kt + 2 < ntile) fetch(key0 + 2 * kAlKeys);
      }
      __syncthreads();
    }
    nmn = -m * kAlSInv;
    inv = 1.0f / (l + lc);
  }
}

// ------------------------------- standardise, median of 7, head mean --
// Workgroup = (clip, tile of 58 frames with a 3-frame halo each side: 64
// columns) x 4 row groups.  Per head of the pass: the columns' mean and
// population variance over the clip's n real rows in f64 (row group r sums rows
// r, r + 4, ... counted from pad[b]; the four parts are added in a fixed order,
// so nothing depends on the padding or the batch), z = (w - mean) / std in
// f64 rounded to f32 (std == 0: 0), then every thread takes the median of its
// frame's seven z of a row and adds it into msum.  Halo columns past either end
// of [0, F) are the reflected ones (index -k -> k, F - 1 + k -> F - 1 - k).
constexpr int kFtOut = 58, kFtCols = 64, kFtRG = 4;

__device__ __forceinline__ float median7(float (&v)[7]) {
  // a full sort of seven by compare-exchange: the fourth smallest
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < 6 - a; ++c) {
      const float lo = fminf(v[c], v[c + 1]), hi = fmaxf(v[c], v[c + 1]);
      v[c] = lo;
      v[c + 1] = hi;
    }
  return v[3];
}

__global__ __launch_bounds__(kFtCols* kFtRG) void align_filter_kernel(const float* __restrict__ w, int B, int P,
                                                                      const int* __restrict__ pad,
                                                                      const int* __restrict__ Fp, int n_heads, int Fld,
                                                                      float* __restrict__ msum, int first, int last,
                                                                      float total_heads) {
  __shared__ double part[kFtRG][kFtCols];
  __shared__ double mean_s[kFtCols], inv_s[kFtCols];
  __shared__ int col_s[kFtCols];
  const int tid = threadIdx.x, s = tid % kFtCols, r = tid / kFtCols;
  const int b = blockIdx.y, f0 = blockIdx.x * kFtOut;
  const int F = Fp[b], pad_b = pad[b], n = P - pad_b;
  if (f0 >= F || n < 1) return;  // workgroup-uniform
  int g = f0 - 3 + s;
  if (g < 0) g = -g;
  if (g > F - 1) g = 2 * (F - 1) - g;
  g = min(max(g, 0), F - 1);  // columns no frame of the tile uses
  if (r == 0) col_s[s] = g;
  const int f = f0 + s - 3;
  const bool out = s >= 3 && s < 3 + kFtOut && f < F;
  for (int h = 0; h < n_heads; ++h) {
    const float* wb = w + (((size_t)h * B + b) * P + pad_b) * Fld;
    double acc = 0.0;
    for (int i = r; i < n; i += kFtRG) acc += (double)wb[(size_t)i * Fld + g];
    part[r][s] = acc;
    __syncthreads();
    const double mean = ((part[0][s] + part[1][s]) + (part[2][s] + part[3][s])) / (double)n;
    __syncthreads();
    acc = 0.0;
    for (int i = r; i < n; i += kFtRG) {
      const double d = (double)wb[(size_t)i * Fld + g] - mean;
      acc += d * d;
    }
    part[r][s] = acc;
    __syncthreads();
    if (r == 0) {
      const double var = ((part[0][s] + part[1][s]) + (part[2][s] + part[3][s])) / (double)n;
      mean_s[s] = mean;
      inv_s[s] = var > 0.0 ? 1.0 / sqrt(var) : 0.0;
    }
    __syncthreads();
    if (out) {
      int c[7];
      double mu[7], is[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        c[k] = col_s[s - 3 + k];
        mu[k] = mean_s[s - 3 + k];
        is[k] = inv_s[s - 3 + k];
      }
      const bool set = first && h == 0, fin = last && h == n_heads - 1;
      for (int i = r; i < n; i += kFtRG) {
        const float* wr = wb + (size_t)i * Fld;
        float z[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) z[k] = (float)(((double)wr[c[k]] - mu[k]) * is[k]);
        const float med = median7(z);
        float* dst = msum + ((size_t)b * P + pad_b + i) * Fld + f;
        float a = set ? med : *dst + med;
        if (fin) a = a / total_heads;
        *dst = a;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ DTW --
// One workgroup per clip; thread t owns row i = t + 1 of the (N + 1) x (F + 1)
// cost table and walks the anti-diagonals d = i + j with the rest, three
// diagonals of cost in LDS indexed by i.  f32, one add per cell:
//   c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]
//   trace 0 if c0 < c1 && c0 < c2, else 1 if c1 < c0 && c1 < c2, else 2
// so the path is bit-determined by x.  A thread reads its row of x four frames
// at a time.  Then lane 0 walks back from (N, F).
constexpr int kDtwThreads = 512;

__global__ __launch_bounds__(kDtwThreads) void align_dtw_kernel(const float* __restrict__ x, long x_bs, int x_ld,
                                                                const int* __restrict__ row0,
                                                                const int* __restrict__ Np,
                                                                const int* __restrict__ Fp, int negate,
                                                                uint8_t* __restrict__ trace, int n_ld, int f_ld,
                                                                int* __restrict__ jump, int jump_ld) {
  __shared__ float cst[3][kDtwThreads];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int N = Np[b], F = Fp[b];
  if (N < 1 || F < 1 || N > n_ld || F > f_ld || N >= kDtwThreads) return;  // workgroup-uniform; the host checks
  const int tld = f_ld + 1;
  uint8_t* tr = trace + (size_t)b * (n_ld + 1) * tld;
  for (int k = 0; k < 3; ++k) cst[k][tid] = INFINITY;
  for (int j = tid; j <= F; j += kDtwThreads) tr[j] = 2;
  __syncthreads();
  for (int i = tid; i <= N; i += kDtwThreads) tr[(size_t)i * tld] = 1;
  if (tid == 0) cst[0][0] = 0.0f;
  __syncthreads();
  const int i = tid + 1;
  const bool live = i <= N;
  const float* xr = x + (size_t)b * x_bs + (size_t)(row0[b] + (live ? tid : 0)) * x_ld;
  float xv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int d = 1; d <= N + F; ++d) {
    float* cur = cst[d % 3];
    const float* p1 = cst[(d + 2) % 3];
    const float* p2 = cst[(d + 1) % 3];
    if (tid == 0) cur[0] = INFINITY;
    const int j = d - i;
    if (live && j == 0) cur[i] = INFINITY;
    if (live && j >= 1 && j <= F) {
      const int e = j - 1;
      if ((e & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = e + k < F ? xr[e + k] : 0.0f;
      }
      const float xe = negate ? -xv[e & 3] : xv[e & 3];
      const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
      float c;
      uint8_t t;
      if (c0 < c1 && c0 < c2) {
        c = c0;
        t = 0;
      } else if (c1 < c0 && c1 < c2) {
        c = c1;
        t = 1;
      } else {
        c = c2;
        t = 2;
      }
      cur[i] = xe + c;
      tr[(size_t)i * tld + j] = t;
    }
    __syncthreads();
  }
  __threadfence_block();
  if (tid == 0) {
    int* jp = jump + (size_t)b * jump_ld;
    int bi = N, bj = F;
    while (bi > 0 || bj > 0) {
      if (bi > 0 && bj > 0) jp[bi - 1] = bj - 1;  // the last visit of a row is its first path point
      const int t = bi == 0 ? 2 : bj == 0 ? 1 : tr[(size_t)bi * tld + bj];
      if (t == 0) {
        --bi;
        --bj;
      } else if (t == 1) {
        --bi;
      } else {
        --bj;
      }
    }
  }
}

}  // namespace

hipError_t launch_align_weights(const float* q, const float* k, int B, int P, int T, int H, const int* pad,
                                const int* F, const int* heads, int n_heads, float* w, int Fld, int ns,
                                hipStream_t st) {
  if (B < 1 || P < 1 || T < 1 || H < 1 || n_heads < 1 || n_heads > kAlignHeadsPerPass || Fld < T || Fld % 4 != 0 || !q ||
      !k || !pad || !F || !heads || !w)
    return hipErrorInvalidValue;
  const dim3 grid((P + 32 * kAlWaves - 1) / (32 * kAlWaves), n_heads, B), block(64 * kAlWaves);
  if (ns == 2)
    hipLaunchKernelGGL((align_weights_kernel<2>), grid, block, 0, st, q, k, B, P, T, H, pad, F, heads, w, Fld);
  else
    hipLaunchKernelGGL((align_weights_kernel<1>), grid, block, 0, st, q, k, B, P, T, H, pad, F, heads, w, Fld);
  return hipGetLastError();
}

hipError_t launch_align_filter(const float* w, int B, int P, const int* pad, const int* F, int n_heads, int Fld,
                               float* msum, bool first, bool last, int total_heads, hipStream_t st) {
  if (B < 1 || P < 1 || n_heads < 1 || n_heads > kAlignHeadsPerPass || total_heads < 1 || !w || !pad || !F || !msum)
    return hipErrorInvalidValue;
  const dim3 grid((Fld + kFtOut - 1) / kFtOut, B), block(kFtCols * kFtRG);
  hipLaunchKernelGGL(align_filter_kernel, grid, block, 0, st, w, B, P, pad, F, n_heads, Fld, msum, first ? 1 : 0,
                     last ? 1 : 0, (float)total_heads);
  return hipGetLastError();
}

hipError_t launch_align_dtw(const float* x, long x_bs, int x_ld, const int* row0, const int* N, const int* F, int B,
                            bool negate, uint8_t* trace, int n_ld, int f_ld, int* jump, int jump_ld, hipStream_t st) {
  if (B < 1 || n_ld < 1 || n_ld >= kDtwThreads || f_ld < 1 || jump_ld < n_ld || !x || !row0 || !N || !F || !trace ||
      !jump)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_dtw_kernel, dim3(B), dim3(kDtwThreads), 0, st, x, x_bs, x_ld, row0, N, F, negate ? 1 : 0,
                     trace, n_ld, f_ld, jump, jump_ld);
  return hipGetLastError();
}

}  // namespace wa
