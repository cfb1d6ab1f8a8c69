// wa_kernels.hip -- gfx950 kernels of the Whisper model around the Q4 path.
//
// Reference semantics (zerr0o/whisper-burn):
//   LayerNorm        src/model/layers.rs:12-32   (eps 1e-5, biased variance)
//   GELU (tanh)      src/model/layers.rs:35-41
//   Conv1D + GELU    src/model/layers.rs:62-132, encoder.rs:87-106
//   SDPA             src/model/attention.rs:243-298 (scores / sqrt(64),
//                    causal mask only when q_len > 1, softmax over keys)
//   KV-cached decode src/model/attention.rs:93-125, decoder.rs:77-112
// (the logits and the token pick: wa_pick.hip)
// Every product here is f32 x f32 (v_mfma_f32_32x32x2_f32: exact products,
// f32 accumulation) or f32 VALU; only the operands handed to the Q4 GEMMs
// are written in the f16 hi/lo A-tiled layout (wq4_layout.hpp).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdlib>

#include "../wq4_device.hpp"
#include "../wq4_lnmath.hpp"
#include "wa_beam.hpp"
#include "wa_kernels.hpp"

namespace wa {

using wq4::floatx16;
using wq4::floatx4;
using wq4::half8;

// attention scores scaled by 1/sqrt(64) * log2(e) (attention.rs:262): the
// softmax runs in base 2, one v_exp_f32 (2^x) per exponential
constexpr float kEaQScale = 0.125f * 1.4426950408889634f;
// Operand scales of the f16-pair MFMAs (the MFMAs flush f16 subnormal inputs,
// wq4_device.hpp split_act): q / 8 (base 2), k and v enter as x * 2^5 (|x| <
// 2047), the softmax weights p in (0, 2] (lazy reference maximum) as p * 2^14
// (<= 32768 < 65504); the scores come out x 2^10 and the output x 2^19 --
// undone in f32, exactly.
constexpr float kQKScale = 32.0f, kSInv = 1.0f / 1024.0f;
constexpr float kPScale = 16384.0f, kPVInv = 1.0f / (16384.0f * 32.0f);
constexpr float kEaLazyMax = 1024.0f;  // 1.0 in base-2 units x 2^10 (the scores' operand scale)
// the conv front-end: input x 2^4, weights x 2^10 (|w| < 64), product x 2^-14
constexpr float kCvAScale = 16.0f, kCvBScale = 1024.0f, kCvInv = 1.0f / (16.0f * 1024.0f);

using wq4::kLnMaxV;
using wq4::wave_sum;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

using wq4::atile_store4;
using wq4::attn_store4;
using wq4::kbp_of;
using wq4::split_f16;



// ------------------------------------ encoder attention, f16x2 MFMA --
// Encoder self-attention (attention.rs:243-298, non-causal; scores use q / 8,
// an exact power-of-two scaling of attention.rs:266-267's division), flash
// style: products on v_mfma_f32_32x32x16_f16 with every operand an
// exact-to-2^-22 f16 pair (x = hi + lo; hi*hi + lo*hi + hi*lo, f32
// accumulation -- the arithmetic of the Q4 GEMMs).  Both products are
// computed transposed (S^T = K Q^T, O^T = V^T P^T) so that a lane owns one
// query and the online-softmax statistics are lane-local.  Workgroup = 8
// waves x 32 queries of one (clip, head); 64-key tiles of K and V are converted to f16
// pairs into LDS (row stride 72 halves: conflict-free b128 and transposed
// reads), the next tile's f32 loads in flight meanwhile.
//   S^T = K Q^T   A = K (m = key, k = dim) ds_read_b128; B = Q^T from registers
//   O^T += V^T P^T  A = V^T via ds_read_b64_tr_b16 of row-major V, in the key
//                 order of the S^T accumulator; B = P^T = that accumulator.
typedef _Float16 ea_half4 __attribute__((ext_vector_type(4)));
typedef __fp16 ea_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
__device__ __forceinline__ ea_half4 ea_tr4(const _Float16* p) {
  return __builtin_bit_cast(ea_half4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                                          (__attribute__((address_space(3))) ea_fp16x4*)(p)));
}
__device__ __forceinline__ floatx16 ea_mfma(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Two split_f16 at once: hi = RNE(x) of both by one v_cvt_pk_f16_f32, the
// exact remainders x - hi by one packed subtract, lo = their RNE -- five
// instructions per pair where two split_f16 take eight; the same bits.
typedef _Float16 ea_half2 __attribute__((ext_vector_type(2)));
typedef float ea_float2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2(float a, float b, ea_half2& hi, ea_half2& lo) {
  hi = __builtin_convertvector((ea_float2){a, b}, ea_half2);
  const ea_float2 r = (ea_float2){a, b} - __builtin_convertvector(hi, ea_float2);
  lo = __builtin_convertvector(r, ea_half2);
}

constexpr int kEaKeys = 64;  // keys per LDS tile
constexpr int kEaLd = 72;    // LDS row stride (halves)

// Registers held to 128 (4 waves per SIMD: two 8-wave workgroups per CU,
// one's staging beside the other's MFMAs); WA_EA_WAVES: A/B builds.
#ifndef WA_EA_WAVES
#define WA_EA_WAVES 4
#endif
template <int NS, int NW>
__global__ __launch_bounds__(64 * NW, WA_EA_WAVES) void encoder_attention_f16_kernel(const float* __restrict__ qkv,
                                                                                    int T, int H,
                                                                                    _Float16* __restrict__ tiled,
                                                                                    float* __restrict__ out32) {
  // two tile buffers: tile kt + 1 is staged into the other one while tile
  // kt is read, one barrier per tile
  __shared__ __attribute__((aligned(16))) _Float16 klsb[2][NS][kEaKeys * kEaLd];
  __shared__ __attribute__((aligned(16))) _Float16 vlsb[2][NS][kEaKeys * kEaLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64, ld = 3 * D;
  const float* base = qkv + (size_t)b * T * ld;
  const int q = blockIdx.x * (32 * NW) + wave * 32 + l32;

  // Q^T operand (k = dim, n = query): lane (query l32, dims 16 ks + 8 lh + 0..7), scaled by 1/8 (exact)
  half8 qb[4][NS];
  {
    const float* qr = base + (size_t)(q < T ? q : 0) * ld + head * 64;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const floatx4 x0 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh);
      const floatx4 x1 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh + 4);
      half8 hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // q / 8 * log2(e): the scores come out in base-2 units, so the
        // softmax exponentials are single v_exp_f32 (2^x) instructions
        const float v = q < T ? (j < 4 ? x0[j] : x1[j - 4]) * kEaQScale : 0.0f;
        _Float16 a, c;
        split_f16(v * kQKScale, a, c);
        hi[j] = a;
        lo[j] = c;
      }
      qb[ks][0] = hi;
      if constexpr (NS == 2) qb[ks][1] = lo;
    }
  }
  // staging: thread (key tid / TPK, dims EPT (tid % TPK) + 0..EPT-1) of K and V
  constexpr int EPT = 64 * kEaKeys / (64 * NW);  // elements per thread and tensor (16 or 8)
  constexpr int TPK = 64 / EPT;                  // threads per key
  const int skey = tid / TPK, sd = (tid % TPK) * EPT;
  floatx4 kreg[EPT / 4], vreg[EPT / 4];
  auto fetch = [&](int key0) {
    const int key = key0 + skey;
    const bool ok = key < T;
    const float* kr = base + (size_t)(ok ? key : 0) * ld + D + head * 64 + sd;
#pragma unroll
    for (int i = 0; i < EPT / 4; ++i) {
      kreg[i] = ok ? *reinterpret_cast<const floatx4*>(kr + 4 * i) : floatx4{0.f, 0.f, 0.f, 0.f};
      vreg[i] = ok ? *reinterpret_cast<const floatx4*>(kr + D + 4 * i) : floatx4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stage = [&](int buf) {
    _Float16(*kls)[kEaKeys * kEaLd] = klsb[buf];
    _Float16(*vls)[kEaKeys * kEaLd] = vlsb[buf];
    half8 kh[EPT / 8], kl[EPT / 8], vh[EPT / 8], vl[EPT / 8];
#pragma unroll
    for (int i = 0; i < EPT; i += 2) {
      ea_half2 h2, l2;
      split2(kreg[i >> 2][i & 3] * kQKScale, kreg[i >> 2][(i & 3) + 1] * kQKScale, h2, l2);
      kh[i >> 3][i & 7] = h2[0];
      kh[i >> 3][(i & 7) + 1] = h2[1];
      kl[i >> 3][i & 7] = l2[0];
      kl[i >> 3][(i & 7) + 1] = l2[1];
      split2(vreg[i >> 2][i & 3] * kQKScale, vreg[i >> 2][(i & 3) + 1] * kQKScale, h2, l2);
      vh[i >> 3][i & 7] = h2[0];
      vh[i >> 3][(i & 7) + 1] = h2[1];
      vl[i >> 3][i & 7] = l2[0];
      vl[i >> 3][(i & 7) + 1] = l2[1];
    }
#pragma unroll
    for (int u = 0; u < EPT / 8; ++u) {
      *reinterpret_cast<half8*>(&kls[0][skey * kEaLd + sd + 8 * u]) = kh[u];
      *reinterpret_cast<half8*>(&vls[0][skey * kEaLd + sd + 8 * u]) = vh[u];
      if constexpr (NS == 2) {
        *reinterpret_cast<half8*>(&kls[NS - 1][skey * kEaLd + sd + 8 * u]) = kl[u];
        *reinterpret_cast<half8*>(&vls[NS - 1][skey * kEaLd + sd + 8 * u]) = vl[u];
      }
    }
  };

  float m = -INFINITY, l = 0.0f;
  floatx16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    o[0][i] = 0.0f;
    o[1][i] = 0.0f;
  }
  // transposed-read geometry: 16-lane group g = lane / 16 covers dims
  // 16 (g & 1) + 0..15 and keys 4 (g >> 1) + 0..3 (+ 8): the S^T
  // accumulator's key order for lanes < 32 / >= 32
  const int g = lane >> 4, gi = lane & 15;
  const int trow = 4 * (g >> 1) + (gi >> 2), tcol = 16 * (g & 1) + 4 * (gi & 3);
  const int ntile = (T + kEaKeys - 1) / kEaKeys;
  fetch(0);
  stage(0);
  __syncthreads();
  if (ntile > 1) fetch(kEaKeys);  // tile 1 in flight during tile 0
  for (int kt = 0; kt < ntile; ++kt) {
    const int key0 = kt * kEaKeys;
    const _Float16(*kls)[kEaKeys * kEaLd] = klsb[kt & 1];
    const _Float16(*vls)[kEaKeys * kEaLd] = vlsb[kt & 1];
#pragma unroll
    for (int sub = 0; sub < kEaKeys / 32; ++sub) {
      floatx16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int off = (sub * 32 + l32) * kEaLd + 16 * ks + 8 * lh;
        const half8 ah = *reinterpret_cast<const half8*>(&kls[0][off]);
        st = ea_mfma(ah, qb[ks][0], st);
        if constexpr (NS == 2) {
          const half8 al = *reinterpret_cast<const half8*>(&kls[1][off]);
          st = ea_mfma(al, qb[ks][0], st);
          st = ea_mfma(ah, qb[ks][1], st);
        }
      }
      // online softmax of query l32 over these 32 keys (16 here, 16 in lane ^ 32)
      if (key0 + sub * 32 + 32 > T) {  // only the last tile holds keys past T (wave-uniform)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = key0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          if (key >= T) st[i] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // lazy reference maximum (as the decoder cross-attention's softmax_entry):
      // the running reference m only moves when the tile's maximum exceeds
      // it by more than 1 (base 2), so p <= 2 and most tiles need no rescale
      // of o (alpha == 1 exactly, skipped when the whole wave agrees); any
      // reference gives the same softmax.  Scores (and m) carry the 2^10
      // operand scale.
      float mn = fmaxf(m, mx);
      if (m != -INFINITY && mn - m <= kEaLazyMax) mn = m;
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * kSInv);  // exp2(-inf) = 0; 1 when mn == m
      float rs = 0.0f;
      // mn is finite: the first 32 keys of tile 0 hold key 0 (< T)
      const float nmn = -mn * kSInv;  // exact (power-of-two scale)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[i] = __builtin_amdgcn_exp2f(fmaf(st[i], kSInv, nmn));
        rs += st[i];
      }
      rs += __shfl_xor(rs, 32, 64);
      l = l * alpha + rs;
      m = mn;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          o[0][i] *= alpha;
          o[1][i] *= alpha;
        }
      }
      // P^T operands: MFMA t takes accumulator registers 8 t .. 8 t + 7.
      // p in (0, 2] is split at p * 2^14 (exact scaling; undone at the end)
      // so that the lo part of a small p stays a normal f16: 22 bits for
      // every p >= 2^-17 instead of an absolute 2^-24 floor
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        half8 ph, pl;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          ea_half2 h2, l2;
          split2(st[8 * t + j] * kPScale, st[8 * t + j + 1] * kPScale, h2, l2);
          ph[j] = h2[0];
          ph[j + 1] = h2[1];
          pl[j] = l2[0];
          pl[j + 1] = l2[1];
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          half8 va[NS];
#pragma unroll
          for (int pp = 0; pp < NS; ++pp) {
            const _Float16* vb = &vls[pp][(sub * 32 + 16 * t + trow) * kEaLd + dt * 32 + tcol];
            const ea_half4 x0 = ea_tr4(vb);
            const ea_half4 x1 = ea_tr4(vb + 8 * kEaLd);
            va[pp] = half8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
          }
          o[dt] = ea_mfma(va[0], ph, o[dt]);
          if constexpr (NS == 2) {
            o[dt] = ea_mfma(va[1], ph, o[dt]);
            o[dt] = ea_mfma(va[0], pl, o[dt]);
          }
        }
      }
    }
    // the next tile into the other buffer (its last readers, tile kt - 1,
    // passed the barrier below one iteration ago), then the one after it
    // into registers
    if (kt + 1 < ntile) {
      stage((kt + 1) & 1);
      if (kt + 2 < ntile) fetch(key0 + 2 * kEaKeys);
    }
    __syncthreads();
  }
  if (q < T) {
    const int row = b * T + q;
    const int kbp = kbp_of(D);
    const float inv = (1.0f / l) * kPVInv;  // exact power-of-two rescale of 1 / l
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int d = dt * 32 + 8 * gg + 4 * lh;
        attn_store4<NS>(tiled, out32, H * 64, row, head * 64 + d, kbp, o[dt][4 * gg] * inv,
                        o[dt][4 * gg + 1] * inv, o[dt][4 * gg + 2] * inv, o[dt][4 * gg + 3] * inv);
      }
  }
}

hipError_t launch_encoder_attention(const float* qkv, int B, int T, int H, _Float16* tiled, int ns,
                                    hipStream_t st, float* out32) {
  // 8 waves x 32 queries per workgroup; when that grid leaves most CUs idle
  // (one or two clips: 120 / 240 workgroups at Large-V3) 4 waves, twice the
  // workgroups (each query's arithmetic is the same either way)
  const bool few = (int64_t)B * H * ((T + 255) / 256) < 256;
  if (few) {
    const dim3 g4((T + 127) / 128, H, B);
    if (ns == 2)
      hipLaunchKernelGGL((encoder_attention_f16_kernel<2, 4>), g4, dim3(256), 0, st, qkv, T, H, tiled, out32);
    else
      hipLaunchKernelGGL((encoder_attention_f16_kernel<1, 4>), g4, dim3(256), 0, st, qkv, T, H, tiled, out32);
    return hipGetLastError();
  }
  const dim3 g2((T + 255) / 256, H, B);
  if (ns == 2)
    hipLaunchKernelGGL((encoder_attention_f16_kernel<2, 8>), g2, dim3(512), 0, st, qkv, T, H, tiled, out32);
  else
    hipLaunchKernelGGL((encoder_attention_f16_kernel<1, 8>), g2, dim3(512), 0, st, qkv, T, H, tiled, out32);
  return hipGetLastError();
}

// ------------------------------------ prefill attention, f16x2 MFMA --
// The decoder's attention over a whole prompt of P rows per clip (wa_prompt.cpp):
// encoder_attention_f16_kernel's arithmetic -- the same operand scales, the
// same 64-key tiles in two 32-key sub-tiles, the same lazy reference maximum
// -- over strided sources, with one difference: the sub-tiles' parts of l and
// o are added with compensated f32 sums (1500 keys are 47 sub-tiles, where the
// encoder's bound was set on up to 9), so its error bound holds at every T.  Query row t of clip b is
// at q + b * q_bs + t * q_ld + head * 64, key / value j of (b, head) at k / v
// + b * kv_bs + head * kv_hs + j * kv_ld.
//   CAUSAL (self-attention over the qkv rows of right-aligned prompts): clip
//     b's rows are [pad[b], P); row t attends keys [pad[b], t].  Keys are
//     tiled from pad[b], so a clip's bits are those of an unpadded clip of
//     P - pad[b] rows: a masked key adds exact zeros, and a sub-tile no query
//     of the wave sees is skipped.  The workgroup also copies K and V of its
//     rows into the head-major caches ck / cv [clip][head][ctx][64] at slots
//     pad[b] .. P - 1 (what the decode step's kernel appends).  Pad rows are
//     written as zeros.
//   otherwise (cross-attention over head-major K / V): every row attends keys
//     [0, T); pad is not read.
// (A kernel of its own, not a mode of the encoder's: the encoder's code, and so
// its registers and timing, stay what they were.)
// Workgroup = 4 waves x 32 queries of one (clip, head), grid (ceil(P / 128), H, B);
// the two tile buffers (72 KiB at two planes) let two workgroups share a CU:
// 2 waves per SIMD, so registers are not held below 256.
constexpr int kPfWaves = 4;

template <int NS, bool CAUSAL>
__global__ __launch_bounds__(64 * kPfWaves, 2) void prefill_attention_kernel(
    const float* __restrict__ qp, long q_ld, long q_bs, const float* __restrict__ kp, const float* __restrict__ vp,
    long kv_ld, long kv_hs, long kv_bs, int P, int T, const int* __restrict__ pad, int H, float* __restrict__ ck,
    float* __restrict__ cv, int ctx, _Float16* __restrict__ tiled, float* __restrict__ out32) {
  constexpr int NW = kPfWaves;
  __shared__ __attribute__((aligned(16))) _Float16 klsb[2][NS][kEaKeys * kEaLd];
  __shared__ __attribute__((aligned(16))) _Float16 vlsb[2][NS][kEaKeys * kEaLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int head = blockIdx.y, b = blockIdx.z;
  const int D = H * 64;
  const int pad_b = CAUSAL ? pad[b] : 0;
  const int q0 = blockIdx.x * (32 * NW);
  const int q = q0 + wave * 32 + l32;
  const int kbp = kbp_of(D);
  const float* kbase = kp + (size_t)b * kv_bs + (size_t)head * kv_hs + (CAUSAL ? (size_t)pad_b * kv_ld : 0);
  const float* vbase = vp + (size_t)b * kv_bs + (size_t)head * kv_hs + (CAUSAL ? (size_t)pad_b * kv_ld : 0);
  // the last row of this workgroup, and the keys (counted from pad_b) it reaches
  const int qlast = min(q0 + 32 * NW, P) - 1;
  const int nkeys = CAUSAL ? qlast - pad_b + 1 : T;
  auto store_zero = [&]() {
    if (q < P) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg)
          attn_store4<NS>(tiled, out32, D, b * P + q, head * 64 + dt * 32 + 8 * gg + 4 * lh, kbp, 0.f, 0.f, 0.f, 0.f);
    }
  };
  if (nkeys <= 0) {  // pad rows only (workgroup-uniform)
    store_zero();
    return;
  }
  if constexpr (CAUSAL) {
    if (ck) {  // K / V of this workgroup's real rows into the caches, bit for bit
      for (int e = tid; e < 32 * NW * 16; e += 64 * NW) {
        const int t = q0 + (e >> 4), s4 = (e & 15) * 4;
        if (t >= pad_b && t < P) {
          const size_t src = (size_t)b * kv_bs + (size_t)head * kv_hs + (size_t)t * kv_ld + s4;
          const size_t dst = (((size_t)b * H + head) * ctx + t) * 64 + s4;
          *reinterpret_cast<floatx4*>(ck + dst) = *reinterpret_cast<const floatx4*>(kp + src);
          *reinterpret_cast<floatx4*>(cv + dst) = *reinterpret_cast<const floatx4*>(vp + src);
        }
      }
    }
  }
  // the row whose query this lane carries: a pad row or a row past P carries a
  // real row's (its result is not stored), so every lane's softmax is finite
  const int qrow = min(max(q, pad_b), P - 1);
  const int kend = CAUSAL ? qrow - pad_b + 1 : T;  // this lane's keys: [0, kend) from pad_b
  // the wave's: the sub-tiles at or past it are skipped (wave-uniform)
  const int wave_kend = CAUSAL ? min(max(q0 + wave * 32 + 31, pad_b), P - 1) - pad_b + 1 : T;

  // range tier 3 (f32 output rows): values past the pair's |x| < 2047 enter at
  // a smaller power of two, chosen from the largest |v| of the (clip, head)'s
  // own keys -- exact, and the same for every workgroup of the clip
  float vscale = kQKScale, pvinv = kPVInv;
  if (out32) {
    __shared__ float vmax_s[NW];
    const int nall = CAUSAL ? P - pad_b : T;
    float mx = 0.0f;
    for (int e = tid; e < nall * 16; e += 64 * NW) {
      const floatx4 x = *reinterpret_cast<const floatx4*>(vbase + (size_t)(e >> 4) * kv_ld + (e & 15) * 4);
      mx = fmaxf(fmaxf(mx, fmaxf(fabsf(x[0]), fabsf(x[1]))), fmaxf(fabsf(x[2]), fabsf(x[3])));
    }
    mx = wave_max(mx);
    if (lane == 0) vmax_s[wave] = mx;
    __syncthreads();
    mx = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) mx = fmaxf(mx, vmax_s[w]);
    if (mx >= 2047.0f && mx < INFINITY) vscale = ldexpf(1.0f, 14 - ilogbf(mx));  // max |v| * vscale < 2^15
    pvinv = 1.0f / (kPScale * vscale);
  }

  half8 qb[4][NS];
  {
    const float* qr = qp + (size_t)b * q_bs + (size_t)qrow * q_ld + head * 64;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const floatx4 x0 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh);
      const floatx4 x1 = *reinterpret_cast<const floatx4*>(qr + 16 * ks + 8 * lh + 4);
      half8 hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (j < 4 ? x0[j] : x1[j - 4]) * kEaQScale;
        _Float16 a, c;
        split_f16(v * kQKScale, a, c);
        hi[j] = a;
        lo[j] = c;
      }
      qb[ks][0] = hi;
      if constexpr (NS == 2) qb[ks][1] = lo;
    }
  }
  // staging: thread (key tid / TPK, dims EPT (tid % TPK) + 0..EPT-1) of K and V
  constexpr int EPT = 64 * kEaKeys / (64 * NW);
  constexpr int TPK = 64 / EPT;
  const int skey = tid / TPK, sd = (tid % TPK) * EPT;
  floatx4 kreg[EPT / 4], vreg[EPT / 4];
  auto fetch = [&](int key0) {
    const int key = key0 + skey;
    const bool ok = key < nkeys;
    const size_t ofs = (size_t)(ok ? key : 0) * kv_ld + sd;
#pragma unroll
    for (int i = 0; i < EPT / 4; ++i) {
      kreg[i] = ok ? *reinterpret_cast<const floatx4*>(kbase + ofs + 4 * i) : floatx4{0.f, 0.f, 0.f, 0.f};
      vreg[i] = ok ? *reinterpret_cast<const floatx4*>(vbase + ofs + 4 * i) : floatx4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stage = [&](int buf) {
    _Float16(*kls)[kEaKeys * kEaLd] = klsb[buf];
    _Float16(*vls)[kEaKeys * kEaLd] = vlsb[buf];
    half8 kh[EPT / 8], kl[EPT / 8], vh[EPT / 8], vl[EPT / 8];
#pragma unroll
    for (int i = 0; i < EPT; i += 2) {
      ea_half2 h2, l2;
      split2(kreg[i >> 2][i & 3] * kQKScale, kreg[i >> 2][(i & 3) + 1] * kQKScale, h2, l2);
      kh[i >> 3][i & 7] = h2[0];
      kh[i >> 3][(i & 7) + 1] = h2[1];
      kl[i >> 3][i & 7] = l2[0];
      kl[i >> 3][(i & 7) + 1] = l2[1];
      split2(vreg[i >> 2][i & 3] * vscale, vreg[i >> 2][(i & 3) + 1] * vscale, h2, l2);
      vh[i >> 3][i & 7] = h2[0];
      vh[i >> 3][(i & 7) + 1] = h2[1];
      vl[i >> 3][i & 7] = l2[0];
      vl[i >> 3][(i & 7) + 1] = l2[1];
    }
#pragma unroll
    for (int u = 0; u < EPT / 8; ++u) {
      *reinterpret_cast<half8*>(&kls[0][skey * kEaLd + sd + 8 * u]) = kh[u];
      *reinterpret_cast<half8*>(&vls[0][skey * kEaLd + sd + 8 * u]) = vh[u];
      if constexpr (NS == 2) {
        *reinterpret_cast<half8*>(&kls[NS - 1][skey * kEaLd + sd + 8 * u]) = kl[u];
        *reinterpret_cast<half8*>(&vls[NS - 1][skey * kEaLd + sd + 8 * u]) = vl[u];
      }
    }
  };

  // l and o are sums over up to 47 sub-tiles (T = 1500): each sub-tile's part
  // is formed on its own and added with a compensated (two-sum) f32 add, lc /
  // oc the running compensations, so the sums' rounding does not grow with T
  float m = -INFINITY, l = 0.0f, lc = 0.0f;
  floatx16 o[2], oc[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    o[0][i] = 0.0f;
    o[1][i] = 0.0f;
    oc[0][i] = 0.0f;
    oc[1][i] = 0.0f;
  }
  auto two_sum = [](float& s, float& c, float x) {
    const float t = s + x, bp = t - s;
    c += (s - (t - bp)) + (x - bp);
    s = t;
  };
  const int g = lane >> 4, gi = lane & 15;
  const int trow = 4 * (g >> 1) + (gi >> 2), tcol = 16 * (g & 1) + 4 * (gi & 3);
  const int ntile = (nkeys + kEaKeys - 1) / kEaKeys;
  fetch(0);
  stage(0);
  __syncthreads();
  if (ntile > 1) fetch(kEaKeys);
  for (int kt = 0; kt < ntile; ++kt) {
    const int key0 = kt * kEaKeys;
    const _Float16(*kls)[kEaKeys * kEaLd] = klsb[kt & 1];
    const _Float16(*vls)[kEaKeys * kEaLd] = vlsb[kt & 1];
#pragma unroll
    for (int sub = 0; sub < kEaKeys / 32; ++sub) {
      if (key0 + sub * 32 >= wave_kend) continue;  // no query of this wave sees these keys
      floatx16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.0f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int off = (sub * 32 + l32) * kEaLd + 16 * ks + 8 * lh;
        const half8 ah = *reinterpret_cast<const half8*>(&kls[0][off]);
        st = ea_mfma(ah, qb[ks][0], st);
        if constexpr (NS == 2) {
          const half8 al = *reinterpret_cast<const half8*>(&kls[1][off]);
          st = ea_mfma(al, qb[ks][0], st);
          st = ea_mfma(ah, qb[ks][1], st);
        }
      }
      if (CAUSAL || key0 + sub * 32 + 32 > T) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = key0 + sub * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
          if (key >= kend) st[i] = -INFINITY;
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, st[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // lazy reference maximum, as the encoder's kernel; a sub-tile wholly
      // masked for this lane leaves m, l and o as they are (alpha 1, p 0)
      float mn = fmaxf(m, mx);
      if (m != -INFINITY && mn - m <= kEaLazyMax) mn = m;
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * kSInv);
      float rs = 0.0f;
      // mn is finite: key 0 is visible to every lane (kend >= 1) and in the first sub-tile
      const float nmn = -mn * kSInv;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        st[i] = __builtin_amdgcn_exp2f(fmaf(st[i], kSInv, nmn));
        rs += st[i];
      }
      rs += __shfl_xor(rs, 32, 64);
      m = mn;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
        l *= alpha;
        lc *= alpha;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          o[0][i] *= alpha;
          o[1][i] *= alpha;
          oc[0][i] *= alpha;
          oc[1][i] *= alpha;
        }
      }
      two_sum(l, lc, rs);
      floatx16 od[2];  // this sub-tile's P V
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        od[0][i] = 0.0f;
        od[1][i] = 0.0f;
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        half8 ph, pl;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          ea_half2 h2, l2;
          split2(st[8 * t + j] * kPScale, st[8 * t + j + 1] * kPScale, h2, l2);
          ph[j] = h2[0];
          ph[j + 1] = h2[1];
          pl[j] = l2[0];
          pl[j + 1] = l2[1];
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          half8 va[NS];
#pragma unroll
          for (int pp = 0; pp < NS; ++pp) {
            const _Float16* vb = &vls[pp][(sub * 32 + 16 * t + trow) * kEaLd + dt * 32 + tcol];
            const ea_half4 x0 = ea_tr4(vb);
            const ea_half4 x1 = ea_tr4(vb + 8 * kEaLd);
            va[pp] = half8{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
          }
          od[dt] = ea_mfma(va[0], ph, od[dt]);
          if constexpr (NS == 2) {
            od[dt] = ea_mfma(va[1], ph, od[dt]);
            od[dt] = ea_mfma(va[0], pl, od[dt]);
          }
        }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {  // two_sum, element-wise
        const floatx16 t = o[dt] + od[dt], bp = t - o[dt];
        oc[dt] += (o[dt] - (t - bp)) + (od[dt] - bp);
        o[dt] = t;
      }
    }
    if (kt + 1 < ntile) {
      stage((kt + 1) & 1);
      if (kt + 2 < ntile) fetch(key0 + 2 * kEaKeys);
    }
    __syncthreads();
  }
  if (q < pad_b) {
    store_zero();
  } else if (q < P) {
    const int row = b * P + q;
    const float inv = (1.0f / (l + lc)) * pvinv;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o[0][i] += oc[0][i];
      o[1][i] += oc[1][i];
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int d = dt * 32 + 8 * gg + 4 * lh;
        attn_store4<NS>(tiled, out32, D, row, head * 64 + d, kbp, o[dt][4 * gg] * inv, o[dt][4 * gg + 1] * inv,
                        o[dt][4 * gg + 2] * inv, o[dt][4 * gg + 3] * inv);
      }
  }
}

hipError_t launch_prefill_self_attention(const float* qkv, float* cache_k, float* cache_v, int B, int P, int H, int ctx,
                                         const int* pad, _Float16* tiled, int ns, hipStream_t st, float* out32) {
  if (B < 1 || P < 1 || H < 1 || !qkv || !pad || (cache_k && (P > ctx || !cache_v))) return hipErrorInvalidValue;
  const long D = 64L * H;
  const dim3 grid((P + 32 * kPfWaves - 1) / (32 * kPfWaves), H, B), block(64 * kPfWaves);
#define WA_PFS(NS_)                                                                                                \
  hipLaunchKernelGGL((prefill_attention_kernel<NS_, true>), grid, block, 0, st, qkv, 3 * D, P * 3 * D, qkv + D,    \
                     qkv + 2 * D, 3 * D, 64L, P * 3 * D, P, P, pad, H, cache_k, cache_v, ctx, tiled, out32)
  if (ns == 2) { WA_PFS(2); } else { WA_PFS(1); }
#undef WA_PFS
  return hipGetLastError();
}

hipError_t launch_prefill_cross_attention(const float* q, const float* k, const float* v, int B, int P, int T, int H,
                                          _Float16* tiled, int ns, hipStream_t st, float* out32) {
  if (B < 1 || P < 1 || T < 1 || H < 1 || !q || !k || !v) return hipErrorInvalidValue;
  const long D = 64L * H;
  const dim3 grid((P + 32 * kPfWaves - 1) / (32 * kPfWaves), H, B), block(64 * kPfWaves);
#define WA_PFX(NS_)                                                                                               \
  hipLaunchKernelGGL((prefill_attention_kernel<NS_, false>), grid, block, 0, st, q, D, P * D, k, v, 64L, 64L * T, \
                     64L * T * H, P, T, nullptr, H, nullptr, nullptr, 0, tiled, out32)
  if (ns == 2) { WA_PFX(2); } else { WA_PFX(1); }
#undef WA_PFX
  return hipGetLastError();
}

// ---------------------------------------------- decode-step attention --
// Shared by self- and cross-attention of the decoder (Tq <= 4 queries per
// clip): 16 lanes share one key (4 dims each), 4 keys per load instruction,
// U instructions in flight per wave, online softmax per 16-lane group, then a
// fixed-order merge over the groups of a wave and over the 4 waves.

// Online-softmax scan of keys [k0, k1).  rows(j, kp, vp) yields this lane's
// 4-float K / V pointers of key j; vis(t, j) says whether query t sees key j.
// attn_fetch issues one pass's loads (4 U keys per wave), attn_update folds
// them in; attn_scan alternates the two.  A caller may issue the first pass's
// loads itself before its queries exist.
template <int TQ>
__device__ __forceinline__ void attn_init(float (&m)[TQ], float (&l)[TQ], floatx4 (&o)[TQ]) {
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.0f;
    o[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int U, class Rows>
__device__ __forceinline__ void attn_fetch(int j0, int k1, int grp, Rows rows, floatx4 (&kk)[U], floatx4 (&vv)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = max(0, min(j0 + 4 * u + grp, k1 - 1));  // clamped: loads never branch
    const float *kp, *vp;
    rows(j, kp, vp);
    kk[u] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(kp));
    vv[u] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(vp));
  }
}

template <int TQ, int U, class Vis>
__device__ __forceinline__ void attn_update(const floatx4 (&qv)[TQ], int Tq, int j0, int k1, int grp, Vis vis,
                                            const floatx4 (&kk)[U], const floatx4 (&vv)[U], float (&m)[TQ],
                                            float (&l)[TQ], floatx4 (&o)[TQ]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = j0 + 4 * u + grp;
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
      if (t < Tq) {
        const float dot =
            wq4::sum16(qv[t][0] * kk[u][0] + qv[t][1] * kk[u][1] + qv[t][2] * kk[u][2] + qv[t][3] * kk[u][3]);
        if (j < k1 && vis(t, j)) {
          const float mn = fmaxf(m[t], dot);
          const float alpha = __builtin_amdgcn_exp2f(m[t] - mn);  // base-2 units
          const float p = __builtin_amdgcn_exp2f(dot - mn);
          l[t] = l[t] * alpha + p;
          o[t] = o[t] * alpha + vv[u] * p;
          m[t] = mn;
        }
      }
    }
  }
}

template <int TQ, int U, class Rows, class Vis>
__device__ __forceinline__ void attn_scan(const floatx4 (&qv)[TQ], int Tq, int k0, int k1, int grp, Rows rows,
                                          Vis vis, float (&m)[TQ], float (&l)[TQ], floatx4 (&o)[TQ]) {
  attn_init<TQ>(m, l, o);
  for (int j0 = k0; j0 < k1; j0 += 4 * U) {
    floatx4 kk[U], vv[U];
    attn_fetch<U>(j0, k1, grp, rows, kk, vv);
    attn_update<TQ, U>(qv, Tq, j0, k1, grp, vis, kk, vv, m, l, o);
  }
}

// Merge the 4 groups of each wave, then the NWV waves, in a fixed order.  Wave
// t (< Tq) returns query t's (mn, ls, os = unnormalised o[lane]).
template <int TQ, int NWV>
__device__ __forceinline__ void attn_merge(int Tq, int wave, int lane, float (&m)[TQ], float (&l)[TQ],
                                           floatx4 (&o)[TQ], float (&wm)[NWV][TQ], float (&wl)[NWV][TQ],
                                           float (&wo)[NWV][TQ][64], float& mn, float& ls, float& os) {
  const int sub = lane & 15, grp = lane >> 4;
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    if (t >= Tq) break;
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
      const float m2 = __shfl_xor(m[t], off, 64), l2 = __shfl_xor(l[t], off, 64);
      floatx4 o2;
#pragma unroll
      for (int e = 0; e < 4; ++e) o2[e] = __shfl_xor(o[t][e], off, 64);
      const float mx = fmaxf(m[t], m2);
      const float a1 = m[t] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m[t] - mx);
      const float a2 = m2 == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m2 - mx);
      l[t] = l[t] * a1 + l2 * a2;
      o[t] = o[t] * a1 + o2 * a2;
      m[t] = mx;
    }
    if (grp == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) wo[wave][t][sub * 4 + e] = o[t][e];
    }
    if (lane == 0) {
      wm[wave][t] = m[t];
      wl[wave][t] = l[t];
    }
  }
  __syncthreads();
  mn = -INFINITY;
  ls = 0.0f;
  os = 0.0f;
  if (wave < Tq) {
    const int t = wave;
#pragma unroll
    for (int w = 0; w < NWV; ++w) mn = fmaxf(mn, wm[w][t]);
#pragma unroll
    for (int w = 0; w < NWV; ++w) {
      const float a = wm[w][t] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(wm[w][t] - mn);
      ls += wl[w][t] * a;
      os += wo[w][t][lane] * a;
    }
  }
}

// ------------------------------------------ decoder self-attention --
// One workgroup per (head, clip); the 4 waves split the keys 0 .. kv_len +
// Tq - 1 (causal inside the new tokens).  Self-K/V caches are head-major
// [clip][head][ctx][64] (contiguous per (clip, head)); the Tq new keys are
// appended there for later steps and read here straight from the qkv rows.
constexpr int kMaxCtx = 448;

template <int NS, int TQ>
__global__ __launch_bounds__(256) void dec_self_attn_kernel(const float* __restrict__ qkv, float* __restrict__ ck,
                                                            float* __restrict__ cv, int Tq_, int H, int ctx,
                                                            const DecodeState* state, int kv_len_host,
                                                            const int* __restrict__ pad,
                                                            _Float16* __restrict__ tiled, float* __restrict__ out32) {
  const int Tq = TQ == 1 ? 1 : Tq_;
  __shared__ float wm[4][TQ], wl[4][TQ];
  __shared__ float wo[4][TQ][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x, b = blockIdx.y;
  // a right-aligned prompt (wa_prefill): the clip's entries start at slot
  // pad_b, and the waves split the keys counted from there -- the order of
  // operations of an unpadded clip with kv_len - pad_b entries
  const int pad_b = pad ? pad[b] : 0;
  const int D = H * 64;
  const int sub = lane & 15, grp = lane >> 4;
  const int kv_len = state ? state->kv_len : kv_len_host;
  const size_t hb = ((size_t)b * H + head) * ctx * 64;
  floatx4 qv[TQ];
  const float* kb = ck + hb + sub * 4;
  const float* vb = cv + hb + sub * 4;
  const float* newb = qkv + (size_t)b * Tq * 3 * D + D + head * 64 + sub * 4;
  // append the new keys / values (decoder.rs:77-112 via Tensor::cat)
  if (tid < Tq * 16) {
    const int t = tid >> 4, s4 = (tid & 15) * 4;
    const float* src = qkv + (size_t)(b * Tq + t) * 3 * D + head * 64 + s4;
    *reinterpret_cast<floatx4*>(ck + hb + (size_t)(kv_len + t) * 64 + s4) = *reinterpret_cast<const floatx4*>(src + D);
    *reinterpret_cast<floatx4*>(cv + hb + (size_t)(kv_len + t) * 64 + s4) =
        *reinterpret_cast<const floatx4*>(src + 2 * D);
  }
#pragma unroll
  for (int t = 0; t < TQ; ++t)
    qv[t] = t < Tq ? *reinterpret_cast<const floatx4*>(qkv + (size_t)(b * Tq + t) * 3 * D + head * 64 + sub * 4) *
                         kEaQScale
                   : floatx4{0.f, 0.f, 0.f, 0.f};
  const int nk = kv_len + Tq - pad_b;
  const int per_wave = (nk + 3) / 4;
  const int k0 = pad_b + min(nk, wave * per_wave), k1 = min(pad_b + nk, k0 + per_wave);
  float m[TQ], l[TQ];
  floatx4 o[TQ];
  attn_scan<TQ, 8>(
      qv, Tq, k0, k1, grp,
      [&](int j, const float*& kp, const float*& vp) {
        if (j < kv_len) {
          kp = kb + (size_t)j * 64;
          vp = vb + (size_t)j * 64;
        } else {  // this step's own keys: not yet visible through the cache
          kp = newb + (size_t)(j - kv_len) * 3 * D;
          vp = kp + D;
        }
      },
      [&](int t, int j) { return j <= kv_len + t; }, m, l, o);
  float mn, ls, os;
  attn_merge<TQ, 4>(Tq, wave, lane, m, l, o, wm, wl, wo, mn, ls, os);
  if (wave < Tq) {
    const int t = wave;
    const float val = os / ls;
    const float v1 = __shfl_down(val, 1, 64), v2 = __shfl_down(val, 2, 64), v3 = __shfl_down(val, 3, 64);
    if ((lane & 3) == 0) attn_store4<NS>(tiled, out32, D, b * Tq + t, head * 64 + lane, kbp_of(D), val, v1, v2, v3);
  }
}

hipError_t launch_decoder_self_attention(const float* qkv, float* cache_k, float* cache_v, int B, int Tq, int H,
                                         int ctx, const DecodeState* state, int kv_len_host, _Float16* tiled,
                                         int ns, hipStream_t st, float* out32, const int* pad) {
  if (Tq > 4 || ctx > kMaxCtx) return hipErrorInvalidValue;
  const dim3 grid(H, B), block(256);
#define WA_SELF(NS_, TQ_)                                                                                     \
  hipLaunchKernelGGL((dec_self_attn_kernel<NS_, TQ_>), grid, block, 0, st, qkv, cache_k, cache_v, Tq, H, ctx, \
                     state, kv_len_host, pad, tiled, out32)
  if (ns == 2) {
    if (Tq == 1) { WA_SELF(2, 1); } else { WA_SELF(2, 4); }
  } else {
    if (Tq == 1) { WA_SELF(1, 1); } else { WA_SELF(1, 4); }
  }
#undef WA_SELF
  return hipGetLastError();
}

// The same step (Tq = 1) over a reindexed cache (beam search, wa_beam.hpp):
// key j < kv_len of row b lives in cache row anc[b][j].  The row's table is
// staged in LDS once, so a key's address waits on an LDS read, not on a
// dependent global load.  Everything else -- the 4-wave key split, the 8-deep
// scan, the merge, the epilogue -- is dec_self_attn_kernel<NS, 1>'s, so an
// identity table gives its bits.  The caches never move: a row appends at its
// own (b, kv_len), slots below kv_len are only read.
template <int NS>
__global__ __launch_bounds__(256) void dec_self_attn_beam_kernel(const float* __restrict__ qkv, float* __restrict__ ck,
                                                                 float* __restrict__ cv, int H, int ctx,
                                                                 const DecodeState* state, int kv_len_host,
                                                                 const int* __restrict__ anc,
                                                                 const int* __restrict__ pad,
                                                                 _Float16* __restrict__ tiled,
                                                                 float* __restrict__ out32) {
  __shared__ float wm[4][1], wl[4][1];
  __shared__ float wo[4][1][64];
  __shared__ int anc_s[kMaxCtx];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x, b = blockIdx.y, rows = gridDim.y;
  const int D = H * 64;
  const int sub = lane & 15, grp = lane >> 4;
  const int kv_len = state ? state->kv_len : kv_len_host;
  // a pair of tables under a device state: beam_select writes the one the next step reads
  const int* arow = anc + (state ? (size_t)((state->step + 1) & 1) * rows * ctx : 0) + (size_t)b * ctx;
  for (int j = tid; j < kv_len; j += 256) anc_s[j] = max(0, min(arow[j], rows - 1));  // loads stay inside the caches
  const size_t hb = ((size_t)b * H + head) * ctx * 64;
  floatx4 qv[1];
  const float* kb = ck + (size_t)head * ctx * 64 + sub * 4;
  const float* vb = cv + (size_t)head * ctx * 64 + sub * 4;
  const size_t row_stride = (size_t)H * ctx * 64;
  const float* newb = qkv + (size_t)b * 3 * D + D + head * 64 + sub * 4;
  if (tid < 16) {
    const int s4 = tid * 4;
    const float* src = qkv + (size_t)b * 3 * D + head * 64 + s4;
    *reinterpret_cast<floatx4*>(ck + hb + (size_t)kv_len * 64 + s4) = *reinterpret_cast<const floatx4*>(src + D);
    *reinterpret_cast<floatx4*>(cv + hb + (size_t)kv_len * 64 + s4) = *reinterpret_cast<const floatx4*>(src + 2 * D);
  }
  qv[0] = *reinterpret_cast<const floatx4*>(qkv + (size_t)b * 3 * D + head * 64 + sub * 4) * kEaQScale;
  __syncthreads();  // the table is staged
  // a right-aligned prompt: as dec_self_attn_kernel, the row's entries start at
  // slot pad_b and the waves split the keys counted from there
  const int pad_b = pad ? pad[b] : 0;
  const int nk = kv_len + 1 - pad_b;
  const int per_wave = (nk + 3) / 4;
  const int k0 = pad_b + min(nk, wave * per_wave), k1 = min(pad_b + nk, k0 + per_wave);
  float m[1], l[1];
  floatx4 o[1];
  attn_scan<1, 8>(
      qv, 1, k0, k1, grp,
      [&](int j, const float*& kp, const float*& vp) {
        if (j < kv_len) {
          const size_t ofs = (size_t)anc_s[j] * row_stride + (size_t)j * 64;
          kp = kb + ofs;
          vp = vb + ofs;
        } else {  // this step's own key: not yet visible through the cache
          kp = newb;
          vp = kp + D;
        }
      },
      [&](int, int j) { return j <= kv_len; }, m, l, o);
  float mn, ls, os;
  attn_merge<1, 4>(1, wave, lane, m, l, o, wm, wl, wo, mn, ls, os);
  if (wave < 1) {
    const float val = os / ls;
    const float v1 = __shfl_down(val, 1, 64), v2 = __shfl_down(val, 2, 64), v3 = __shfl_down(val, 3, 64);
    if ((lane & 3) == 0) attn_store4<NS>(tiled, out32, D, b, head * 64 + lane, kbp_of(D), val, v1, v2, v3);
  }
}

hipError_t launch_decoder_self_attention_beam(const float* qkv, float* cache_k, float* cache_v, int rows, int H,
                                              int ctx, const DecodeState* state, int kv_len_host, const int* anc,
                                              _Float16* tiled, int ns, hipStream_t st, float* out32, const int* pad) {
  if (rows < 1 || H < 1 || ctx < 1 || ctx > kMaxCtx || !anc || (!state && (kv_len_host < 0 || kv_len_host >= ctx)))
    return hipErrorInvalidValue;
  const dim3 grid(H, rows), block(256);
  if (ns == 2)
    hipLaunchKernelGGL(dec_self_attn_beam_kernel<2>, grid, block, 0, st, qkv, cache_k, cache_v, H, ctx, state,
                       kv_len_host, anc, pad, tiled, out32);
  else
    hipLaunchKernelGGL(dec_self_attn_beam_kernel<1>, grid, block, 0, st, qkv, cache_k, cache_v, H, ctx, state,
                       kv_len_host, anc, pad, tiled, out32);
  return hipGetLastError();
}

// ------------------------- cross-attention over cached K / V (few clips) --
// The reference's own formulation (attention.rs:177-206 forward_init_cache:
// K = enc Wk^T, V = enc Wv^T + bv cached per layer; :208-236 / 243-298
// forward_with_cache: softmax(q K^T / 8) V), for decode groups of a few
// clips: there the step is a latency chain, and one GEMV launch over the
// cached K / V (f32, head-major [clip][head][T][64], written by the
// head-major Q4 GEMM after the encoder) replaces the four launches of the
// cache-free form (wa_xattn.hip).  Products are f32 x f32 (exact), sums and
// softmax f32, as the reference's.
//
// Grid (H * S, B): the T keys of each (head, clip) are split over S
// workgroups (S from T only: a clip's bits do not depend on its batch).
// Each publishes (o[64], m, l) per query write-through (sc1 stores); the
// last arriver of the (clip, head), told by its counter ticket, merges the S
// partials in split order (sc1 loads; MI355X_MICROARCH.md hand-off table,
// row 1) and writes the A-tiled operand of the output projection.
constexpr int kXkvMaxSplit = 32;
constexpr int kXkvPart = 68;  // floats per (query) partial: o[64], m, l, pad

// 188 keys per split (8 splits at T = 1500, <= 47 keys per wave: one
// 12-deep scan pass); measured at one clip (Large-V3, in the decode step):
// 9.2 us per launch vs 9.9 at 96 keys, 11.1 at 375, 13.4 at 48 (r03).  A
// function of T only: a clip's bits do not depend on its batch.
constexpr int kXkvKeys = 188;
int cross_attention_kv_splits(int T) {
  const int s = (T + kXkvKeys - 1) / kXkvKeys;
  return s < 1 ? 1 : (s > kXkvMaxSplit ? kXkvMaxSplit : s);
}

template <int NS, int TQ>
__global__ __launch_bounds__(256) void cross_attn_kv_kernel(const float* __restrict__ q, const float* __restrict__ kc,
                                                            const float* __restrict__ vc, int Tq_, int T, int H,
                                                            int S, float* __restrict__ part,
                                                            int* __restrict__ counters,
                                                            _Float16* __restrict__ tiled, float* __restrict__ out32) {
  constexpr int U = TQ == 1 ? 12 : 8;  // <= 48 keys per wave in flight at once (decode step)
  const int Tq = TQ == 1 ? 1 : Tq_;
  __shared__ float wm[4][TQ], wl[4][TQ];
  __shared__ float wo[4][TQ][64];
  __shared__ int last_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x / S, split = blockIdx.x - head * S, b = blockIdx.y;
  const int D = H * 64;
  const int sub = lane & 15, grp = lane >> 4;
  const int per_split = (T + S - 1) / S;
  const int s0 = min(T, split * per_split), s1 = min(T, s0 + per_split);
  const int per_wave = (s1 - s0 + 3) / 4;
  const int k0 = min(s1, s0 + wave * per_wave), k1 = min(s1, k0 + per_wave);
  const size_t hofs = ((size_t)b * H + head) * T * 64 + sub * 4;
  const float* kb = kc + hofs;
  const float* vb = vc + hofs;
  auto rows = [&](int j, const float*& kp, const float*& vp) {
    kp = kb + (size_t)j * 64;
    vp = vb + (size_t)j * 64;
  };
  float m[TQ], l[TQ];
  floatx4 o[TQ];
  floatx4 qv[TQ];
  attn_init<TQ>(m, l, o);
#pragma unroll
  for (int t = 0; t < TQ; ++t)
    qv[t] = t < Tq ? *reinterpret_cast<const floatx4*>(q + (size_t)(b * Tq + t) * D + head * 64 + sub * 4) *
                         kEaQScale
                   : floatx4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = k0; j0 < k1; j0 += 4 * U) {
    floatx4 kk[U], vv[U];
    attn_fetch<U>(j0, k1, grp, rows, kk, vv);
    attn_update<TQ, U>(qv, Tq, j0, k1, grp, [](int, int) { return true; }, kk, vv, m, l, o);
  }
  float mn, ls, os;
  attn_merge<TQ, 4>(Tq, wave, lane, m, l, o, wm, wl, wo, mn, ls, os);
  if (S > 1) {
    typedef __attribute__((address_space(1))) float gfloat;
    typedef __attribute__((address_space(1))) int gint;
    const size_t bh = (size_t)b * H + head;
    if (wave < Tq) {  // this split's partial, write-through
      gfloat* pp = (gfloat*)(part + ((bh * S + split) * 4 + wave) * kXkvPart);
      __hip_atomic_store(pp + lane, os, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) __hip_atomic_store(pp + 64, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 1) __hip_atomic_store(pp + 65, ls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains before the ticket
    __syncthreads();
    if (tid == 0) {
      const int prev = __hip_atomic_fetch_add((gint*)(counters + bh), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_flag = prev == S - 1;
      if (prev == S - 1) __hip_atomic_store((gint*)(counters + bh), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last_flag || wave >= Tq) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler-only: the loads stay below the ticket
    // merge the S partials in split order (sc1 loads of sc1-stored bytes)
    float po[kXkvMaxSplit], pm[kXkvMaxSplit], pl[kXkvMaxSplit];
#pragma unroll
    for (int sp = 0; sp < kXkvMaxSplit; ++sp) {
      if (sp < S) {
        gfloat* pp = (gfloat*)(part + ((bh * S + sp) * 4 + wave) * kXkvPart);
        po[sp] = __hip_atomic_load(pp + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pm[sp] = __hip_atomic_load(pp + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pl[sp] = __hip_atomic_load(pp + 65, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    mn = -INFINITY;
#pragma unroll
    for (int sp = 0; sp < kXkvMaxSplit; ++sp)
      if (sp < S) mn = fmaxf(mn, pm[sp]);
    ls = 0.0f;
    os = 0.0f;
#pragma unroll
    for (int sp = 0; sp < kXkvMaxSplit; ++sp) {
      if (sp < S) {
        const float a = pm[sp] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(pm[sp] - mn);
        ls += pl[sp] * a;
        os += po[sp] * a;
      }
    }
  }
  if (wave < Tq) {
    const int t = wave;
    const float val = os / ls;
    const float v1 = __shfl_down(val, 1, 64), v2 = __shfl_down(val, 2, 64), v3 = __shfl_down(val, 3, 64);
    if ((lane & 3) == 0) attn_store4<NS>(tiled, out32, D, b * Tq + t, head * 64 + lane, kbp_of(D), val, v1, v2, v3);
  }
}

size_t cross_attention_kv_part_floats(int B, int H, int T) {
  return (size_t)B * H * cross_attention_kv_splits(T) * 4 * kXkvPart;
}

hipError_t launch_cross_attention_kv(const float* q, const float* k, const float* v, int B, int Tq, int T, int H,
                                     float* part, int* counters, _Float16* tiled, int ns, hipStream_t st,
                                     float* out32) {
  if (Tq < 1 || Tq > 4 || B < 1 || T < 1 || H < 1 || !q) return hipErrorInvalidValue;
  const int S = cross_attention_kv_splits(T);
  const dim3 grid(H * S, B), block(256);
#define WA_XKV(NS_, TQ_)                                                                                           \
  hipLaunchKernelGGL((cross_attn_kv_kernel<NS_, TQ_>), grid, block, 0, st, q, k, v, Tq, T, H, S, part, counters, \
                     tiled, out32)
  if (ns == 2) {
    if (Tq == 1) { WA_XKV(2, 1); } else { WA_XKV(2, 4); }
  } else {
    if (Tq == 1) { WA_XKV(1, 1); } else { WA_XKV(1, 4); }
  }
#undef WA_XKV
  return hipGetLastError();
}

// ------------------------------------------------------ conv + GELU --
// out[b, t, n] = gelu(bias[n] + sum_{kk, c} in(b, c, t*S + kk - 1) W[n, c, kk])
// (+ pos[t, n]).  GEMM view: rows (b, t), cols n, K = 3C (k = kk*C + c, the
// reference's im2col order, layers.rs:92-121).
constexpr int kCvLd = 40;
template <int NS>
__global__ __launch_bounds__(256) void conv_gelu_f16_kernel(const float* __restrict__ in, long in_bs, long in_cs,
                                                            long in_ts, int B, int C, int T_in, int S,
                                                            const float* __restrict__ wt,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ pos, int N,
                                                            float* __restrict__ out, int T_out) {
  __shared__ __attribute__((aligned(16))) _Float16 as[NS][128 * kCvLd];
  __shared__ __attribute__((aligned(16))) _Float16 bs[NS][128 * kCvLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, lh = lane >> 5;
  const int M = B * T_out, K = 3 * C;
  const int m0 = blockIdx.x * 128, n0 = blockIdx.y * 128;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  floatx16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][c][i] = 0.0f;
  auto put = [&](_Float16 (&dst)[NS][128 * kCvLd], int row, int kl, floatx4 v, float scale) {
    ea_half4 hi, lo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      _Float16 a, b;
      split_f16(v[j] * scale, a, b);
      hi[j] = a;
      lo[j] = b;
    }
    *reinterpret_cast<ea_half4*>(&dst[0][row * kCvLd + kl]) = hi;
    if constexpr (NS == 2) *reinterpret_cast<ea_half4*>(&dst[NS - 1][row * kCvLd + kl]) = lo;
  };
  for (int kc = 0; kc < K; kc += 32) {
    // stage A (im2col gather) and B: 128 rows x 32 k each, (row, 4 k) per item
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = it * 256 + tid;
      const int ml = e >> 3, kl = (e & 7) * 4;
      const int m = m0 + ml, k = kc + kl;
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < M && k < K) {
        const int bb = m / T_out, t = m - bb * T_out;
        if (in_cs == 1) {  // 4 consecutive channels of one tap (C % 4 == 0)
          const int kk = k / C, c = k - kk * C;
          const int ti = t * S + kk - 1;
          if (ti >= 0 && ti < T_in) v = *reinterpret_cast<const floatx4*>(in + bb * in_bs + c + (long)ti * in_ts);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int kj = k + j, kk = kj / C, c = kj - kk * C;
            const int ti = t * S + kk - 1;
            if (kj < K && ti >= 0 && ti < T_in) v[j] = in[bb * in_bs + c * in_cs + (long)ti * in_ts];
          }
        }
      }
      put(as, ml, kl, v, kCvAScale);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int e = it * 256 + tid;
      const int nl = e >> 3, kl = (e & 7) * 4;
      const int n = n0 + nl, k = kc + kl;
      const floatx4 v = (n < N && k + 3 < K) ? *reinterpret_cast<const floatx4*>(wt + (size_t)n * K + k)
                                             : floatx4{0.f, 0.f, 0.f, 0.f};
      put(bs, nl, kl, v, kCvBScale);
    }
    __syncthreads();
#pragma unroll
    for (int k16 = 0; k16 < 2; ++k16) {
      half8 a[2][NS], b[2][NS];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int p = 0; p < NS; ++p) {
          a[i][p] = *reinterpret_cast<const half8*>(&as[p][(wm + 32 * i + l32) * kCvLd + 16 * k16 + 8 * lh]);
          b[i][p] = *reinterpret_cast<const half8*>(&bs[p][(wn + 32 * i + l32) * kCvLd + 16 * k16 + 8 * lh]);
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = ea_mfma(a[i][0], b[j][0], acc[i][j]);
          if constexpr (NS == 2) {
            acc[i][j] = ea_mfma(a[i][1], b[j][0], acc[i][j]);
            acc[i][j] = ea_mfma(a[i][0], b[j][1], acc[i][j]);
          }
        }
    }
    __syncthreads();
  }
  // acc[i][j]: A = rows (m), B = cols (n): lane holds column n = l32, rows (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm + 32 * a + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int n = n0 + wn + 32 * c + l32;
        if (m < M && n < N) {
          float v = wq4::gelu_tanh(acc[a][c][i] * kCvInv + bias[n]);
          if (pos) v = v + pos[(size_t)(m % T_out) * N + n];
          out[(size_t)m * N + n] = v;
        }
      }
}

hipError_t launch_conv_gelu(const float* in, long in_bs, long in_cs, long in_ts, int B, int C, int T_in,
                            int stride, const float* w_t, const float* bias, const float* pos, int N, float* out,
                            hipStream_t st) {
  if (C % 4 != 0) return hipErrorInvalidValue;  // float4 channel staging (n_mels 80 / 128, D)
  const int T_out = (T_in + 2 - 3) / stride + 1;
  const dim3 grid((B * T_out + 127) / 128, (N + 127) / 128), block(256);
  hipLaunchKernelGGL(conv_gelu_f16_kernel<2>, grid, block, 0, st, in, in_bs, in_cs, in_ts, B, C, T_in, stride, w_t,
                     bias, pos, N, out, T_out);
  return hipGetLastError();
}

// ----------------------------------------------------------- embedding --
__global__ void embed_kernel(const int* __restrict__ tokens, const float* __restrict__ te,
                             const float* __restrict__ pe, int Tq, int D, const DecodeState* state, int pos0,
                             const int* __restrict__ pad, float* __restrict__ x) {
  const int row = blockIdx.x;  // b * Tq + t
  const int t = row % Tq;
  // a right-aligned prompt: the clip's positions count from its slot pad[b]
  // (a pad row of the prefill: position 0, never read by a real row)
  const int p = max(0, (state ? state->position : pos0) + t - (pad ? pad[row / Tq] : 0));
  const int tok = tokens[row];
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    x[(size_t)row * D + d] = te[(size_t)tok * D + d] + pe[(size_t)p * D + d];
}

hipError_t launch_embed(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                        const DecodeState* state, int pos0_host, float* x, hipStream_t st, const int* pad) {
  hipLaunchKernelGGL(embed_kernel, dim3(B * Tq), dim3(256), 0, st, tokens, tok_emb, pos_emb, Tq, D, state,
                     pos0_host, pad, x);
  return hipGetLastError();
}

// Embedding + the LayerNorm-fold producer of the first decoder layer's
// attn_ln (wq4_gemm_tiled_lnfold): x rows as embed_kernel, plus the A-tiled
// operand of x * gamma and per (row, 16-column tile) the tile mean and sum
// of squared deviations.  One workgroup per row; thread t owns the float4 at
// columns 4 t + 1024 i, so a tile is 4 consecutive lanes.
template <int NS>
__global__ __launch_bounds__(256) void embed_fold_kernel(const int* __restrict__ tokens, const float* __restrict__ te,
                                                         const float* __restrict__ pe, int Tq, int D,
                                                         const DecodeState* state, int pos0,
                                                         const int* __restrict__ pad, float* __restrict__ x,
                                                         const float* __restrict__ gamma, _Float16* __restrict__ at,
                                                         float* __restrict__ stats) {
  const int row = blockIdx.x;  // b * Tq + t
  const int t = row % Tq;
  const int p = max(0, (state ? state->position : pos0) + t - (pad ? pad[row / Tq] : 0));  // as embed_kernel
  const int tok = tokens[row];
  const int kbp = kbp_of(D);
  for (int c = 4 * threadIdx.x; c < ((D + 1023) / 1024) * 1024; c += 1024) {
    const bool in = c < D;  // D % 32 == 0: a tile is wholly in or out
    floatx4 v = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
    if (in) {
      const floatx4 a = *reinterpret_cast<const floatx4*>(te + (size_t)tok * D + c);
      const floatx4 b = *reinterpret_cast<const floatx4*>(pe + (size_t)p * D + c);
      g = *reinterpret_cast<const floatx4*>(gamma + c);
      v = a + b;
      *reinterpret_cast<floatx4*>(x + (size_t)row * D + c) = v;
      atile_store4<NS>(at, row, c, kbp, v[0] * g[0], v[1] * g[1], v[2] * g[2], v[3] * g[3]);
    }
    // statistics per 16-column tile (the decode-step GEMM's LayerNorm fold)
    float sum = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum * (1.0f / 16.0f);
    float m2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) m2 += (v[j] - mean) * (v[j] - mean);
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) m2 += __shfl_xor(m2, o, 64);
    if (in && (threadIdx.x & 3) == 0) {
      float* st = stats + ((size_t)row * (D / 16) + c / 16) * 2;
      st[0] = mean;
      st[1] = m2;
    }
  }
}

hipError_t launch_embed_fold(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                             const DecodeState* state, int pos0_host, float* x, const float* gamma, _Float16* at,
                             float* stats, int ns, hipStream_t st, const int* pad) {
  if (D % 32 != 0) return hipErrorInvalidValue;
  if (ns == 2)
    hipLaunchKernelGGL(embed_fold_kernel<2>, dim3(B * Tq), dim3(256), 0, st, tokens, tok_emb, pos_emb, Tq, D, state,
                       pos0_host, pad, x, gamma, at, stats);
  else
    hipLaunchKernelGGL(embed_fold_kernel<1>, dim3(B * Tq), dim3(256), 0, st, tokens, tok_emb, pos_emb, Tq, D, state,
                       pos0_host, pad, x, gamma, at, stats);
  return hipGetLastError();
}

}  // namespace wa
