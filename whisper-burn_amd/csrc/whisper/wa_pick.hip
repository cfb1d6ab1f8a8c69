// wa_pick.hip -- gfx950 kernels of the decoder's output end: the logits, the
// token pick in every decoding mode (greedy, scored, timestamps, sampled,
// sampled + timestamps) and the greedy loop's bookkeeping (wa_pick.hpp).
//
// Reference semantics (zerr0o/whisper-burn):
//   logits / argmax  src/model/decoder.rs:289-292, 342-347; whisper.rs:131-138
//   greedy loop      src/model/whisper.rs:97-125
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../wq4_device.hpp"
#include "wa_pick.hpp"
#include "wa_tsrule.hpp"

// WA_LOGITS_NT (default on): the decode step's 266-MB embedding-table stream
// (logits_argmax_f16_k32_kernel) with the nontemporal policy, so it does not
// push the encoder planes the next step's cross-attention re-reads out of the
// Infinity Cache: decode 928 -> 920 ms at 32 clips, RTF +0.7 % (two A/B runs
// bracketed by the base build, profiles/r06af_libs.txt, r06ag_libs.txt).
#ifndef WA_LOGITS_NT
#define WA_LOGITS_NT 1
#endif

namespace wa {

using wq4::floatx16;
using wq4::floatx4;
using wq4::half8;
using wq4::split_f16;

constexpr int kEOT = 50257;
// logits: hidden rows as GEMM activations (x 2^4), the f16-pair table x 2^8
// (|e| < 255), logits x 2^-12
constexpr float kEmbScale = 256.0f, kLgInv = 1.0f / (16.0f * 256.0f);

__device__ __forceinline__ floatx16 mfma_f32(float a, float b, const floatx16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// -------------------------------------------------------------- logits --
// logits[b, v] = sum_d h[b, d] E[v, d]; B <= 32 clips per call.  One wave =
// 32 vocabulary rows; h staged in LDS in 256-wide k chunks.
__global__ __launch_bounds__(256) void logits_kernel(const float* __restrict__ hid, int B, int D, long ldh,
                                                     const float* __restrict__ emb, int V,
                                                     float* __restrict__ logits) {
  __shared__ float hs[32][256 + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n = blockIdx.x * 128 + wave * 32 + r;
  const float* er = emb + (size_t)(n < V ? n : 0) * D;
  floatx16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  for (int kc = 0; kc < D; kc += 256) {
    const int kw = min(256, D - kc);
    __syncthreads();
    for (int e = tid; e < 32 * 256; e += 256) {
      const int row = e >> 8, k = e & 255;
      hs[row][k] = (row < B && k < kw) ? hid[(size_t)row * ldh + kc + k] : 0.0f;
    }
    __syncthreads();
    for (int k8 = 0; k8 < kw; k8 += 8) {
      const floatx4 e4 = n < V ? *reinterpret_cast<const floatx4*>(er + kc + k8 + 4 * h) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = mfma_f32(hs[r][k8 + 4 * h + s], e4[s], acc);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < B && n < V) logits[(size_t)row * V + n] = acc[i];
  }
}

hipError_t launch_logits(const float* h, int B, int D, long ldh, const float* emb, int V, float* logits,
                         hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int nb = min(32, B - b0);
    hipLaunchKernelGGL(logits_kernel, dim3((V + 127) / 128), dim3(256), 0, st, h + (size_t)b0 * ldh, nb, D, ldh,
                       emb, V, logits + (size_t)b0 * V);
  }
  return hipGetLastError();
}

// -------------------------------------------------------------- argmax --
// Rust `max_by(partial_cmp)` keeps the LAST of equal maxima (whisper.rs:131-138):
// (value, index) compared lexicographically, the one comparator of every pick.
// Returns whether (v, i) replaced (bv, bi).
__device__ __forceinline__ bool better(float& bv, int& bi, float v, int i) {
  const bool won = v > bv || (v == bv && i > bi);
  if (won) {
    bv = v;
    bi = i;
  }
  return won;
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int V, int lo, int hi,
                                                     int suppress_fixed, int min_tokens, const DecodeState* state,
                                                     int* __restrict__ out, int out_stride, int* __restrict__ range_flag,
                                                     const uint32_t* __restrict__ sup) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* lg = logits + (size_t)b * V;
  const int suppress = state ? (state->step + 1 < min_tokens) : suppress_fixed;
  float bv = -INFINITY;
  int bi = -1;
  bool bad = false;
  for (int i = lo + tid; i < hi; i += 256) {
    float v = lg[i];
    bad |= !__builtin_isfinite(v);
    if ((suppress && i == kEOT) || sup_masked(sup, i)) v = -INFINITY;
    better(bv, bi, v, i);
  }
  if (bad && range_flag) *range_flag = 1;  // plain vector store: every writer stores 1
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(bv, o, 64);
    const int i = __shfl_xor(bi, o, 64);
    better(bv, bi, v, i);
  }
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) better(bv, bi, sv[w], si[w]);
    out[(size_t)b * out_stride] = bi < 0 ? lo : bi;
  }
}

hipError_t launch_argmax(const float* logits, int B, int V, int lo, int hi, int suppress_eot,
                         int* out_tok, int out_stride, int* range_flag, hipStream_t st, const uint32_t* sup) {
  hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(256), 0, st, logits, V, lo, hi, suppress_eot, 0,
                     (const DecodeState*)nullptr, out_tok, out_stride, range_flag, sup);
  return hipGetLastError();
}

hipError_t launch_argmax_step(const float* logits, int B, int V, int min_tokens, const DecodeState* state,
                              int* out_tok, int* range_flag, hipStream_t st, const uint32_t* sup) {
  hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(256), 0, st, logits, V, 0, V, 0, min_tokens, state, out_tok, 1,
                     range_flag, sup);
  return hipGetLastError();
}

// ------------------------------------------------------ suppress masks --
int64_t sup_mask_words(int V) { return emb_tiled_rows(V) / 32; }

void sup_mask_build(const int32_t* ids, int n, int V, uint32_t* words) {
  std::fill(words, words + sup_mask_words(V), 0u);
  for (int i = 0; i < n; ++i)
    if (ids[i] >= 0 && ids[i] < V) words[ids[i] >> 5] |= 1u << (ids[i] & 31);
}

// ------------------------------------------------- timestamp rules --
// The rule record's history update (ts_rule_step) and the masks a-e read from
// a record (ts_masked): wa_tsrule.hpp, shared with the beam search's kernels.
TsRule ts_rule_first(int ts0, int V, int max_initial) {
  TsRule r{};
  r.text_ok = 0;
  r.ts_lo = ts0;
  r.ts_hi = max_initial < 0 ? V - 1 : (int)std::min<int64_t>(V - 1, (int64_t)ts0 + max_initial);
  r.first = 1;
  r.last = 0;
  r.penult = 1;
  r.t_last = -1;
  return r;
}

TsRule ts_rule_next(const TsRule& r, int tok, int ts0, int V) { return ts_rule_step(r, tok, ts0, V); }

// The mass rule and the pick from a row's two sides: (mt, it) the best text
// candidate with st = sum exp(z - mt) over the text side, (mx, ix, sx) the
// same over the timestamps; a side with nothing allowed is (-inf, -1, 0).
// lp = the pick's log-probability over the sides that survive.
__device__ __forceinline__ void ts_decide(float mt, int it, float st, float mx, int ix, float sx, int& tok, float& lp,
                                          int& mass) {
  const float lse_x = mx > -INFINITY ? mx + logf(sx) : -INFINITY;
  mass = lse_x > mt ? 1 : 0;  // rule f: raw logits, the softmax normaliser is common to both sides
  if (mass) {
    tok = ix;
    lp = -logf(sx);
  } else {
    float M = mt;
    tok = it;
    better(M, tok, mx, ix);
    const float a = mt > -INFINITY ? st * expf(mt - M) : 0.0f;
    const float b = mx > -INFINITY ? sx * expf(mx - M) : 0.0f;
    lp = -logf(a + b);
  }
  if (tok < 0) tok = 0;
}

// ------------------------------------------------ temperature sampling --
// Gumbel-max: argmax_v (z_v + T g_v), g i.i.d. standard Gumbel, is a draw
// from softmax(z / T) -- the pick stays an argmax, over perturbed keys.  The
// noise is a pure function of (clip seed, pick index, token id): splitmix64's
// finaliser over a per-pick key, 23 bits to a uniform strictly inside (0, 1)
// (exact in f32), g = -log(-log u) in [-2.82, 16.64].  The one definition,
// shared by the fused kernel, the row kernel and the host (sample_noise).
__host__ __device__ inline uint64_t smp_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
__host__ __device__ inline uint64_t smp_pick_key(uint64_t seed, int pick) {
  return smp_mix(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(pick + 1));
}
__host__ __device__ inline float smp_uniform(uint64_t k, int v) {
  const uint32_t h = (uint32_t)(smp_mix(k ^ (uint64_t)v) >> 41);  // 23 bits
  return ((float)h + 0.5f) * 0x1p-23f;                            // exact: 2 h + 1 < 2^24
}
__host__ __device__ inline float smp_gumbel(uint64_t k, int v) { return -logf(-logf(smp_uniform(k, v))); }
// The key of logit z: a clip with T = 0 evaluates no noise; -inf stays -inf (g is finite).
__device__ __forceinline__ float smp_key(float z, float T, uint64_t k, int v) {
  return T > 0.0f ? fmaf(T, smp_gumbel(k, v), z) : z;
}

void sample_noise(uint64_t seed, int pick, int id0, int n, float* u_out, float* g_out) {
  const uint64_t k = smp_pick_key(seed, pick);
  for (int i = 0; i < n; ++i) {
    if (u_out) u_out[i] = smp_uniform(k, id0 + i);
    if (g_out) g_out[i] = smp_gumbel(k, id0 + i);
  }
}

// ------------------------------------------------------------ the pick --
// Every decoding mode picks by one reduction over a row's logits z, split
// into one or two sides (two: ids below ts0 are text, the rest timestamps).
// Per side it keeps
//   m      the raw maximum (fmaxf, never touched by the noise)
//   i      the index of the best key, the LARGEST index among equal keys
//   s      SUMS: sum exp(z - m) -- a masked (-inf) logit adds 0, two equal
//          maxima add 1 each
//   k, z   KEYS: the best Gumbel-perturbed key (smp_key) and the raw logit at i
// Without KEYS the key is the logit: (m, i) is the candidate and nothing more
// is kept.  A side with nothing allowed is (-inf, -1, 0).  (value, index) is
// compared lexicographically, so the result equals the sequential Rust max_by
// scan whatever the reduction order.
//   greedy <1, 0, 0>   scored <1, 1, 0>   timestamps <2, 1, 0>
//   sampled <1, 1, 1>  sampled + timestamps <2, 1, 1>     (<SIDES, SUMS, KEYS>)
struct PickSide {
  float m = -INFINITY;
  int i = -1;
  float s = 0.0f;
  float k = -INFINITY, z = -INFINITY;
};

template <int KEYS>
__device__ __forceinline__ void pick_merge(PickSide& a, const PickSide& o) {
  if constexpr (KEYS) {
    a.m = fmaxf(a.m, o.m);
    if (better(a.k, a.i, o.k, o.i)) a.z = o.z;
  } else {
    better(a.m, a.i, o.m, o.i);
  }
}

// pick_merge with lane ^ o's candidate
template <int KEYS>
__device__ __forceinline__ void pick_merge_xor(PickSide& a, int o) {
  PickSide c;
  c.m = __shfl_xor(a.m, o, 64);
  c.i = __shfl_xor(a.i, o, 64);
  if constexpr (KEYS) {
    c.k = __shfl_xor(a.k, o, 64);
    c.z = __shfl_xor(a.z, o, 64);
  }
  pick_merge<KEYS>(a, c);
}

// A partial sum s relative to its own maximum m, rescaled to the row's M.
__device__ __forceinline__ float pick_rescaled(float s, float m, float M) { return s * expf(m - M); }

// The decision from a row's merged side(s) (x is t when SIDES = 1), shared by
// the fused reduction and the stored-row kernel: rule f and the log-probability
// lpg = -log sum exp(z - Ms) over the surviving side(s), Ms their raw maximum
// (ts_decide; one side: -log s); under KEYS the best key over the surviving
// side(s) -- the noise never reaches rule f -- whose token lies d = z_tok - Ms
// below that (d = 0: the greedy token, and the unsampled forms' bits).
template <int SIDES, int SUMS, int KEYS>
__device__ __forceinline__ void pick_decide(const PickSide& t, const PickSide& x, int& tok, float& lp, int& mass) {
  float lpg = 0.0f;
  mass = 0;
  if constexpr (SIDES == 2) {
    ts_decide(t.m, t.i, t.s, x.m, x.i, x.s, tok, lpg, mass);  // tok: the pick when the key is the logit
  } else {
    tok = t.i;
    if constexpr (SUMS) lpg = -logf(t.s);
  }
  lp = lpg;
  if constexpr (KEYS) {
    float Ms = t.m, zt = t.z;
    tok = t.i;
    if constexpr (SIDES == 2) {
      if (mass) {
        Ms = x.m;
        tok = x.i;
        zt = x.z;
      } else {
        float kk = t.k;
        Ms = fmaxf(t.m, x.m);
        if (better(kk, tok, x.k, x.i)) zt = x.z;
      }
    }
    const float d = zt - Ms;
    lp = d == 0.0f ? lpg : d + lpg;
  }
  if (tok < 0) tok = 0;
}

// What the fused kernel's pick reads and writes (wa_pick.hpp): PickArgs.
enum { kPkMax = 0, kPkIdx = 1, kPkSum = 2, kPkKey = 3, kPkZ = 4 };

// The pick of a workgroup's 32 x 128 logits block lg[clip][kLgPickLd]
// (already masked), then the last-arriving workgroup's pick over all
// workgroups' candidates: each workgroup leaves per row and side its
// PickSide in the scratch block [side][array][32][groups] (2 + SUMS + 2 KEYS
// arrays per side, kPk*; a workgroup stores the sides it holds ids of), with
// write-through stores ahead of an agent-scope ticket (cdna_hip_programming.md
// Guideline 16 R1); the last arriver merges the candidates, then, knowing each
// side's M, sums S = sum_w s_w exp(m_w - M), decides (pick_decide) and re-arms
// the counter.  out_lp = log softmax(z)[tok] over the finally masked row,
// untempered.  f32 throughout; the additions of a sum come in a fixed order:
// 16 per thread, the xor butterfly 1-2-4, the candidates j = part, part + 8,
// .., the butterfly again (73 at V = 51866, and one more to join two sides).
// The pick key k(seed, pick) is hashed once per thread; a row with T = 0
// evaluates no noise and repeats the unsampled forms' bits.
constexpr int kLgPickLd = 132;
template <int SIDES, int SUMS, int KEYS>
__device__ __forceinline__ void pick_from_lds(const float* lg, int B, int V, int pick, const PickArgs& a, int* ticket) {
  constexpr int A = 2 + SUMS + 2 * KEYS;  // arrays per side
  const int tid = threadIdx.x, nwg = gridDim.x;
  const int ts0 = SIDES == 2 ? a.ts0 : V;                          // one side: every id on side 0
  const int n0 = SIDES == 2 ? min(nwg, (ts0 + 127) / 128) : nwg;  // workgroups [0, n0) hold side-0 ids
  const int j1 = min(nwg, ts0 / 128);                              // workgroups [j1, nwg) hold side-1 ids
  const bool has0 = SIDES == 1 || (int)blockIdx.x < n0, has1 = SIDES == 2 && (int)blockIdx.x >= j1;
  __syncthreads();
  const int row = tid >> 3, part = tid & 7;
  float T = 0.0f;
  uint64_t nk = 0;
  if constexpr (KEYS) {
    T = row < B ? a.temp[row] : 0.0f;  // rows >= B: no noise
    nk = T > 0.0f ? smp_pick_key(a.seed[row], pick) : 0;
  }
  PickSide sd[SIDES];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int c = part * 16 + j;
    const int idx = blockIdx.x * 128 + c;
    PickSide one;
    one.m = lg[row * kLgPickLd + c];
    one.i = idx;
    if constexpr (KEYS) {
      one.k = smp_key(one.m, T, nk, idx);
      one.z = one.m;
    }
    if (idx < V) {
      if (SIDES == 1 || idx < ts0)
        pick_merge<KEYS>(sd[0], one);
      else
        pick_merge<KEYS>(sd[SIDES - 1], one);
    }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1)
#pragma unroll
    for (int s = 0; s < SIDES; ++s) pick_merge_xor<KEYS>(sd[s], o);
  if constexpr (SUMS) {
    // each side's sum relative to its own maximum (the same in the row's 8
    // threads); a side with every logit masked: 0
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int c = part * 16 + j;
      const int idx = blockIdx.x * 128 + c;
      const float v = lg[row * kLgPickLd + c];
      if (idx < V) {
        if (SIDES == 1 || idx < ts0) {
          if (sd[0].m > -INFINITY) sd[0].s += expf(v - sd[0].m);
        } else {
          if (sd[SIDES - 1].m > -INFINITY) sd[SIDES - 1].s += expf(v - sd[SIDES - 1].m);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1)
#pragma unroll
      for (int s = 0; s < SIDES; ++s) sd[s].s += __shfl_xor(sd[s].s, o, 64);
  }
  const uint32_t plane = 32u * nwg * 4u;  // bytes of one [32][groups] array
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.scratch, 0, SIDES * A * plane, 0x00020000);
  auto put = [&](int side, int arr, uint32_t off, uint32_t bits) {
    __builtin_amdgcn_raw_buffer_store_b32(bits, rs, (uint32_t)(side * A + arr) * plane + off, 0, 16);  // sc1
  };
  auto get = [&](int side, int arr, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)(side * A + arr) * plane + off, 0, 16);
  };
  auto f2u = [](float f) { return __builtin_bit_cast(uint32_t, f); };
  auto u2f = [](uint32_t u) { return __builtin_bit_cast(float, u); };
  auto put_side = [&](int side, uint32_t off, const PickSide& p) {
    put(side, kPkMax, off, f2u(p.m));
    put(side, kPkIdx, off, (uint32_t)p.i);
    if constexpr (SUMS) put(side, kPkSum, off, f2u(p.s));
    if constexpr (KEYS) {
      put(side, kPkKey, off, f2u(p.k));
      put(side, kPkZ, off, f2u(p.z));
    }
  };
  // workgroups [j0, jn) of one side: their candidates into p, or (sums) their
  // partial sums rescaled to p.m
  auto merge_side = [&](int side, int j0, int jn, PickSide& p) {
    for (int j = j0 + part; j < jn; j += 8) {
      const uint32_t off = (uint32_t)(row * nwg + j) * 4;
      PickSide c;
      c.m = u2f(get(side, kPkMax, off));
      c.i = (int)get(side, kPkIdx, off);
      if constexpr (KEYS) {
        c.k = u2f(get(side, kPkKey, off));
        c.z = u2f(get(side, kPkZ, off));
      }
      pick_merge<KEYS>(p, c);
    }
  };
  auto sum_side = [&](int side, int j0, int jn, PickSide& p) {
    if (p.m > -INFINITY)
      for (int j = j0 + part; j < jn; j += 8) {
        const uint32_t off = (uint32_t)(row * nwg + j) * 4;
        p.s += pick_rescaled(u2f(get(side, kPkSum, off)), u2f(get(side, kPkMax, off)), p.m);
      }
  };
  if (part == 0 && row < B) {
    const uint32_t off = (uint32_t)(row * nwg + blockIdx.x) * 4;  // < plane: row < 32, blockIdx.x < nwg
    if (has0) put_side(0, off, sd[0]);
    if constexpr (SIDES == 2)
      if (has1) put_side(1, off, sd[1]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    typedef __attribute__((address_space(1))) int gint;
    const int prev = __hip_atomic_fetch_add((gint*)a.counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *ticket = prev == nwg - 1;
  }
  __syncthreads();
  if (!*ticket) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // compiler-only: loads stay below the ticket
#pragma unroll
  for (int s = 0; s < SIDES; ++s) sd[s] = PickSide{};
  if (row < B) {
    merge_side(0, 0, n0, sd[0]);
    if constexpr (SIDES == 2) merge_side(1, j1, nwg, sd[1]);
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1)
#pragma unroll
    for (int s = 0; s < SIDES; ++s) pick_merge_xor<KEYS>(sd[s], o);
  if constexpr (SUMS) {
    // sd[].m = each side's M in the row's 8 threads: the candidates again, rescaled to it
    if (row < B) {
      sum_side(0, 0, n0, sd[0]);
      if constexpr (SIDES == 2) sum_side(1, j1, nwg, sd[1]);
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1)
#pragma unroll
      for (int s = 0; s < SIDES; ++s) sd[s].s += __shfl_xor(sd[s].s, o, 64);
  }
  if (part == 0 && row < B) {
    int tok, mass;
    float lp;
    pick_decide<SIDES, SUMS, KEYS>(sd[0], sd[SIDES - 1], tok, lp, mass);
    a.out_tok[row] = tok;
    if constexpr (SUMS) a.out_lp[row] = lp;
    if constexpr (SIDES == 2)
      if (a.out_mass) a.out_mass[row] = mass;
  }
  if (tid == 0) {
    typedef __attribute__((address_space(1))) int gint;
    __hip_atomic_store((gint*)a.counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm
  }
}

constexpr int kLg2Chunk = 128;
// 16-row groups of the fragment-tiled table (V padded to 128-row workgroups)
__host__ __device__ inline int64_t emb_groups16(int V) { return (int64_t)(V + 127) / 128 * 8; }

// Tied-embedding logits of the decode step on f16 MFMA, fused with the pick
// (pick_from_lds<SIDES, SUMS, KEYS>: the logits never reach HBM): the
// embedding as exact-to-2^-22 f16 pairs E = hi + lo in a fragment-tiled table (launch_emb_tiled: a lane's fragment is 8 dims of one
// of 16 rows, one load instruction reads 1 KiB contiguous), the hidden rows
// as the A-tiled f16-pair operand the final LayerNorm writes (wq4_layernorm,
// the same split as the GEMMs); three 16x16x32 f16 MFMAs per product
// (hi*hi + lo*hi + hi*lo), f32 accumulation.  Wave = 32 vocabulary rows as
// two 16-row m-tiles, the 32 clips as two n-tiles.  Per 128-dim chunk the
// hidden fragments (32 rows x 128 dims, 8 or 16 KiB) come into an LDS double
// buffer through registers one chunk ahead, beside the next chunk's table
// fragments in registers: one barrier per chunk, no conversion.  trace_out
// (diagnostics, null in the product graph): the logits of
// trace_ids[clip][step + 1][0..trace_k) are written to the same slots of
// trace_out, as the pick sees them (EOT already masked).
// SIDES = 2 (timestamp transcribes): the masks of the rows' rule records
// (ts_masked) while lg[] is written.  KEYS (sampled transcribes): the pick
// index of the noise is state->step + 1.  An instantiation reads the members
// of `pick` its mode needs and no others.
// SUP (a model with suppress lists): the wave's 32 vocabulary rows v0 .. v0 +
// 31 are word v0 / 32 of pick.sup -- one scalar word load per wave, issued
// ahead of the chunk loop, and a bit test per value where lg[] is written,
// ahead of the EOT / rule masks.  SUP = 0 is the kernel without any of it.
template <int NS, int SIDES, int SUMS, int KEYS, int SUP>
__global__ __launch_bounds__(256) void logits_argmax_f16_k32_kernel(
    const _Float16* __restrict__ htiled, int B, int D, const _Float16* __restrict__ emb2, int V, int min_tokens,
    const DecodeState* __restrict__ state, PickArgs pick, const int* __restrict__ trace_ids,
    float* __restrict__ trace_out, int trace_s1, int trace_k, int* __restrict__ range_flag) {
  constexpr bool TS = SIDES == 2;
  constexpr int KS = kLg2Chunk / 32;             // Q4-block-sized k-steps per chunk
  constexpr int HCH = KS * 2 * NS * 1024;        // bytes of hidden fragments per chunk
  static_assert(HCH % (256 * 16) == 0, "whole glds rounds");
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * HCH + 32 * kLgPickLd * 4 + 16];
  float* lg = reinterpret_cast<float*>(smem + 2 * HCH);
  int* ticket = reinterpret_cast<int*>(smem + 2 * HCH + 32 * kLgPickLd * 4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, lq = lane >> 4;
  const int v0 = blockIdx.x * 128 + wave * 32;
  // chunk-major table (launch_emb_tiled): this wave's two 16-row groups are
  // 2 KS NS KiB contiguous per chunk, and a chunk of the whole table is one
  // contiguous stretch (every wave streams the same region at once)
  const int nch = D / kLg2Chunk;
  const size_t chunk_halves = (size_t)emb_groups16(V) * KS * NS * 512;
  const _Float16* er = emb2 + (size_t)(v0 / 16) * KS * NS * 512 + lane * 8;
  floatx4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
  half8 ec[2][KS][NS], en[2][KS][NS];
  auto load_e = [&](half8 (&e)[2][KS][NS], int kc) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int p = 0; p < NS; ++p)  // D % kLg2Chunk == 0 (launcher): always in range
          e[mt][ks][p] = WA_LOGITS_NT ? __builtin_nontemporal_load(reinterpret_cast<const half8*>(
                                            er + (kc / kLg2Chunk) * chunk_halves + ((mt * KS + ks) * NS + p) * 512))
                                      : *reinterpret_cast<const half8*>(er + (kc / kLg2Chunk) * chunk_halves +
                                                                         ((mt * KS + ks) * NS + p) * 512);
  };
  // the hidden fragments of chunk c: A-tiled m-tile 0, blocks 4c .. 4c + 3
  // (kk, plane, lane: 1 KiB each, contiguous), staged through registers into
  // LDS buffer c & 1 lane-linear.  Not global_load_lds: while an LDS DMA is in
  // flight hipcc waits vmcnt(0) at the first use of any ordinary load result
  // (cdna_hip_programming.md "Pipelining across barriers"), which would drain
  // the next chunk's table loads at the first MFMA of every chunk.
  constexpr int HPT = HCH / (256 * 16);  // 16-B pieces per thread per chunk
  half8 hr[HPT];
  auto load_h = [&](int c) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(htiled) + (size_t)c * HCH;
#pragma unroll
    for (int i = 0; i < HPT; ++i) hr[i] = *reinterpret_cast<const half8*>(src + (i * 256 + tid) * 16);
  };
  auto store_h = [&](int c) {
#pragma unroll
    for (int i = 0; i < HPT; ++i) *reinterpret_cast<half8*>(smem + (c & 1) * HCH + (i * 256 + tid) * 16) = hr[i];
  };
  uint32_t supw = 0;  // SUP: the mask bits of ids v0 .. v0 + 31 (word < sup_mask_words(V): v0 < emb_tiled_rows(V))
  if constexpr (SUP) supw = pick.sup[__builtin_amdgcn_readfirstlane(v0 >> 5)];
  load_h(0);
  load_e(ec, 0);
  store_h(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    // hidden c + 1 first (its wait after the MFMAs then leaves the table loads
    // in flight), the next chunk's table second
    if (c + 1 < nch) load_h(c + 1);
    load_e(en, c + 1 < nch ? (c + 1) * kLg2Chunk : c * kLg2Chunk);  // the last chunk re-loads itself
    // keep the loads here: left to itself the scheduler sinks them below the
    // MFMAs (fewer live registers), and every chunk then waits a full latency
    __builtin_amdgcn_sched_barrier(0);
    const uint8_t* hb = smem + (c & 1) * HCH;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        // B: clip 16 nt + l16, dims 32 ks + 8 lq .. + 7 = fragment (ks, kk = lq >> 1),
        // lane' = clip + 32 (lq & 1)
        const int off = ((ks * 2 + (lq >> 1)) * NS) * 1024 + (16 * nt + l16 + 32 * (lq & 1)) * 16;
        const half8 bh = *reinterpret_cast<const half8*>(hb + off);
        half8 bl;
        if constexpr (NS == 2) bl = *reinterpret_cast<const half8*>(hb + off + 1024);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ec[mt][ks][0], bh, acc[mt][nt], 0, 0, 0);
          if constexpr (NS == 2) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ec[mt][ks][1], bh, acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ec[mt][ks][0], bl, acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
    // buffer (c + 1) & 1 was last read in chunk c - 1, before the previous barrier
    if (c + 1 < nch) store_h(c + 1);
    __syncthreads();  // no LDS DMA in flight: a bare s_barrier, the table loads survive it
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int p = 0; p < NS; ++p) ec[mt][ks][p] = en[mt][ks][p];
  }
  // acc[mt][nt]: lane holds clip 16 nt + l16, vocab v0 + 16 mt + 4 lq + j
  const int suppress = state->step + 1 < min_tokens;
  bool bad = false;
  int4 rule[2] = {};  // TS: the records of this lane's two clips (a padded clip reads the last one's)
  if constexpr (TS) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
      rule[nt] = *reinterpret_cast<const int4*>(pick.rules + min(16 * nt + l16, B - 1));
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int vl = 16 * mt + 4 * lq + j;
        const int n = v0 + vl;
        float v = acc[mt][nt][j] * kLgInv;
        bad |= n < V && 16 * nt + l16 < B && !__builtin_isfinite(v);
        if constexpr (SUP) {
          if ((supw >> vl) & 1u) v = -INFINITY;
        }
        if constexpr (TS) {
          if (n >= V || ts_masked(n, pick.ts0, rule[nt], suppress != 0)) v = -INFINITY;
        } else {
          if (n >= V || (suppress && n == kEOT)) v = -INFINITY;
        }
        lg[(16 * nt + l16) * kLgPickLd + wave * 32 + vl] = v;
      }
  // an MFMA operand out of the f16-pair range upstream turns every logit of
  // the clip into inf / NaN: flag it (plain vector store, every writer stores 1)
  if (bad && range_flag) *range_flag = 1;
  if (trace_out) {  // diagnostics only: uniform branch
    __syncthreads();
    const int slot = state->step + 1;
    if (slot < trace_s1)
      for (int e = tid; e < B * trace_k; e += 256) {
        const int b = e / trace_k;
        const size_t o = ((size_t)b * trace_s1 + slot) * trace_k + (e - b * trace_k);
        const int id = trace_ids[o] - (int)blockIdx.x * 128;
        if (id >= 0 && id < 128) trace_out[o] = lg[b * kLgPickLd + id];
      }
  }
  pick_from_lds<SIDES, SUMS, KEYS>(lg, B, V, state->step + 1, pick, ticket);
}

int logits_argmax_groups(int V) { return (V + 127) / 128; }

// f32 rows -> fragment-tiled f16 planes, chunk-major: fragment
// f = (chunk * groups + g) * KS + ks holds rows 16 g .. + 15, dims
// 128 chunk + 32 ks + 8 (lane >> 4) .. + 7; thread = (fragment, lane): 8 values
template <int NS>
__global__ __launch_bounds__(256) void emb_tiled_kernel(const float* __restrict__ x, int V, int D, int64_t nfrag,
                                                        _Float16* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nfrag * 64) return;
  const int lane = (int)(i & 63);
  constexpr int KS = kLg2Chunk / 32;
  const int64_t f = i >> 6;
  const int64_t groups = emb_groups16(V);
  const int64_t cg = f / KS;  // chunk * groups + g
  const int64_t chunk = cg / groups, g = cg - chunk * groups;
  const int s = (int)(chunk * KS + (f - cg * KS));
  const int64_t v = g * 16 + (lane & 15);
  const int k = s * 32 + 8 * (lane >> 4);
  half8 hi, lo;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 a = (_Float16)0.0f, b = (_Float16)0.0f;
    if (v < V) split_f16(x[v * D + k + j] * kEmbScale, a, b);
    hi[j] = a;
    lo[j] = b;
  }
  *reinterpret_cast<half8*>(out + (f * NS + 0) * 512 + lane * 8) = hi;
  if constexpr (NS == 2) *reinterpret_cast<half8*>(out + (f * NS + 1) * 512 + lane * 8) = lo;
}

bool emb_tiled_supported(int D) { return D % kLg2Chunk == 0; }
int64_t emb_tiled_rows(int V) { return (int64_t)logits_argmax_groups(V) * 128; }

hipError_t launch_emb_tiled(const float* emb, int V, int D, int ns, _Float16* out, hipStream_t st) {
  if (!emb_tiled_supported(D) || (ns != 1 && ns != 2)) return hipErrorInvalidValue;
  const int64_t nfrag = emb_tiled_rows(V) / 16 * (D / 32);
  const dim3 g((unsigned)((nfrag * 64 + 255) / 256));
  if (ns == 2)
    hipLaunchKernelGGL(emb_tiled_kernel<2>, g, dim3(256), 0, st, emb, V, D, nfrag, out);
  else
    hipLaunchKernelGGL(emb_tiled_kernel<1>, g, dim3(256), 0, st, emb, V, D, nfrag, out);
  return hipGetLastError();
}

int64_t logits_pick_scratch_floats(int V) { return (int64_t)2 * 5 * 32 * logits_argmax_groups(V); }

// The instantiation of a mode (every one has the same argument list):
// out_lp -> SUMS, rules -> two sides, temp -> KEYS, sup -> SUP.
template <int NS, int SUP>
static auto pick_kernel_mode(const PickArgs& p) -> decltype(&logits_argmax_f16_k32_kernel<NS, 1, 0, 0, SUP>) {
  if (p.temp)
    return p.rules ? &logits_argmax_f16_k32_kernel<NS, 2, 1, 1, SUP> : &logits_argmax_f16_k32_kernel<NS, 1, 1, 1, SUP>;
  if (p.rules) return &logits_argmax_f16_k32_kernel<NS, 2, 1, 0, SUP>;
  return p.out_lp ? &logits_argmax_f16_k32_kernel<NS, 1, 1, 0, SUP> : &logits_argmax_f16_k32_kernel<NS, 1, 0, 0, SUP>;
}
template <int NS>
static auto pick_kernel_of(const PickArgs& p) -> decltype(&logits_argmax_f16_k32_kernel<NS, 1, 0, 0, 0>) {
  return p.sup ? pick_kernel_mode<NS, 1>(p) : pick_kernel_mode<NS, 0>(p);
}

hipError_t launch_logits_pick(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                              int min_tokens, const DecodeState* state, const PickArgs& pick, const int* trace_ids,
                              float* trace_out, int trace_s1, int trace_k, int* range_flag, hipStream_t st) {
  if (B < 1 || B > 32 || !emb_tiled_supported(D) || !state || !emb2 || !htiled) return hipErrorInvalidValue;
  if (!pick.scratch || !pick.counter || !pick.out_tok) return hipErrorInvalidValue;
  // the log-probability comes with the timestamp rule and with sampling; a
  // sampled launch has both of temp / seed
  if (((pick.rules || pick.temp) && !pick.out_lp) || (pick.rules && pick.ts0 < 1) || !pick.temp != !pick.seed)
    return hipErrorInvalidValue;
  const auto kernel = ns == 2 ? pick_kernel_of<2>(pick) : pick_kernel_of<1>(pick);
  hipLaunchKernelGGL(kernel, dim3(logits_argmax_groups(V)), dim3(256), 0, st, htiled, B, D, emb2, V, min_tokens,
                     state, pick, trace_ids, trace_out, trace_s1, trace_k, range_flag);
  return hipGetLastError();
}

// ------------------------------------------------------ row log-prob --
// out[row * out_stride] = z[id] - logsumexp(z[lo:hi]) of the stored logit row
// z = logits + row * ld, id = idx ? idx[row * idx_stride] : fixed_idx, EOT
// treated as -inf when mask_eot (the pick's own masking, whisper.rs:97-98,
// 120-122; mask_state: when mask_state->step + 1 < min_tokens instead).  One
// workgroup per row, two passes over the range: the maximum, then
// sum exp(z - max) -- per thread ceil((hi - lo) / 256) terms, 6 shuffle adds,
// 3 adds over the waves -- and z[id] - max - log(sum).  A -inf entry adds 0;
// an id outside [lo, hi) or a row with no finite entry gives NaN.
__global__ __launch_bounds__(256) void row_logprob_kernel(const float* __restrict__ logits, int64_t ld, int lo, int hi,
                                                          int mask_eot, int min_tokens,
                                                          const DecodeState* __restrict__ mask_state,
                                                          const int* __restrict__ idx, int idx_stride, int fixed_idx,
                                                          float* __restrict__ out, int out_stride,
                                                          const uint32_t* __restrict__ sup) {
  __shared__ float sm[4];
  __shared__ float ss[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* z = logits + (size_t)b * ld;
  const bool mask = mask_state ? (mask_state->step + 1 < min_tokens) : mask_eot != 0;
  auto masked = [&](int i) { return (mask && i == kEOT) || sup_masked(sup, i); };
  float m = -INFINITY;
  for (int i = lo + tid; i < hi; i += 256) {
    const float v = masked(i) ? -INFINITY : z[i];
    m = fmaxf(m, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) sm[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float s = 0.0f;
  if (m > -INFINITY)
    for (int i = lo + tid; i < hi; i += 256) {
      const float v = masked(i) ? -INFINITY : z[i];
      s += expf(v - m);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) ss[wave] = s;
  __syncthreads();
  if (tid == 0) {
    s = ((ss[0] + ss[1]) + ss[2]) + ss[3];
    const int id = idx ? idx[(size_t)b * idx_stride] : fixed_idx;
    float r = NAN;
    if (id >= lo && id < hi && m > -INFINITY) {
      const float v = masked(id) ? -INFINITY : z[id];
      r = (v - m) - logf(s);
    }
    out[(size_t)b * out_stride] = r;
  }
}

hipError_t launch_row_logprob(const float* logits, int rows, int64_t ld, int lo, int hi, int mask_eot, int min_tokens,
                              const DecodeState* mask_state, const int* idx, int idx_stride, int fixed_idx, float* out,
                              int out_stride, hipStream_t st, const uint32_t* sup) {
  if (rows < 1 || lo < 0 || lo >= hi || hi > ld || !logits || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(row_logprob_kernel, dim3(rows), dim3(256), 0, st, logits, ld, lo, hi, mask_eot, min_tokens,
                     mask_state, idx, idx_stride, fixed_idx, out, out_stride, sup);
  return hipGetLastError();
}

// exp of every entry, in place (row log-probabilities -> probabilities)
__global__ void exp_inplace_kernel(float* __restrict__ x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = expf(x[i]);
}

hipError_t launch_exp_inplace(float* x, int n, hipStream_t st) {
  hipLaunchKernelGGL(exp_inplace_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, n);
  return hipGetLastError();
}

// ------------------------------------------------------------ bookkeep --
// logprob non-null (scored transcribes): the pick's log-probability next_lp[b]
// goes where its token goes, logprob[b][ntok[b]] (rows of max_tokens + 1), and
// the EOT pick that ends a clip leaves its own in the slot after the clip's
// last token.  rules non-null (timestamp transcribes): every row's rule record
// also advances by the token that is fed to this step (ts_rule_step), done
// clips included -- their picks go nowhere, and a record of any history leaves
// a non-empty allowed set.  Both tests are of kernel arguments: wave-uniform.
__global__ void bookkeep_kernel(const int* __restrict__ next, const float* __restrict__ next_lp,
                                int* __restrict__ tokens, float* __restrict__ logprob, int* __restrict__ ntok,
                                int* __restrict__ done, int B, int max_tokens, int eot_stop, DecodeState* state,
                                TsRule* __restrict__ rules, int ts0, int V) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int tk = next[b];
    if (!done[b]) {
      float* const lp_slot = logprob ? logprob + (size_t)b * (max_tokens + 1) + ntok[b] : nullptr;
      if (eot_stop && tk == kEOT) {
        done[b] = 1;
        atomicAdd(&state->n_done, 1);
        if (lp_slot) *lp_slot = next_lp[b];
      } else if (ntok[b] < max_tokens) {
        tokens[(size_t)b * max_tokens + ntok[b]] = tk;
        if (lp_slot) *lp_slot = next_lp[b];
        ntok[b] += 1;
      }
    }
    if (rules) rules[b] = ts_rule_step(rules[b], tk, ts0, V);
  }
  if (threadIdx.x == 0) {
    state->position += 1;
    state->kv_len += 1;
    state->step += 1;
  }
}

hipError_t launch_bookkeep(const int* next_tok, const float* next_lp, int* tokens, float* logprob, int* n_tokens,
                           int* done, int B, int max_tokens, int eot_stop, DecodeState* state, TsRule* rules, int ts0,
                           int V, hipStream_t st) {
  if (!logprob != !next_lp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bookkeep_kernel, dim3(1), dim3(256), 0, st, next_tok, next_lp, tokens, logprob, n_tokens, done, B,
                     max_tokens, eot_stop, state, rules, ts0, V);
  return hipGetLastError();
}


// dst[i] = src[i * stride], i < n
__global__ void gather_int_kernel(const int* __restrict__ src, int stride, int* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[(size_t)i * stride];
}

hipError_t launch_gather_int(const int* src, int stride, int* dst, int n, hipStream_t st) {
  hipLaunchKernelGGL(gather_int_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, stride, dst, n);
  return hipGetLastError();
}

// ------------------------------------------------------ pick of a row --
// The timestamp (KEYS = 0) or sampled (KEYS = 1) pick over a stored logit row
// (the prompt's pick, pick 0, and decode groups wider than 32 rows): under the
// timestamp rule, or (rules null) with EOT suppression only and the whole row
// on side 0.  One workgroup per row, two passes -- each side's PickSide under
// the masks, then each side's sum exp(z - max) -- and pick_decide in thread 0.
// Per side a thread adds ceil(V / 256) terms, 6 shuffle adds, 3 adds over the
// waves: row_logprob_kernel's order.  temp / seed are read under KEYS only.
template <int KEYS>
__global__ __launch_bounds__(256) void row_pick_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                       int suppress_fixed, int min_tokens,
                                                       const DecodeState* __restrict__ state,
                                                       const TsRule* __restrict__ rules, int ts0_rule,
                                                       const float* __restrict__ temp,
                                                       const uint64_t* __restrict__ seed, int pick_fixed,
                                                       int* __restrict__ out_tok, float* __restrict__ out_lp,
                                                       int* __restrict__ out_mass, int* __restrict__ range_flag,
                                                       const uint32_t* __restrict__ sup) {
  __shared__ float sf[KEYS ? 4 : 2][2][4];  // per side and wave: max, sum (KEYS: key, raw logit)
  __shared__ int si[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* z = logits + (size_t)b * ld;
  const bool suppress = state ? (state->step + 1 < min_tokens) : suppress_fixed != 0;
  const int ts0 = rules ? ts0_rule : V;
  int4 rule = {};
  if (rules) rule = *reinterpret_cast<const int4*>(rules + b);
  auto masked = [&](int i) {
    return sup_masked(sup, i) || (rules ? ts_masked(i, ts0, rule, suppress) : (suppress && i == kEOT));
  };
  float T = 0.0f;
  uint64_t nk = 0;
  if constexpr (KEYS) {
    T = temp[b];
    nk = T > 0.0f ? smp_pick_key(seed[b], state ? state->step + 1 : pick_fixed) : 0;
  }
  PickSide sd[2];
  bool bad = false;
  for (int i = tid; i < V; i += 256) {
    PickSide one;
    one.m = z[i];
    one.i = i;
    bad |= !__builtin_isfinite(one.m);
    if (masked(i)) one.m = -INFINITY;
    if constexpr (KEYS) {
      one.k = smp_key(one.m, T, nk, i);
      one.z = one.m;
    }
    if (i < ts0)
      pick_merge<KEYS>(sd[0], one);
    else
      pick_merge<KEYS>(sd[1], one);
  }
  if (bad && range_flag) *range_flag = 1;  // plain vector store: every writer stores 1
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int s = 0; s < 2; ++s) pick_merge_xor<KEYS>(sd[s], o);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sf[0][s][wave] = sd[s].m;
      si[s][wave] = sd[s].i;
      if constexpr (KEYS) {
        sf[2][s][wave] = sd[s].k;
        sf[3][s][wave] = sd[s].z;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    sd[s] = PickSide{};
    for (int w = 0; w < 4; ++w) {
      PickSide c;
      c.m = sf[0][s][w];
      c.i = si[s][w];
      if constexpr (KEYS) {
        c.k = sf[2][s][w];
        c.z = sf[3][s][w];
      }
      pick_merge<KEYS>(sd[s], c);
    }
  }
  for (int i = tid; i < V; i += 256) {
    const float v = masked(i) ? -INFINITY : z[i];
    if (i < ts0) {
      if (sd[0].m > -INFINITY) sd[0].s += expf(v - sd[0].m);
    } else {
      if (sd[1].m > -INFINITY) sd[1].s += expf(v - sd[1].m);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int s = 0; s < 2; ++s) sd[s].s += __shfl_xor(sd[s].s, o, 64);
  if (lane == 0) {
    sf[1][0][wave] = sd[0].s;
    sf[1][1][wave] = sd[1].s;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) sd[s].s = ((sf[1][s][0] + sf[1][s][1]) + sf[1][s][2]) + sf[1][s][3];
    int tok, mass;
    float lp;
    pick_decide<2, 1, KEYS>(sd[0], sd[1], tok, lp, mass);  // an empty timestamp side: -log s, no mass
    out_tok[b] = tok;
    if (out_lp) out_lp[b] = lp;
    if (out_mass) out_mass[b] = mass;
  }
}

hipError_t launch_row_pick(const float* logits, int rows, int64_t ld, int V, int suppress_eot, int min_tokens,
                           const DecodeState* state, const TsRule* rules, int ts0, const float* temp,
                           const uint64_t* seed, int pick, int* out_tok, float* out_lp, int* out_mass,
                           int* range_flag, hipStream_t st, const uint32_t* sup) {
  if (rows < 1 || V < 1 || V > ld || !logits || !out_tok || (rules && ts0 < 1) || !temp != !seed || pick < 0)
    return hipErrorInvalidValue;
  if (temp)
    hipLaunchKernelGGL(row_pick_kernel<1>, dim3(rows), dim3(256), 0, st, logits, ld, V, suppress_eot, min_tokens, state,
                       rules, ts0, temp, seed, pick, out_tok, out_lp, out_mass, range_flag, sup);
  else
    hipLaunchKernelGGL(row_pick_kernel<0>, dim3(rows), dim3(256), 0, st, logits, ld, V, suppress_eot, min_tokens, state,
                       rules, ts0, temp, seed, pick, out_tok, out_lp, out_mass, range_flag, sup);
  return hipGetLastError();
}


}  // namespace wa
