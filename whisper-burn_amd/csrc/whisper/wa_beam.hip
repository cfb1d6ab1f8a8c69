// wa_beam.hip -- gfx950 kernels of beam-search decoding (wa_beam.hpp; the
// semantics: include/whisper_amd.h, "Beam search"): the per-row log-softmax +
// top-(K + 1) and the per-clip merge that keeps K beams, files the finished
// sequences and advances the decode state.  The step's self-attention over the
// ancestor table sits beside the kernel it mirrors (wa_kernels.hip).
//
// Reference semantics: openai/whisper decoding.py, BeamSearchDecoder.update
// (written out in the header; the dictionary order of the original replaced by
// a total order).
#include <hip/hip_runtime.h>

#include "wa_beam.hpp"
#include "wa_tsrule.hpp"

namespace wa {

namespace {

constexpr int kEOT = 50257;
constexpr int kTop = kBeamMaxTop;

// The one order of the picks (wa_pick.hip `better`): larger value first, equal
// values: larger id first ("last maximum wins").
__device__ __forceinline__ bool ahead(float v, int i, float bv, int bi) { return v > bv || (v == bv && i > bi); }

// Sorted insertion into a thread's top kTop, every index static (registers).
__device__ __forceinline__ void top_insert(float (&tv)[kTop], int (&ti)[kTop], float v, int i) {
  if (!ahead(v, i, tv[kTop - 1], ti[kTop - 1])) return;
#pragma unroll
  for (int k = 0; k < kTop; ++k) {
    if (ahead(v, i, tv[k], ti[k])) {
      const float fv = tv[k];
      const int fi = ti[k];
      tv[k] = v;
      ti[k] = i;
      v = fv;
      i = fi;
    }
  }
}

// (m, s) <- (m, s) + (m2, s2): s = sum exp(z - m) over both parts.  At most
// three roundings (two products, one of them by exp(0) = 1, and the sum).
__device__ __forceinline__ void lse_join(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx == -INFINITY) {
    s = 0.0f;
  } else {
    s = s * expf(m - mx) + s2 * expf(m2 - mx);
  }
  m = mx;
}

// ------------------------------------------------------------ beam_topk --
// One workgroup per row.  A thread walks its elements once -- groups of four
// 256 groups apart, then one of the up to 3 left over -- keeping (m, s) online
// (a new maximum rescales s: two roundings per element at most) and its sorted
// top 9.  Then 6 shuffle joins, 3
// joins over the waves, and kp rounds of a workgroup-wide maximum over the
// threads' list heads, the winner popping its head.
__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits, int64_t ld, int V, int kp,
                                                        int suppress_fixed, int min_tokens, int eot_stop,
                                                        const DecodeState* __restrict__ state,
                                                        int* __restrict__ out_tok, float* __restrict__ out_lp,
                                                        int* __restrict__ range_flag,
                                                        const uint32_t* __restrict__ sup) {
  __shared__ float sm[4], ss[4];
  __shared__ float cv[2][4];
  __shared__ int ci[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* z = logits + (size_t)row * ld;
  const bool mask = !eot_stop || (state ? (state->step + 1 < min_tokens) : suppress_fixed != 0);
  float tv[kTop];
  int ti[kTop];
#pragma unroll
  for (int k = 0; k < kTop; ++k) {
    tv[k] = -INFINITY;
    ti[k] = -1;
  }
  float m = -INFINITY, s = 0.0f;
  bool bad = false;
  auto take = [&](float raw, int i, bool listed) {
    bad |= !__builtin_isfinite(raw);
    const float v = (listed || (mask && i == kEOT)) ? -INFINITY : raw;
    if (v > m) {
      s = s * expf(m - v) + 1.0f;  // m = -inf: s = 0 * 0 + 1
      m = v;
    } else if (v > -INFINITY) {
      s += expf(v - m);
    }
    top_insert(tv, ti, v, i);
  };
  // Elements go to threads by index alone (4 c .. 4 c + 3 to thread c mod 256),
  // never by the row's address: a row's bits do not depend on where it sits.
  // The address only picks the load width (wave-uniform).
  const uintptr_t addr = reinterpret_cast<uintptr_t>(z);
  const int nvec = V >> 2, tail0 = 4 * nvec;
  auto load4 = [&](int i0) {
    if ((addr & 15) == 0) return *reinterpret_cast<const float4*>(z + i0);
    if ((addr & 7) == 0) {
      const float2 a = *reinterpret_cast<const float2*>(z + i0), b = *reinterpret_cast<const float2*>(z + i0 + 2);
      return make_float4(a.x, a.y, b.x, b.y);
    }
    return make_float4(z[i0], z[i0 + 1], z[i0 + 2], z[i0 + 3]);
  };
  // kTopLoads groups in flight per thread (clamped addresses: the loads never
  // branch), taken in ascending order: the sums are those of a one-by-one walk
  // sup (a model with suppress lists; a kernel argument: wave-uniform): a
  // group's four ids share one mask word, loaded beside the group
  constexpr int kTopLoads = 8;
  for (int c0 = tid; c0 < nvec; c0 += 256 * kTopLoads) {
    float4 x[kTopLoads];
    uint32_t w[kTopLoads] = {};
#pragma unroll
    for (int u = 0; u < kTopLoads; ++u) x[u] = load4(4 * min(c0 + 256 * u, nvec - 1));
    if (sup) {
#pragma unroll
      for (int u = 0; u < kTopLoads; ++u) w[u] = sup[min(c0 + 256 * u, nvec - 1) >> 3];
    }
#pragma unroll
    for (int u = 0; u < kTopLoads; ++u) {
      const int c = c0 + 256 * u;
      if (c < nvec) {
        const int i0 = 4 * c;
        const uint32_t b4 = w[u] >> (i0 & 31);
        take(x[u].x, i0, b4 & 1u);
        take(x[u].y, i0 + 1, b4 & 2u);
        take(x[u].z, i0 + 2, b4 & 4u);
        take(x[u].w, i0 + 3, b4 & 8u);
      }
    }
  }
  if (tail0 + tid < V && tid < 3) take(z[tail0 + tid], tail0 + tid, sup_masked(sup, tail0 + tid));
  if (bad && range_flag) *range_flag = 1;  // plain vector store: every writer stores 1
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_join(m, s, m2, s2);
  }
  if (lane == 0) {
    sm[wave] = m;
    ss[wave] = s;
  }
  __syncthreads();
  m = sm[0];
  s = ss[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) lse_join(m, s, sm[w], ss[w]);
  const float logs = logf(s);
  for (int r = 0; r < kp; ++r) {
    float bv = tv[0];
    int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (ahead(v2, i2, bv, bi)) {
        bv = v2;
        bi = i2;
      }
    }
    if (lane == 0) {
      cv[r & 1][wave] = bv;
      ci[r & 1][wave] = bi;
    }
    __syncthreads();
    bv = cv[r & 1][0];
    bi = ci[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (ahead(cv[r & 1][w], ci[r & 1][w], bv, bi)) {
        bv = cv[r & 1][w];
        bi = ci[r & 1][w];
      }
    if (bi >= 0 && ti[0] == bi) {  // ids are unique: one thread pops
#pragma unroll
      for (int k = 0; k + 1 < kTop; ++k) {
        tv[k] = tv[k + 1];
        ti[k] = ti[k + 1];
      }
      tv[kTop - 1] = -INFINITY;
      ti[kTop - 1] = -1;
    }
    if (tid == 0) {
      out_tok[(size_t)row * kp + r] = max(bi, 0);
      out_lp[(size_t)row * kp + r] = bi < 0 ? NAN : (bv - m) - logs;
    }
  }
}

// ------------------------------------------------------ beam_topk_rules --
// beam_topk under the timestamp rules: row r's record gives masks a-e as id
// range tests at load (ts_masked).  Rule f needs both sides before the
// denominator and the list are known, so the row (207 KB, L2-resident) is
// walked twice with the walk of the plain kernel: walk 1 keeps the text side's
// maximum and the timestamp side's online (m, s) -- a handful of registers --
// and the workgroup decides mass = logsumexp(timestamps) > max(text, EOT) as
// ts_decide (wa_pick.hip) does; walk 2 is the plain kernel's, with the text
// side masked as well where the rule fired.  Carrying per-side lists through
// one walk would double the 18 list registers instead.  A masked id enters the
// lists as -inf and leaves as (0, -inf): not a candidate.
template <class F>
__device__ __forceinline__ void row_walk(const float* __restrict__ z, int V, int tid,
                                         const uint32_t* __restrict__ sup, F&& take) {
  // as beam_topk_kernel: elements go to threads by index alone, the address
  // only picks the load width
  const uintptr_t addr = reinterpret_cast<uintptr_t>(z);
  const int nvec = V >> 2, tail0 = 4 * nvec;
  auto load4 = [&](int i0) {
    if ((addr & 15) == 0) return *reinterpret_cast<const float4*>(z + i0);
    if ((addr & 7) == 0) {
      const float2 a = *reinterpret_cast<const float2*>(z + i0), b = *reinterpret_cast<const float2*>(z + i0 + 2);
      return make_float4(a.x, a.y, b.x, b.y);
    }
    return make_float4(z[i0], z[i0 + 1], z[i0 + 2], z[i0 + 3]);
  };
  // sup: as beam_topk_kernel, one mask word per group of four ids
  constexpr int kTopLoads = 8;
  for (int c0 = tid; c0 < nvec; c0 += 256 * kTopLoads) {
    float4 x[kTopLoads];
    uint32_t w[kTopLoads] = {};
#pragma unroll
    for (int u = 0; u < kTopLoads; ++u) x[u] = load4(4 * min(c0 + 256 * u, nvec - 1));
    if (sup) {
#pragma unroll
      for (int u = 0; u < kTopLoads; ++u) w[u] = sup[min(c0 + 256 * u, nvec - 1) >> 3];
    }
#pragma unroll
    for (int u = 0; u < kTopLoads; ++u) {
      const int c = c0 + 256 * u;
      if (c < nvec) {
        const int i0 = 4 * c;
        const uint32_t b4 = w[u] >> (i0 & 31);
        take(x[u].x, i0, b4 & 1u);
        take(x[u].y, i0 + 1, b4 & 2u);
        take(x[u].z, i0 + 2, b4 & 4u);
        take(x[u].w, i0 + 3, b4 & 8u);
      }
    }
  }
  if (tail0 + tid < V && tid < 3) take(z[tail0 + tid], tail0 + tid, sup_masked(sup, tail0 + tid));
}

__global__ __launch_bounds__(256) void beam_topk_rules_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                              int kp, int suppress_fixed, int min_tokens,
                                                              int eot_stop, const DecodeState* __restrict__ state,
                                                              const TsRule* __restrict__ rules, int ts0,
                                                              int* __restrict__ out_tok, float* __restrict__ out_lp,
                                                              int* __restrict__ out_mass,
                                                              int* __restrict__ range_flag,
                                                              const uint32_t* __restrict__ sup) {
  __shared__ float pt[4], pm[4], ps[4];  // walk 1: text maximum, timestamp (m, s) per wave
  __shared__ float sm[4], ss[4];
  __shared__ float cv[2][4];
  __shared__ int ci[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* z = logits + (size_t)row * ld;
  const bool mask = !eot_stop || (state ? (state->step + 1 < min_tokens) : suppress_fixed != 0);
  const int4 rule = *reinterpret_cast<const int4*>(rules + row);
  // ---- walk 1: rule f from the row after masks a-e
  float mt = -INFINITY, mx = -INFINITY, sx = 0.0f;
  row_walk(z, V, tid, sup, [&](float raw, int i, bool listed) {
    if (listed || ts_masked(i, ts0, rule, mask)) return;
    if (i < ts0) {
      mt = fmaxf(mt, raw);
    } else if (raw > mx) {
      sx = sx * expf(mx - raw) + 1.0f;
      mx = raw;
    } else if (raw > -INFINITY) {
      sx += expf(raw - mx);
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mt = fmaxf(mt, __shfl_xor(mt, o, 64));
    const float m2 = __shfl_xor(mx, o, 64), s2 = __shfl_xor(sx, o, 64);
    lse_join(mx, sx, m2, s2);
  }
  if (lane == 0) {
    pt[wave] = mt;
    pm[wave] = mx;
    ps[wave] = sx;
  }
  __syncthreads();
  mt = fmaxf(fmaxf(pt[0], pt[1]), fmaxf(pt[2], pt[3]));
  mx = pm[0];
  sx = ps[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) lse_join(mx, sx, pm[w], ps[w]);
  const float lse_x = mx > -INFINITY ? mx + logf(sx) : -INFINITY;
  const bool mass = lse_x > mt;  // every thread: the same LDS values, the same decision
  if (tid == 0 && out_mass) out_mass[row] = mass ? 1 : 0;
  // ---- walk 2: the plain kernel over the finally masked row
  float tv[kTop];
  int ti[kTop];
#pragma unroll
  for (int k = 0; k < kTop; ++k) {
    tv[k] = -INFINITY;
    ti[k] = -1;
  }
  float m = -INFINITY, s = 0.0f;
  bool bad = false;
  row_walk(z, V, tid, sup, [&](float raw, int i, bool listed) {
    bad |= !__builtin_isfinite(raw);  // the range flag: the raw logits
    const float v = (listed || ts_masked(i, ts0, rule, mask) || (mass && i < ts0)) ? -INFINITY : raw;
    if (v > m) {
      s = s * expf(m - v) + 1.0f;  // m = -inf: s = 0 * 0 + 1
      m = v;
    } else if (v > -INFINITY) {
      s += expf(v - m);
    }
    top_insert(tv, ti, v, i);
  });
  if (bad && range_flag) *range_flag = 1;  // plain vector store: every writer stores 1
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_join(m, s, m2, s2);
  }
  if (lane == 0) {
    sm[wave] = m;
    ss[wave] = s;
  }
  __syncthreads();
  m = sm[0];
  s = ss[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) lse_join(m, s, sm[w], ss[w]);
  const float logs = logf(s);
  for (int r = 0; r < kp; ++r) {
    float bv = tv[0];
    int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (ahead(v2, i2, bv, bi)) {
        bv = v2;
        bi = i2;
      }
    }
    if (lane == 0) {
      cv[r & 1][wave] = bv;
      ci[r & 1][wave] = bi;
    }
    __syncthreads();
    bv = cv[r & 1][0];
    bi = ci[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (ahead(cv[r & 1][w], ci[r & 1][w], bv, bi)) {
        bv = cv[r & 1][w];
        bi = ci[r & 1][w];
      }
    if (bi >= 0 && ti[0] == bi) {  // ids are unique: one thread pops
#pragma unroll
      for (int k = 0; k + 1 < kTop; ++k) {
        tv[k] = tv[k + 1];
        ti[k] = ti[k + 1];
      }
      tv[kTop - 1] = -INFINITY;
      ti[kTop - 1] = -1;
    }
    if (tid == 0) {
      const bool cand = bi >= 0 && bv > -INFINITY;  // fewer allowed ids than kp: the surplus is (0, -inf)
      out_tok[(size_t)row * kp + r] = cand ? bi : 0;
      out_lp[(size_t)row * kp + r] = cand ? (bv - m) - logs : -INFINITY;
    }
  }
}

// ---------------------------------------------------------- beam_select --
__global__ __launch_bounds__(128) void beam_select_kernel(BeamSelect a, int n_clips, int K, int C, int ctx, int ts0,
                                                          int V) {
  constexpr int kCand = kBeamMaxK * kBeamMaxTop;
  __shared__ float sc[kCand];
  __shared__ int tk[kCand];
  __shared__ float nS[kBeamMaxK], fSum[kBeamMaxK];
  __shared__ int nTok[kBeamMaxK], nPar[kBeamMaxK], fSrc[kBeamMaxK];
  __shared__ TsRule pr[kBeamMaxK];  // the clip's parent records, staged before any is rewritten
  __shared__ int nMet;
  const int clip = blockIdx.x, tid = threadIdx.x;
  const int KP = K + 1, NC = K * KP, rows = n_clips * K, r0 = clip * K;
  // the state before this step's advance: read here, advanced by the last workgroup (below)
  const int kv_len = a.state->kv_len, step = a.state->step;
  const int cur = (step + 1) & 1;
  const int* anc_cur = a.anc + (size_t)cur * rows * ctx;
  int* anc_nxt = a.anc + (size_t)(cur ^ 1) * rows * ctx;
  const int fin0 = a.fin_n[clip];
  const bool was_complete = a.complete[clip] != 0;
  if (tid < kBeamMaxK) {  // a beam no candidate fills: dead (-inf), feeds token 0, continues itself
    nS[tid] = -INFINITY;
    nTok[tid] = 0;
    nPar[tid] = tid;
    fSrc[tid] = -1;
  }
  if (tid == 0) nMet = 0;
  if (a.rules && tid < K) pr[tid] = a.rules[r0 + tid];
  float s = -INFINITY;
  int t = 0;
  const int j = tid / KP;
  if (tid < NC) {
    s = a.S[r0 + j] + a.top_lp[(size_t)r0 * KP + tid];  // one f32 addition
    t = a.top_tok[(size_t)r0 * KP + tid];
    if (!(s > -INFINITY)) s = -INFINITY;  // -inf (and NaN) candidates are dropped
    sc[tid] = s;
    tk[tid] = t;
  }
  __syncthreads();
  if (tid < NC && s > -INFINITY) {
    int nn = 0, ne = 0;  // non-EOT / EOT candidates in front of this one
    for (int u = 0; u < NC; ++u) {
      const float su = sc[u];
      if (su > s || (su == s && u < tid)) {  // (j, i) ascending = the candidate index ascending
        if (tk[u] == kEOT) ++ne; else ++nn;
      }
    }
    if (nn < K) {  // the walk has not stopped
      if (t != kEOT) {
        nS[nn] = s;
        nTok[nn] = t;
        nPar[nn] = j;
      } else {
        atomicAdd(&nMet, 1);
        if (!was_complete && fin0 + ne < C && ne < kBeamMaxK) {
          fSrc[ne] = j;
          fSum[ne] = s;
        }
      }
    }
  }
  __syncthreads();
  const bool room = kv_len + 1 < ctx;
  if (tid < K) {
    a.S[r0 + tid] = nS[tid];
    a.next_tok[r0 + tid] = nTok[tid];
    a.parent[r0 + tid] = r0 + nPar[tid];
    // the new beam's history is its parent's plus its token (a dead beam: its own plus token 0)
    if (a.rules) a.rules[r0 + tid] = ts_rule_step(pr[nPar[tid]], nTok[tid], ts0, V);
    if (room) {
      a.fed[(size_t)(kv_len + 1) * rows + r0 + tid] = nTok[tid];
      anc_nxt[(size_t)(r0 + tid) * ctx + kv_len + 1] = r0 + tid;
    }
  }
  const int ncopy = min(kv_len + 1, ctx);
  for (int n = 0; n < K; ++n) {
    const int* src = anc_cur + (size_t)(r0 + nPar[n]) * ctx;
    int* dst = anc_nxt + (size_t)(r0 + n) * ctx;
    for (int p = tid; p < ncopy; p += 128) dst[p] = src[p];
  }
  for (int e = 0; e < kBeamMaxK; ++e) {
    if (fSrc[e] < 0) continue;
    const size_t f = (size_t)clip * C + fin0 + e;
    const int* src = anc_cur + (size_t)(r0 + fSrc[e]) * ctx;
    for (int p = tid; p < ncopy; p += 128) a.fin_anc[f * ctx + p] = src[p];
    if (tid == 0) {
      a.fin_sum[f] = fSum[e];
      a.fin_len[f] = step + 1;
    }
  }
  if (tid == 0 && !was_complete) {
    const int n = min(C, fin0 + nMet);
    a.fin_n[clip] = n;
    if (n >= C) {
      a.complete[clip] = 1;
      atomicAdd(&a.state->n_done, 1);
    }
  }
  __syncthreads();
  // Every workgroup read the state above; the one whose ticket is the last
  // advances it and re-arms the counter (what launch_bookkeep does for a
  // greedy step).  No bytes are handed between workgroups.
  if (tid == 0) {
    typedef __attribute__((address_space(1))) int gint;
    const int prev = __hip_atomic_fetch_add((gint*)a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == n_clips - 1) {
      __hip_atomic_store((gint*)a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.state->position += 1;
      a.state->kv_len += 1;
      a.state->step += 1;
    }
  }
}

}  // namespace

hipError_t launch_beam_topk(const float* logits, int rows, int64_t ld, int V, int kp, int suppress_fixed, int min_tokens,
                            int eot_stop, const DecodeState* state, int* out_tok, float* out_lp, int* range_flag,
                            hipStream_t st, const uint32_t* sup) {
  if (rows < 1 || V < 16 || ld < V || kp < 2 || kp > kBeamMaxTop || !logits || !out_tok || !out_lp)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(rows), dim3(256), 0, st, logits, ld, V, kp, suppress_fixed, min_tokens,
                     eot_stop, state, out_tok, out_lp, range_flag, sup);
  return hipGetLastError();
}

hipError_t launch_beam_topk_rules(const float* logits, int rows, int64_t ld, int V, int kp, int suppress_fixed,
                                  int min_tokens, int eot_stop, const DecodeState* state, const TsRule* rules, int ts0,
                                  int* out_tok, float* out_lp, int* out_mass, int* range_flag, hipStream_t st,
                                  const uint32_t* sup) {
  if (rows < 1 || V < 16 || ld < V || kp < 2 || kp > kBeamMaxTop || !logits || !out_tok || !out_lp || !rules ||
      ts0 <= kEOT || ts0 > V)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_topk_rules_kernel, dim3(rows), dim3(256), 0, st, logits, ld, V, kp, suppress_fixed,
                     min_tokens, eot_stop, state, rules, ts0, out_tok, out_lp, out_mass, range_flag, sup);
  return hipGetLastError();
}

hipError_t launch_beam_select(const BeamSelect& a, int n_clips, int K, int C, int ctx, hipStream_t st, int ts0,
                              int V) {
  if (n_clips < 1 || K < 1 || K > kBeamMaxK || C < K || C > kBeamMaxCand || ctx < 2) return hipErrorInvalidValue;
  if (a.rules && (ts0 < 1 || V < ts0)) return hipErrorInvalidValue;
  for (const void* p : {(const void*)a.top_tok, (const void*)a.top_lp, (const void*)a.S, (const void*)a.next_tok,
                        (const void*)a.parent, (const void*)a.anc, (const void*)a.fed, (const void*)a.fin_sum,
                        (const void*)a.fin_len, (const void*)a.fin_anc, (const void*)a.fin_n, (const void*)a.complete,
                        (const void*)a.ticket, (const void*)a.state})
    if (!p) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_select_kernel, dim3(n_clips), dim3(128), 0, st, a, n_clips, K, C, ctx, ts0, V);
  return hipGetLastError();
}

}  // namespace wa
