// wa_checks.cpp -- C ABI entries that run one kernel on caller-supplied
// buffers (the wa_*_check test entries) and the log-mel front-end.
#include <cmath>
#include <map>
#include <mutex>

#include "wa_mel.hpp"
#include "wa_model.hpp"

using namespace wa;

namespace {

int planes(wq4_precision prec) { return prec == WQ4_PREC_F16 ? 1 : 2; }

// The scaffold of the attention checks: `launch` writes R rows of width D as
// the A-tiled GEMM operand into a zeroed buffer, returned as f32 rows.
template <class Launch>
wq4_status tiled_check(Dev& d, int64_t R, int D, wq4_precision prec, float* out_dev, Launch launch) {
  const size_t tb = wq4_atiled_bytes(R, D, prec);
  auto* tiled = d.alloc<_Float16>(tb / 2);
  if (!tiled) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(tiled, 0, tb));
  WA_HIP(launch(tiled));
  WA_HIP(launch_untile(tiled, (int)R, D, planes(prec), out_dev, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// The device mask of a check entry's id list (every id in [0, bound)), null
// for an empty list: the launch of the entry it extends.
wq4_status sup_upload(Dev& d, const int32_t* ids, int n_ids, int V, int bound, const uint32_t** out) {
  *out = nullptr;
  if (n_ids < 0 || (n_ids > 0 && !ids)) return fail(WQ4_EINVAL, "bad id list");
  for (int i = 0; i < n_ids; ++i)
    if (ids[i] < 0 || ids[i] >= bound) return fail(WQ4_EINVAL, "suppressed id outside [0, ts0)");
  if (n_ids == 0) return WQ4_OK;
  std::vector<uint32_t> words((size_t)sup_mask_words(V));
  sup_mask_build(ids, n_ids, V, words.data());
  auto* dev = d.alloc<uint32_t>(words.size());
  if (!dev) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(dev, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  *out = dev;
  return WQ4_OK;
}

// wa_beam_topk_check / wa_beam_topk_rules_check (records non-null) and their
// form under a list.
wq4_status beam_topk_check(int device, const float* logits_dev, int n_rows, int V, int kp, int suppress_eot, int step,
                           int eot_stop, int ts0, const int32_t* records, const int32_t* ids, int n_ids,
                           int32_t* tok_dev, float* lp_dev, int32_t* mass_dev, int32_t* flag_out) {
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, ids, n_ids, V, ts0 > 0 ? std::min(ts0, V) : V, &sup));
  auto* flag = d.alloc<int>(1);
  TsRule* rules = records ? d.alloc<TsRule>(n_rows) : nullptr;
  DecodeState* st = step >= 0 ? d.alloc<DecodeState>(1) : nullptr;
  if (!flag || (records && !rules) || (step >= 0 && !st)) return fail(WQ4_ENOMEM, "allocation failed");
  if (st) {
    const DecodeState s0{0, 0, step, 0};
    WA_HIP(hipMemcpy(st, &s0, sizeof(s0), hipMemcpyHostToDevice));
  }
  if (rules) WA_HIP(hipMemcpy(rules, records, (size_t)n_rows * sizeof(TsRule), hipMemcpyHostToDevice));
  WA_HIP(hipMemset(flag, 0, sizeof(int)));
  if (rules)
    WA_HIP(launch_beam_topk_rules(logits_dev, n_rows, V, V, kp, suppress_eot, kMinTokens, eot_stop, st, rules, ts0,
                                  tok_dev, lp_dev, mass_dev, flag, nullptr, sup));
  else
    WA_HIP(launch_beam_topk(logits_dev, n_rows, V, V, kp, suppress_eot, kMinTokens, eot_stop, st, tok_dev, lp_dev, flag,
                            nullptr, sup));
  int f = 0;
  WA_HIP(hipMemcpy(&f, flag, sizeof(int), hipMemcpyDeviceToHost));
  if (flag_out) *flag_out = f;
  return WQ4_OK;
}

}  // namespace

extern "C" {

wq4_status wa_xattn_check(int device, const float* q_dev, const uint8_t* wk_dev, const uint8_t* wv_dev,
                          const float* bv_dev, int weight_type, const float* enc_dev, int n_clips, int Tq, int T,
                          int H, wq4_precision prec, float* out_dev) {
  if (!q_dev || !wk_dev || !wv_dev || !bv_dev || !enc_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || Tq < 1 || T < 1 || H < 1) return fail(WQ4_EINVAL, "bad sizes");
  const int D = 64 * H, ns = planes(prec), R = n_clips * Tq;
  const int HP = (H + 15) / 16 * 16;
  WA_HIP(hipSetDevice(device));
  Dev d;
  auto* enc = d.alloc<_Float16>((size_t)n_clips * T * ns * D);
  auto* qt = d.alloc<_Float16>((size_t)R * ns * HP * D);
  auto* part = d.alloc<float>(xattn_part_floats(R, H, D, T));
  if (!enc || !qt || !part) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(qt, 0, (size_t)R * ns * HP * D * 2));
  WA_HIP(launch_enc_planes(enc_dev, (int64_t)n_clips * T, D, ns, enc, nullptr));
  uint32_t* wvp = nullptr;
  if (weight_type == 0) {
    wvp = d.alloc<uint32_t>(wv_pack_words(H, D));
    if (!wvp) return fail(WQ4_ENOMEM, "allocation failed");
    WA_HIP(launch_wv_pack(wv_dev, H, D, wvp, nullptr));
  }
  // the policy of a decode with these clips live (WA_XATTN_RESIDENT_MB: the tests force each share)
  const XattnResidency res = xattn_residency(n_clips, T, ns, D);
  // nothing runs beside the launch: the default plan (WA_XATTN_SPLITS_RT: the tests force each split count)
  const XattnPlan plan = xattn_plan(T, R);
  return tiled_check(d, R, D, prec, out_dev, [&](_Float16* tiled) {
    return launch_xattn(q_dev, wk_dev, wv_dev, wvp, bv_dev, weight_type, enc, n_clips, Tq, T, H, D, qt, part, tiled,
                        ns, res, plan, nullptr);
  });
}

int wa_xattn_resident_share(int live_clips, int T, int planes, int D, double budget_mb) {
  if (live_clips < 1 || T < 1 || planes < 1 || planes > 2 || D < 1) return -1;
  return xattn_residency(live_clips, T, planes, D, budget_mb).q;
}

int wa_xattn_chunk_resident(int chunk, int share) {
  if (chunk < 0 || share < 0 || share > kXattnResDen) return -1;
  return xattn_chunk_resident(chunk, share) ? 1 : 0;
}

wq4_status wa_xattn_plan(int T, int* splits, int* chunks_per_split) {
  if (T < 1 || !splits || !chunks_per_split) return fail(WQ4_EINVAL, "bad arguments");
  const XattnPlan p = xattn_plan(T, 1, 0, 0);
  *splits = p.splits;
  *chunks_per_split = p.ch;
  return WQ4_OK;
}

wq4_status wa_xattn_plan_splits(int T, int rows, int free_cus, int* splits, int* chunks_per_split) {
  if (T < 1 || rows < 1 || !splits || !chunks_per_split) return fail(WQ4_EINVAL, "bad arguments");
  const XattnPlan p = xattn_plan(T, rows, free_cus, 0);
  *splits = p.splits;
  *chunks_per_split = p.ch;
  return WQ4_OK;
}

long long wa_decode_graph_key(const wa_model* m, int group) {
  if (!m || group < 0 || group >= (int)m->groups.size()) return -1;
  return m->groups[group].graph_key;
}

long long wa_decode_graph_key_check(int mode, int lane, int b0, int nb, int eot, int trace, int group_kv,
                                    int range_tier, int splits, int residency) {
  return graph_key(mode, lane, b0, nb, eot, trace, group_kv, range_tier, splits, residency);
}

wq4_status wa_xattn_kv_check(int device, const float* q_dev, const float* k_dev, const float* v_dev, int n_clips,
                             int Tq, int T, int H, wq4_precision prec, float* out_dev) {
  if (!q_dev || !k_dev || !v_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || Tq < 1 || Tq > 4 || T < 1 || H < 1) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  auto* part = d.alloc<float>(cross_attention_kv_part_floats(n_clips, H, T));
  auto* ctr = d.alloc<int>((size_t)n_clips * H);
  if (!part || !ctr) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(ctr, 0, (size_t)n_clips * H * sizeof(int)));
  return tiled_check(d, n_clips * Tq, 64 * H, prec, out_dev, [&](_Float16* tiled) {
    return launch_cross_attention_kv(q_dev, k_dev, v_dev, n_clips, Tq, T, H, part, ctr, tiled, planes(prec), nullptr);
  });
}

wq4_status wa_encoder_attention_check(int device, const float* qkv_dev, int n_clips, int T, int H, wq4_precision prec,
                                      float* out_dev) {
  if (!qkv_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || T < 1 || H < 1) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  return tiled_check(d, (int64_t)n_clips * T, 64 * H, prec, out_dev, [&](_Float16* tiled) {
    return launch_encoder_attention(qkv_dev, n_clips, T, H, tiled, planes(prec), nullptr);
  });
}

wq4_status wa_self_attention_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                   int n_clips, int Tq, int H, int ctx, int kv_len, wq4_precision prec,
                                   float* out_dev) {
  if (!qkv_dev || !cache_k_dev || !cache_v_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || Tq < 1 || Tq > 4 || H < 1 || ctx < 1 || ctx > 448 || kv_len < 0 || kv_len + Tq > ctx)
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  return tiled_check(d, n_clips * Tq, 64 * H, prec, out_dev, [&](_Float16* tiled) {
    return launch_decoder_self_attention(qkv_dev, cache_k_dev, cache_v_dev, n_clips, Tq, H, ctx, nullptr, kv_len,
                                         tiled, planes(prec), nullptr);
  });
}

// ---- beam search: the product kernels on caller data ----------------------
wq4_status wa_self_attention_beam_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                        const int32_t* anc_dev, int n_rows, int H, int ctx, int kv_len,
                                        wq4_precision prec, int f32_out, float* out_dev) {
  if (!qkv_dev || !cache_k_dev || !cache_v_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || H < 1 || ctx < 1 || ctx > 448 || kv_len < 0 || kv_len + 1 > ctx)
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  if (anc_dev) {  // every entry names a cache row
    std::vector<int32_t> anc((size_t)n_rows * ctx);
    WA_HIP(hipMemcpy(anc.data(), anc_dev, anc.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_rows; ++r)
      for (int j = 0; j < kv_len; ++j)
        if (anc[(size_t)r * ctx + j] < 0 || anc[(size_t)r * ctx + j] >= n_rows)
          return fail(WQ4_EINVAL, "ancestor row outside [0, n_rows)");
  }
  auto launch = [&](_Float16* tiled, float* out32) {
    return anc_dev ? launch_decoder_self_attention_beam(qkv_dev, cache_k_dev, cache_v_dev, n_rows, H, ctx, nullptr,
                                                        kv_len, anc_dev, tiled, planes(prec), nullptr, out32)
                   : launch_decoder_self_attention(qkv_dev, cache_k_dev, cache_v_dev, n_rows, 1, H, ctx, nullptr,
                                                   kv_len, tiled, planes(prec), nullptr, out32);
  };
  if (f32_out) {
    WA_HIP(launch(nullptr, out_dev));
    WA_HIP(hipDeviceSynchronize());
    return WQ4_OK;
  }
  Dev d;
  return tiled_check(d, n_rows, 64 * H, prec, out_dev, [&](_Float16* tiled) { return launch(tiled, nullptr); });
}

wq4_status wa_beam_topk_check(int device, const float* logits_dev, int n_rows, int V, int kp, int suppress_eot,
                              int step, int eot_stop, int32_t* tok_dev, float* lp_dev, int32_t* flag_out) {
  if (!logits_dev || !tok_dev || !lp_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || V < 16 || kp < 2 || kp > kBeamMaxTop) return fail(WQ4_EINVAL, "bad sizes");
  return beam_topk_check(device, logits_dev, n_rows, V, kp, suppress_eot, step, eot_stop, 0, nullptr, nullptr, 0, tok_dev,
                         lp_dev, nullptr, flag_out);
}

wq4_status wa_beam_topk_suppress_check(int device, const float* logits_dev, int n_rows, int V, int kp,
                                       int suppress_eot, int step, int eot_stop, int ts0, const int32_t* ids,
                                       int n_ids, const int32_t* records, int32_t* tok_dev, float* lp_dev,
                                       int32_t* mass_dev, int32_t* flag_out) {
  if (!logits_dev || !tok_dev || !lp_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || V < 16 || kp < 2 || kp > kBeamMaxTop || ts0 <= 50257 || ts0 > V)
    return fail(WQ4_EINVAL, "bad sizes");
  return beam_topk_check(device, logits_dev, n_rows, V, kp, suppress_eot, step, eot_stop, ts0, records, ids, n_ids,
                         tok_dev, lp_dev, mass_dev, flag_out);
}

static_assert(sizeof(DecodeState) == 4 * sizeof(int32_t), "the decode state is 4 int32 at the ABI");

wq4_status wa_beam_select_check(int device, const int32_t* top_tok_dev, const float* top_lp_dev, float* S_dev,
                                int32_t* next_tok_dev, int32_t* parent_dev, int32_t* anc_dev, int32_t* fed_dev,
                                float* fin_sum_dev, int32_t* fin_len_dev, int32_t* fin_anc_dev, int32_t* fin_n_dev,
                                int32_t* complete_dev, int32_t* state_dev, int n_clips, int K, int C, int ctx) {
  if (!top_tok_dev || !top_lp_dev || !S_dev || !next_tok_dev || !parent_dev || !anc_dev || !fed_dev || !fin_sum_dev ||
      !fin_len_dev || !fin_anc_dev || !fin_n_dev || !complete_dev || !state_dev)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 512 || K < 1 || K > kBeamMaxK || C < K || C > kBeamMaxCand || ctx < 2 || ctx > 448)
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  DecodeState s0;
  WA_HIP(hipMemcpy(&s0, state_dev, sizeof(s0), hipMemcpyDeviceToHost));
  if (s0.kv_len < 0 || s0.kv_len >= ctx) return fail(WQ4_EINVAL, "need 0 <= kv_len < ctx");
  std::vector<int32_t> fin_n(n_clips);
  WA_HIP(hipMemcpy(fin_n.data(), fin_n_dev, (size_t)n_clips * 4, hipMemcpyDeviceToHost));
  for (int n : fin_n)
    if (n < 0 || n > C) return fail(WQ4_EINVAL, "fin_n outside [0, C]");
  Dev d;
  auto* ticket = d.alloc<int>(1);
  if (!ticket) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(ticket, 0, sizeof(int)));
  const BeamSelect a{top_tok_dev, top_lp_dev,  S_dev,     next_tok_dev, parent_dev, anc_dev, fed_dev,
                     fin_sum_dev, fin_len_dev, fin_anc_dev, fin_n_dev,  complete_dev, ticket,
                     reinterpret_cast<DecodeState*>(state_dev)};
  WA_HIP(launch_beam_select(a, n_clips, K, C, ctx, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_beam_topk_rules_check(int device, const float* logits_dev, int n_rows, int V, int kp, int suppress_eot,
                                    int step, int eot_stop, int ts0, const int32_t* records, int32_t* tok_dev,
                                    float* lp_dev, int32_t* mass_dev, int32_t* flag_out) {
  if (!logits_dev || !tok_dev || !lp_dev || !records) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || V < 16 || kp < 2 || kp > kBeamMaxTop || ts0 <= 50257 || ts0 > V)
    return fail(WQ4_EINVAL, "bad sizes");
  return beam_topk_check(device, logits_dev, n_rows, V, kp, suppress_eot, step, eot_stop, ts0, records, nullptr, 0,
                         tok_dev, lp_dev, mass_dev, flag_out);
}

wq4_status wa_beam_select_rules_check(int device, const int32_t* top_tok_dev, const float* top_lp_dev, float* S_dev,
                                      int32_t* next_tok_dev, int32_t* parent_dev, int32_t* anc_dev, int32_t* fed_dev,
                                      float* fin_sum_dev, int32_t* fin_len_dev, int32_t* fin_anc_dev,
                                      int32_t* fin_n_dev, int32_t* complete_dev, int32_t* state_dev,
                                      int32_t* records_dev, int ts0, int V, int n_clips, int K, int C, int ctx) {
  if (!top_tok_dev || !top_lp_dev || !S_dev || !next_tok_dev || !parent_dev || !anc_dev || !fed_dev || !fin_sum_dev ||
      !fin_len_dev || !fin_anc_dev || !fin_n_dev || !complete_dev || !state_dev)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 512 || K < 1 || K > kBeamMaxK || C < K || C > kBeamMaxCand || ctx < 2 || ctx > 448 ||
      (records_dev && (ts0 < 1 || V < ts0)))
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  DecodeState s0;
  WA_HIP(hipMemcpy(&s0, state_dev, sizeof(s0), hipMemcpyDeviceToHost));
  if (s0.kv_len < 0 || s0.kv_len >= ctx) return fail(WQ4_EINVAL, "need 0 <= kv_len < ctx");
  std::vector<int32_t> fin_n(n_clips);
  WA_HIP(hipMemcpy(fin_n.data(), fin_n_dev, (size_t)n_clips * 4, hipMemcpyDeviceToHost));
  for (int n : fin_n)
    if (n < 0 || n > C) return fail(WQ4_EINVAL, "fin_n outside [0, C]");
  Dev d;
  auto* ticket = d.alloc<int>(1);
  if (!ticket) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(ticket, 0, sizeof(int)));
  const BeamSelect a{top_tok_dev, top_lp_dev,  S_dev,       next_tok_dev, parent_dev,   anc_dev, fed_dev,
                     fin_sum_dev, fin_len_dev, fin_anc_dev, fin_n_dev,    complete_dev, ticket,
                     reinterpret_cast<DecodeState*>(state_dev), reinterpret_cast<TsRule*>(records_dev)};
  WA_HIP(launch_beam_select(a, n_clips, K, C, ctx, nullptr, ts0, V));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_self_attention_beam_pad_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                            const int32_t* anc_dev, const int32_t* pad, int n_rows, int H, int ctx,
                                            int kv_len, wq4_precision prec, int f32_out, float* out_dev) {
  if (!qkv_dev || !cache_k_dev || !cache_v_dev || !anc_dev || !pad || !out_dev)
    return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || H < 1 || ctx < 1 || ctx > 448 || kv_len < 0 || kv_len + 1 > ctx)
    return fail(WQ4_EINVAL, "bad sizes");
  for (int r = 0; r < n_rows; ++r)
    if (pad[r] < 0 || pad[r] > kv_len) return fail(WQ4_EINVAL, "pad outside [0, kv_len]");
  WA_HIP(hipSetDevice(device));
  std::vector<int32_t> anc((size_t)n_rows * ctx);  // every entry read names a cache row
  WA_HIP(hipMemcpy(anc.data(), anc_dev, anc.size() * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < n_rows; ++r)
    for (int j = pad[r]; j < kv_len; ++j)
      if (anc[(size_t)r * ctx + j] < 0 || anc[(size_t)r * ctx + j] >= n_rows)
        return fail(WQ4_EINVAL, "ancestor row outside [0, n_rows)");
  Dev d;
  auto* pad_dev = d.alloc<int>(n_rows);
  if (!pad_dev) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(pad_dev, pad, (size_t)n_rows * 4, hipMemcpyHostToDevice));
  auto launch = [&](_Float16* tiled, float* out32) {
    return launch_decoder_self_attention_beam(qkv_dev, cache_k_dev, cache_v_dev, n_rows, H, ctx, nullptr, kv_len,
                                              anc_dev, tiled, planes(prec), nullptr, out32, pad_dev);
  };
  if (f32_out) {
    WA_HIP(launch(nullptr, out_dev));
    WA_HIP(hipDeviceSynchronize());
    return WQ4_OK;
  }
  return tiled_check(d, n_rows, 64 * H, prec, out_dev, [&](_Float16* tiled) { return launch(tiled, nullptr); });
}

wq4_status wa_conv_gelu_check(int device, const float* in_dev, int64_t in_bs, int64_t in_cs, int64_t in_ts, int B,
                              int C, int T_in, int stride, const float* w_dev, const float* bias_dev,
                              const float* pos_dev, int N, float* out_dev) {
  if (!in_dev || !w_dev || !bias_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (B < 1 || C < 1 || T_in < 1 || N < 1 || (stride != 1 && stride != 2)) return fail(WQ4_EINVAL, "bad sizes");
  if (C % 4 != 0) return fail(WQ4_EINVAL, "C must be a multiple of 4");
  if (in_bs < 0 || in_cs < 1 || in_ts < 1) return fail(WQ4_EINVAL, "bad strides");
  // channel-contiguous input: the kernel loads 4 channels as one 16-byte vector
  if (in_cs == 1 && (in_ts % 4 != 0 || in_bs % 4 != 0))
    return fail(WQ4_EINVAL, "a channel-contiguous input needs time and clip strides that are multiples of 4");
  const int T_out = (T_in - 1) / stride + 1;
  if ((int64_t)B * T_out > 2147483647LL - 128 || (int64_t)N * C > 2147483647LL / 3)
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  const size_t nw = (size_t)N * C * 3;
  std::vector<float> w(nw);
  WA_HIP(hipMemcpy(w.data(), w_dev, nw * 4, hipMemcpyDeviceToHost));
  const std::vector<float> wt = conv_weight_im2col(w.data(), N, C);
  auto* wt_dev = d.alloc<float>(nw);
  if (!wt_dev) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(wt_dev, wt.data(), nw * 4, hipMemcpyHostToDevice));
  WA_HIP(launch_conv_gelu(in_dev, (long)in_bs, (long)in_cs, (long)in_ts, B, C, T_in, stride, wt_dev, bias_dev, pos_dev,
                          N, out_dev, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_embed_check(int device, const int32_t* tokens, const float* tok_emb_dev, int V,
                          const float* pos_emb_dev, int ctx, int B, int Tq, int D, int pos0, int use_state,
                          const float* gamma_dev, wq4_precision prec, float* x_dev, void* tiled_dev,
                          float* stats_dev) {
  if (!tokens || !tok_emb_dev || !pos_emb_dev || !x_dev) return fail(WQ4_EINVAL, "null argument");
  if (gamma_dev && (!tiled_dev || !stats_dev)) return fail(WQ4_EINVAL, "gamma needs the operand and statistics outputs");
  if (B < 1 || Tq < 1 || D < 1 || V < 1 || ctx < 1 || (int64_t)B * Tq > 2147483647LL)
    return fail(WQ4_EINVAL, "bad sizes");
  if (gamma_dev && D % 32 != 0) return fail(WQ4_EINVAL, "the folded form needs D % 32 == 0");
  if (pos0 < 0 || (int64_t)pos0 + Tq > ctx) return fail(WQ4_EINVAL, "need 0 <= pos0 and pos0 + Tq <= ctx");
  const int R = B * Tq;
  for (int i = 0; i < R; ++i)
    if (tokens[i] < 0 || tokens[i] >= V) return fail(WQ4_EINVAL, "token id outside [0, V)");
  WA_HIP(hipSetDevice(device));
  Dev d;
  auto* tok = d.alloc<int>(R);
  if (!tok) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(tok, tokens, (size_t)R * 4, hipMemcpyHostToDevice));
  // through the device state the host position is a value no row may use
  DecodeState* st = nullptr;
  if (use_state) {
    st = d.alloc<DecodeState>(1);
    if (!st) return fail(WQ4_ENOMEM, "allocation failed");
    const DecodeState s0{pos0, 0, 0, 0};
    WA_HIP(hipMemcpy(st, &s0, sizeof(s0), hipMemcpyHostToDevice));
  }
  const int pos0_host = use_state ? -1 : pos0;
  if (gamma_dev)
    WA_HIP(launch_embed_fold(tok, tok_emb_dev, pos_emb_dev, B, Tq, D, st, pos0_host, x_dev, gamma_dev,
                             static_cast<_Float16*>(tiled_dev), stats_dev, planes(prec), nullptr));
  else
    WA_HIP(launch_embed(tok, tok_emb_dev, pos_emb_dev, B, Tq, D, st, pos0_host, x_dev, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// The fused pick on caller data, in the mode the arguments select (PickArgs):
// wa_logits_argmax_check; with logprob_dev the scored launch of
// wa_logits_logprob_check; with rules_host (n_clips records) the timestamp
// launch of wa_logits_timestamp_check; with temperature / seed (host, n_clips
// each) the sampled launch of wa_logits_sample_check; with sup_ids any of them
// under that list (wa_logits_suppress_check).
static wq4_status logits_pick_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                    int step, wq4_precision prec, int32_t* tok_dev, float* logprob_dev,
                                    float* logits_dev, const TsRule* rules_host = nullptr, int ts0 = 0,
                                    int32_t* mass_dev = nullptr, const float* temperature = nullptr,
                                    const uint64_t* seed = nullptr, const int32_t* sup_ids = nullptr,
                                    int n_sup = 0) {
  const int ns = planes(prec);
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, sup_ids, n_sup, V, ts0 > 0 ? std::min(ts0, V) : V, &sup));
  auto* emb2 = d.alloc<_Float16>((size_t)emb_tiled_rows(V) * ns * D);
  auto* st = d.alloc<DecodeState>(1);
  const size_t tb = wq4_atiled_bytes(n_clips, D, prec);
  auto* ht = d.alloc<_Float16>(tb / 2);
  PickArgs p{};
  p.scratch = d.alloc<float>((size_t)logits_pick_scratch_floats(V));
  p.counter = d.alloc<int>(1);
  p.out_tok = tok_dev;
  p.out_lp = logprob_dev;
  p.out_mass = mass_dev;
  p.ts0 = ts0;
  p.sup = sup;
  if (!emb2 || !st || !ht || !p.scratch || !p.counter) return fail(WQ4_ENOMEM, "allocation failed");
  if (rules_host) {
    auto* rules = d.alloc<TsRule>(n_clips);
    if (!rules) return fail(WQ4_ENOMEM, "allocation failed");
    WA_HIP(hipMemcpy(rules, rules_host, (size_t)n_clips * sizeof(TsRule), hipMemcpyHostToDevice));
    p.rules = rules;
  }
  if (temperature) {
    auto* temp = d.alloc<float>(n_clips);
    auto* sd = d.alloc<uint64_t>(n_clips);
    if (!temp || !sd) return fail(WQ4_ENOMEM, "allocation failed");
    WA_HIP(hipMemcpy(temp, temperature, (size_t)n_clips * 4, hipMemcpyHostToDevice));
    WA_HIP(hipMemcpy(sd, seed, (size_t)n_clips * 8, hipMemcpyHostToDevice));
    p.temp = temp;
    p.seed = sd;
  }
  WA_HIP(launch_emb_tiled(emb_dev, V, D, ns, emb2, nullptr));
  WA_WQ4(wq4_tile_activations(hid_dev, n_clips, D, D, prec, ht, tb, nullptr));
  // A trace writes slot state->step + 1 of [clip][state->step + 2][V] (every
  // id listed at that slot).  A sampled pick keeps the caller's step in the
  // state (its pick index is step + 1); the others trace with step 0, and the
  // EOT suppression of `step` (step + 1 < 3, whisper.rs:120-122) is passed
  // through min_tokens instead.
  const bool fold = logits_dev && !temperature;
  const DecodeState s0{0, 0, fold ? 0 : step, 0};
  const int min_tokens = !fold ? kMinTokens : (step + 1 < kMinTokens ? 1 << 30 : 0);
  WA_HIP(hipMemcpy(st, &s0, sizeof(s0), hipMemcpyHostToDevice));
  WA_HIP(hipMemset(p.counter, 0, sizeof(int)));
  const int s1 = s0.step + 2;
  int* ids = nullptr;
  float* tr = nullptr;
  if (logits_dev) {
    ids = d.alloc<int>((size_t)n_clips * s1 * V);
    tr = d.alloc<float>((size_t)n_clips * s1 * V);
    if (!ids || !tr) return fail(WQ4_ENOMEM, "allocation failed");
    std::vector<int> h((size_t)n_clips * s1 * V, 0);
    for (int b = 0; b < n_clips; ++b)
      for (int v = 0; v < V; ++v) h[((size_t)b * s1 + s1 - 1) * V + v] = v;
    WA_HIP(hipMemcpy(ids, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  }
  WA_HIP(launch_logits_pick(ht, n_clips, D, emb2, ns, V, min_tokens, st, p, ids, tr, s1, V, nullptr, nullptr));
  if (logits_dev)
    for (int b = 0; b < n_clips; ++b)
      WA_HIP(hipMemcpy(logits_dev + (size_t)b * V, tr + ((size_t)b * s1 + s1 - 1) * V, (size_t)V * 4,
                       hipMemcpyDeviceToDevice));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_logits_argmax_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                  int step, wq4_precision prec, int32_t* tok_dev, float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 32 || V < 1 || !emb_tiled_supported(D)) return fail(WQ4_EINVAL, "bad sizes");
  return logits_pick_check(device, hid_dev, emb_dev, n_clips, D, V, step, prec, tok_dev, nullptr, logits_dev);
}

wq4_status wa_logits_logprob_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                   int step, wq4_precision prec, int32_t* tok_dev, float* logprob_dev,
                                   float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev || !logprob_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 32 || V < 1 || !emb_tiled_supported(D)) return fail(WQ4_EINVAL, "bad sizes");
  return logits_pick_check(device, hid_dev, emb_dev, n_clips, D, V, step, prec, tok_dev, logprob_dev, logits_dev);
}

wq4_status wa_row_logprob_check(int device, const float* logits_dev, int n_rows, int V, int lo, int hi, int mask_eot,
                                const int32_t* idx_dev, int fixed_idx, float* logprob_dev) {
  if (!logits_dev || !logprob_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || n_rows > 32 || V < 1 || lo < 0 || hi > V || lo >= hi) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  WA_HIP(launch_row_logprob(logits_dev, n_rows, V, lo, hi, mask_eot, 0, nullptr, idx_dev, 1, fixed_idx, logprob_dev, 1,
                            nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// ---- timestamp rules: the product kernels on caller data -----------------
static_assert(sizeof(TsRule) == 8 * sizeof(int32_t), "a rule record is 8 int32 at the ABI");

wq4_status wa_timestamp_rule(const int32_t* tokens, int n, int ts0, int V, int max_initial, int32_t* record_out) {
  if (!record_out || n < 0 || (n > 0 && !tokens) || ts0 < 1 || V < ts0) return fail(WQ4_EINVAL, "bad arguments");
  TsRule r = ts_rule_first(ts0, V, max_initial);
  for (int i = 0; i < n; ++i) r = ts_rule_next(r, tokens[i], ts0, V);
  std::memcpy(record_out, &r, sizeof(r));
  return WQ4_OK;
}

wq4_status wa_logits_timestamp_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                     int step, wq4_precision prec, int ts0, const int32_t* records, int32_t* tok_dev,
                                     float* logprob_dev, int32_t* mass_dev, float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev || !logprob_dev || !records) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 32 || V < 1 || ts0 < 1 || !emb_tiled_supported(D)) return fail(WQ4_EINVAL, "bad sizes");
  return logits_pick_check(device, hid_dev, emb_dev, n_clips, D, V, step, prec, tok_dev, logprob_dev, logits_dev,
                           reinterpret_cast<const TsRule*>(records), ts0, mass_dev);
}

wq4_status wa_row_timestamp_check(int device, const float* logits_dev, int n_rows, int V, int suppress_eot, int ts0,
                                  const int32_t* records, int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev) {
  if (!logits_dev || !records || !tok_dev || !logprob_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || n_rows > 32 || V < 1 || ts0 < 1) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  auto* rules = d.alloc<TsRule>(n_rows);
  if (!rules) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(rules, records, (size_t)n_rows * sizeof(TsRule), hipMemcpyHostToDevice));
  WA_HIP(launch_row_pick(logits_dev, n_rows, V, V, suppress_eot, 0, nullptr, rules, ts0, nullptr, nullptr, 0, tok_dev,
                         logprob_dev, mass_dev, nullptr, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_timestamp_bookkeep_check(int device, const int32_t* tokens, int n_rows, int n_steps, int ts0, int V,
                                       int max_initial, int32_t* records_out) {
  if (!tokens || !records_out) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || n_rows > 256 || n_steps < 1 || n_steps > kMaxTokens || ts0 < 1 || V < ts0)
    return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  const size_t B = (size_t)n_rows;
  auto* rules = d.alloc<TsRule>(B);
  auto* next = d.alloc<int>(B);
  auto* lp = d.alloc<float>(B);
  auto* toks = d.alloc<int>(B * kMaxTokens);
  auto* logprob = d.alloc<float>(B * (kMaxTokens + 1));
  auto* ntok = d.alloc<int>(B);
  auto* done = d.alloc<int>(B);
  auto* st = d.alloc<DecodeState>(1);
  if (!rules || !next || !lp || !toks || !logprob || !ntok || !done || !st) return fail(WQ4_ENOMEM, "allocation failed");
  const std::vector<TsRule> first(B, ts_rule_first(ts0, V, max_initial));
  WA_HIP(hipMemcpy(rules, first.data(), B * sizeof(TsRule), hipMemcpyHostToDevice));
  WA_HIP(hipMemset(lp, 0, B * 4));
  WA_HIP(hipMemset(ntok, 0, B * 4));
  WA_HIP(hipMemset(done, 0, B * 4));
  WA_HIP(hipMemset(st, 0, sizeof(DecodeState)));
  std::vector<int> col(B);
  for (int s = 0; s < n_steps; ++s) {  // one token per row and launch, as a decode step feeds them
    for (size_t b = 0; b < B; ++b) col[b] = tokens[b * n_steps + s];
    WA_HIP(hipMemcpy(next, col.data(), B * 4, hipMemcpyHostToDevice));
    WA_HIP(launch_bookkeep(next, lp, toks, logprob, ntok, done, n_rows, kMaxTokens, 0, st, rules, ts0, V, nullptr));
    WA_HIP(hipMemcpy(records_out + (size_t)s * B * 8, rules, B * sizeof(TsRule), hipMemcpyDeviceToHost));
  }
  return WQ4_OK;
}

// ---- temperature sampling: the product kernels on caller data -------------
wq4_status wa_logits_sample_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                  int step, wq4_precision prec, const float* temperature, const uint64_t* seed,
                                  int ts0, const int32_t* records, int32_t* tok_dev, float* logprob_dev,
                                  int32_t* mass_dev, float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev || !logprob_dev || !temperature || !seed)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 32 || V < 1 || step < 0 || step > 16 || (records && ts0 < 1) ||
      !emb_tiled_supported(D))
    return fail(WQ4_EINVAL, "bad sizes");
  for (int b = 0; b < n_clips; ++b)
    if (!(temperature[b] >= 0.0f) || !std::isfinite(temperature[b]))
      return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  return logits_pick_check(device, hid_dev, emb_dev, n_clips, D, V, step, prec, tok_dev, logprob_dev, logits_dev,
                           reinterpret_cast<const TsRule*>(records), ts0, mass_dev, temperature, seed);
}

wq4_status wa_row_sample_check(int device, const float* logits_dev, int n_rows, int V, int suppress_eot, int pick,
                               const float* temperature, const uint64_t* seed, int ts0, const int32_t* records,
                               int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev) {
  if (!logits_dev || !tok_dev || !logprob_dev || !temperature || !seed) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || n_rows > 32 || V < 1 || pick < 0 || (records && ts0 < 1)) return fail(WQ4_EINVAL, "bad sizes");
  for (int b = 0; b < n_rows; ++b)
    if (!(temperature[b] >= 0.0f) || !std::isfinite(temperature[b]))
      return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  WA_HIP(hipSetDevice(device));
  Dev d;
  auto* temp = d.alloc<float>(n_rows);
  auto* sd = d.alloc<uint64_t>(n_rows);
  TsRule* rules = records ? d.alloc<TsRule>(n_rows) : nullptr;
  if (!temp || !sd || (records && !rules)) return fail(WQ4_ENOMEM, "allocation failed");
  if (records) WA_HIP(hipMemcpy(rules, records, (size_t)n_rows * sizeof(TsRule), hipMemcpyHostToDevice));
  WA_HIP(hipMemcpy(temp, temperature, (size_t)n_rows * 4, hipMemcpyHostToDevice));
  WA_HIP(hipMemcpy(sd, seed, (size_t)n_rows * 8, hipMemcpyHostToDevice));
  WA_HIP(launch_row_pick(logits_dev, n_rows, V, V, suppress_eot, 0, nullptr, rules, ts0, temp, sd, pick, tok_dev,
                         logprob_dev, mass_dev, nullptr, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// ---- suppress-token lists: the rule on the host, the kernels on caller data --
wq4_status wa_suppress_check(const int32_t* always, int n_always, const int32_t* first, int n_first, int ts0) {
  constexpr int kEot = 50257, kMinText = 16;
  if (n_always < 0 || n_first < 0 || (n_always > 0 && !always) || (n_first > 0 && !first))
    return fail(WQ4_EINVAL, "bad suppress lists");
  if (ts0 <= kEot) return fail(WQ4_EINVAL, "ts0 must lie above EOT");
  std::vector<bool> listed(kEot, false);
  for (int i = 0; i < n_always; ++i) {
    if (always[i] < 0 || always[i] >= ts0 || always[i] == kEot)
      return fail(WQ4_EINVAL, "an `always` id lies outside [0, EOT) and (EOT, ts0)");
    if (always[i] < kEot) listed[always[i]] = true;
  }
  for (int i = 0; i < n_first; ++i) {
    if (first[i] < 0 || first[i] >= ts0) return fail(WQ4_EINVAL, "a `first` id lies outside [0, ts0)");
    if (first[i] < kEot) listed[first[i]] = true;
  }
  int left = 0;
  for (int v = 0; v < kEot; ++v) left += listed[v] ? 0 : 1;
  if (left < kMinText) return fail(WQ4_EINVAL, "the lists leave fewer than 16 text ids");
  return WQ4_OK;
}

wq4_status wa_logits_suppress_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                    int step, wq4_precision prec, const int32_t* ids, int n_ids,
                                    const float* temperature, const uint64_t* seed, int ts0, const int32_t* records,
                                    int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev, float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev || !temperature != !seed) return fail(WQ4_EINVAL, "null argument");
  if ((records || temperature) && !logprob_dev) return fail(WQ4_EINVAL, "this mode needs logprob_dev");
  if (n_clips < 1 || n_clips > 32 || V < 1 || ts0 < 1 || ts0 > V || !emb_tiled_supported(D) ||
      (temperature && (step < 0 || step > 16)))
    return fail(WQ4_EINVAL, "bad sizes");
  if (temperature)
    for (int b = 0; b < n_clips; ++b)
      if (!(temperature[b] >= 0.0f) || !std::isfinite(temperature[b]))
        return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  return logits_pick_check(device, hid_dev, emb_dev, n_clips, D, V, step, prec, tok_dev, logprob_dev, logits_dev,
                           reinterpret_cast<const TsRule*>(records), ts0, mass_dev, temperature, seed, ids, n_ids);
}

wq4_status wa_row_suppress_check(int device, const float* logits_dev, int n_rows, int V, int suppress_eot, int pick,
                                 const int32_t* ids, int n_ids, const float* temperature, const uint64_t* seed,
                                 int ts0, const int32_t* records, int32_t* tok_dev, float* logprob_dev,
                                 int32_t* mass_dev) {
  if (!logits_dev || !tok_dev || !temperature != !seed) return fail(WQ4_EINVAL, "null argument");
  if ((records || temperature) && !logprob_dev) return fail(WQ4_EINVAL, "this mode needs logprob_dev");
  if (n_rows < 1 || n_rows > 32 || V < 1 || pick < 0 || ts0 < 1 || ts0 > V) return fail(WQ4_EINVAL, "bad sizes");
  if (temperature)
    for (int b = 0; b < n_rows; ++b)
      if (!(temperature[b] >= 0.0f) || !std::isfinite(temperature[b]))
        return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, ids, n_ids, V, ts0, &sup));
  if (!temperature && !records) {  // the plain / scored pick of a stored row
    WA_HIP(launch_argmax(logits_dev, n_rows, V, 0, V, suppress_eot, tok_dev, 1, nullptr, nullptr, sup));
    if (logprob_dev)
      WA_HIP(launch_row_logprob(logits_dev, n_rows, V, 0, V, suppress_eot, 0, nullptr, tok_dev, 1, 0, logprob_dev, 1,
                                nullptr, sup));
    WA_HIP(hipDeviceSynchronize());
    return WQ4_OK;
  }
  float* temp = nullptr;
  uint64_t* sd = nullptr;
  if (temperature) {
    temp = d.alloc<float>(n_rows);
    sd = d.alloc<uint64_t>(n_rows);
    if (!temp || !sd) return fail(WQ4_ENOMEM, "allocation failed");
    WA_HIP(hipMemcpy(temp, temperature, (size_t)n_rows * 4, hipMemcpyHostToDevice));
    WA_HIP(hipMemcpy(sd, seed, (size_t)n_rows * 8, hipMemcpyHostToDevice));
  }
  TsRule* rules = records ? d.alloc<TsRule>(n_rows) : nullptr;
  if (records && !rules) return fail(WQ4_ENOMEM, "allocation failed");
  if (records) WA_HIP(hipMemcpy(rules, records, (size_t)n_rows * sizeof(TsRule), hipMemcpyHostToDevice));
  WA_HIP(launch_row_pick(logits_dev, n_rows, V, V, suppress_eot, 0, nullptr, rules, ts0, temp, sd, pick, tok_dev,
                         logprob_dev, mass_dev, nullptr, nullptr, sup));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- log-mel --
// Per-device constants (window, filterbank, twiddles; per n_mels) and the
// per-workgroup-max scratch, allocated on first use outside stream capture.
namespace {
struct MelDevice {
  std::map<int, uint8_t*> consts;
  float* part = nullptr;
  int part_clips = 0;
  // windows of long recordings: the recordings' table and per-workgroup maxima
  // of wa_long_mel_max, the clips' descriptors of wa_long_mel_windows; the
  // tables are staged in pinned memory and uploaded on the launch stream
  // (*_uploaded: the table's last upload, awaited before its staging is rewritten)
  MelStream* streams = nullptr;
  MelStream* streams_host = nullptr;
  int streams_cap = 0;
  float* long_part = nullptr;
  int64_t long_part_cap = 0;
  MelWindow* wins = nullptr;
  MelWindow* wins_host = nullptr;
  int wins_cap = 0;
  hipEvent_t streams_uploaded = nullptr, wins_uploaded = nullptr;
};
std::mutex g_mel_mu;
std::map<int, MelDevice> g_mel;

wq4_status not_capturing(hipStream_t st, const char* who) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  WA_HIP(hipStreamIsCapturing(st, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return fail(WQ4_EINVAL, std::string(who) + ": run once outside stream capture first (allocates)");
  return WQ4_OK;
}

// The (device, n_mels) constants, created on first use.
wq4_status mel_consts(MelDevice& md, int n_mels, hipStream_t st, const char* who, uint8_t** out) {
  uint8_t*& c = md.consts[n_mels];
  if (!c) {
    WA_TRY(not_capturing(st, who));
    const MelBank bank = make_mel_bank(n_mels);
    std::vector<uint8_t> host(mel_const_bytes(n_mels));
    mel_pack_consts(bank, host.data());
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&c), host.size()));
    WA_HIP(hipMemcpy(c, host.data(), host.size(), hipMemcpyHostToDevice));
  }
  *out = c;
  return WQ4_OK;
}

// A device array and its pinned staging of at least `need` entries.
template <class T>
wq4_status grow_table(T*& dev, T*& host, int& cap, int need, hipStream_t st, const char* who) {
  if (cap >= need) return WQ4_OK;
  WA_TRY(not_capturing(st, who));
  WA_HIP(hipDeviceSynchronize());
  if (dev) WA_HIP(hipFree(dev));
  if (host) WA_HIP(hipHostFree(host));
  dev = host = nullptr;
  cap = 0;
  WA_HIP(hipMalloc(reinterpret_cast<void**>(&dev), (size_t)need * sizeof(T)));
  WA_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), (size_t)need * sizeof(T), 0));
  cap = need;
  return WQ4_OK;
}

// The staging may be rewritten once the last upload from it has run.
wq4_status staging_free(hipEvent_t& uploaded) {
  if (!uploaded) WA_HIP(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
  WA_HIP(hipEventSynchronize(uploaded));
  return WQ4_OK;
}
}  // namespace

extern "C" {

wq4_status wa_log_mel(int device, const float* audio_dev, int n_clips, int64_t n_samples, int64_t ld_audio,
                      int n_mels, float* mel_dev, void* stream) {
  if (!mel_dev || (!audio_dev && n_samples > 0)) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1) return fail(WQ4_EINVAL, "n_clips must be >= 1");
  if (n_samples < 0 || ld_audio < n_samples) return fail(WQ4_EINVAL, "need 0 <= n_samples <= ld_audio");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_log_mel", &c));
  if (md.part_clips < n_clips) {
    WA_TRY(not_capturing(st, "wa_log_mel"));
    WA_HIP(hipDeviceSynchronize());
    if (md.part) WA_HIP(hipFree(md.part));
    md.part = nullptr;
    md.part_clips = 0;
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&md.part), (size_t)n_clips * kMelWgPerClip * sizeof(float)));
    md.part_clips = n_clips;
  }
  WA_HIP(launch_log_mel(audio_dev, n_clips, n_samples, ld_audio, n_mels, c, md.part, mel_dev, st));
  return WQ4_OK;
}

wq4_status wa_long_mel_max(int device, const float* audio_dev, int n_streams, const int64_t* offset,
                           const int64_t* n_samples, int n_mels, float* max_dev, void* stream) {
  if (!audio_dev || !offset || !n_samples || !max_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_streams < 1) return fail(WQ4_EINVAL, "n_streams must be >= 1");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  int64_t n_wg = 0;
  for (int r = 0; r < n_streams; ++r) {
    if (offset[r] < 0 || n_samples[r] < 0 || n_samples[r] >= kMelLongMaxSamples)
      return fail(WQ4_EINVAL, "need offset >= 0 and 0 <= n_samples < 160 * (2^31 - 3001)");
    n_wg += (mel_stream_frames(n_samples[r]) + kMelFramesPerWg - 1) / kMelFramesPerWg;
  }
  if (n_wg > 2147483647LL) return fail(WQ4_EINVAL, "more than 2^31 - 1 workgroups of frames in one call");
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_long_mel_max", &c));
  WA_TRY(grow_table(md.streams, md.streams_host, md.streams_cap, n_streams, st, "wa_long_mel_max"));
  if (md.long_part_cap < n_wg) {
    WA_TRY(not_capturing(st, "wa_long_mel_max"));
    WA_HIP(hipDeviceSynchronize());
    if (md.long_part) WA_HIP(hipFree(md.long_part));
    md.long_part = nullptr;
    md.long_part_cap = 0;
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&md.long_part), (size_t)n_wg * sizeof(float)));
    md.long_part_cap = n_wg;
  }
  WA_TRY(staging_free(md.streams_uploaded));
  int64_t wg = 0;
  for (int r = 0; r < n_streams; ++r) {
    const int64_t frames = mel_stream_frames(n_samples[r]);
    md.streams_host[r] = MelStream{offset[r], n_samples[r], frames, wg};
    wg += (frames + kMelFramesPerWg - 1) / kMelFramesPerWg;
  }
  WA_HIP(hipMemcpyAsync(md.streams, md.streams_host, (size_t)n_streams * sizeof(MelStream), hipMemcpyHostToDevice, st));
  WA_HIP(hipEventRecord(md.streams_uploaded, st));
  WA_HIP(launch_long_mel_max(audio_dev, md.streams, n_streams, n_wg, n_mels, c, md.long_part, max_dev, st));
  return WQ4_OK;
}

wq4_status wa_long_mel_windows(int device, const float* audio_dev, int n_clips, const int64_t* offset,
                               const int64_t* n_samples, const int32_t* seek, const int32_t* max_index,
                               const float* max_dev, int n_mels, float* mel_dev, void* stream) {
  if (!audio_dev || !offset || !n_samples || !seek || !max_index || !max_dev || !mel_dev)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 65535) return fail(WQ4_EINVAL, "n_clips must be in [1, 65535]");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  for (int c = 0; c < n_clips; ++c) {
    if (offset[c] < 0 || n_samples[c] < 0 || n_samples[c] >= kMelLongMaxSamples)
      return fail(WQ4_EINVAL, "need offset >= 0 and 0 <= n_samples < 160 * (2^31 - 3001)");
    if (seek[c] < 0 || seek[c] >= n_samples[c] / kMelHop)
      return fail(WQ4_EINVAL, "need 0 <= seek < n_samples / 160");
    if (max_index[c] < 0) return fail(WQ4_EINVAL, "max_index must be >= 0");
  }
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_long_mel_windows", &c));
  WA_TRY(grow_table(md.wins, md.wins_host, md.wins_cap, n_clips, st, "wa_long_mel_windows"));
  WA_TRY(staging_free(md.wins_uploaded));
  for (int i = 0; i < n_clips; ++i) md.wins_host[i] = MelWindow{offset[i], n_samples[i], seek[i], max_index[i]};
  WA_HIP(hipMemcpyAsync(md.wins, md.wins_host, (size_t)n_clips * sizeof(MelWindow), hipMemcpyHostToDevice, st));
  WA_HIP(hipEventRecord(md.wins_uploaded, st));
  WA_HIP(launch_long_mel_windows(audio_dev, md.wins, n_clips, max_dev, n_mels, c, mel_dev, st));
  return WQ4_OK;
}

wq4_status wa_mel_filterbank(int n_mels, float* filters_out, float* window_out) {
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  const MelBank bank = make_mel_bank(n_mels);
  if (filters_out) std::memcpy(filters_out, bank.filters.data(), bank.filters.size() * sizeof(float));
  if (window_out) std::memcpy(window_out, bank.window.data(), bank.window.size() * sizeof(float));
  return WQ4_OK;
}

}  // extern "C"
