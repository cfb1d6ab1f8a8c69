// wa_checks.cpp -- the kernel check entries (include/whisper_amd_checks.h):
// each runs one product kernel, in the mode its arguments select, on
// caller-supplied buffers for the parity tests; and the host-only probes of the
// rules behind a decode's layout.  Every entry checks what it can see on the
// host before it touches the device.
#include <set>

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

// n host values on the device; a null array stays null
template <class T>
wq4_status to_device(Dev& d, const T* host, size_t n, T** out) {
  *out = nullptr;
  if (!host) return WQ4_OK;
  T* p = d.alloc<T>(n);
  if (!p) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return WQ4_OK;
}

// a host pad array (nullable), each in [0, hi]
bool pad_ok(const int32_t* pad, int n, int hi) {
  for (int i = 0; pad && i < n; ++i)
    if (pad[i] < 0 || pad[i] > hi) return false;
  return true;
}
wq4_status pad_to_device(Dev& d, const int32_t* pad, int n, int** out) { return to_device<int>(d, pad, (size_t)n, out); }

// host rule records [n][8] (nullable) on the device
static_assert(sizeof(TsRule) == 8 * sizeof(int32_t), "a rule record is 8 int32 at the ABI");
static_assert(sizeof(DecodeState) == 4 * sizeof(int32_t), "the decode state is 4 int32 at the ABI");
wq4_status records_to_device(Dev& d, const int32_t* records, int n, TsRule** out) {
  return to_device(d, reinterpret_cast<const TsRule*>(records), (size_t)n, out);
}

// The id list of a pick entry: ids in [0, ts0) -- the whole row where the entry
// runs without a ts0 -- and its device mask, null for an empty list.
int sup_bound(int ts0, int V) { return ts0 > 0 ? std::min(ts0, V) : V; }
bool sup_ok(const int32_t* ids, int n_ids, int bound) {
  if (n_ids < 0 || (n_ids > 0 && !ids)) return false;
  for (int i = 0; i < n_ids; ++i)
    if (ids[i] < 0 || ids[i] >= bound) return false;
  return true;
}
wq4_status sup_upload(Dev& d, const int32_t* ids, int n_ids, int V, const uint32_t** out) {
  *out = nullptr;
  if (n_ids == 0) return WQ4_OK;
  std::vector<uint32_t> words((size_t)sup_mask_words(V));
  sup_mask_build(ids, n_ids, V, words.data());
  uint32_t* dev = nullptr;
  WA_TRY(to_device(d, words.data(), words.size(), &dev));
  *out = dev;
  return WQ4_OK;
}

// What the pick entries share: ts0 in [0, V] (records need one), the list,
// temperature and seed together and then with a log-probability output.
wq4_status pick_args_ok(int n_rows, int V, int ts0, const int32_t* records, const int32_t* ids, int n_ids,
                        const float* temperature, const uint64_t* seed, const float* logprob_dev) {
  if (!temperature != !seed) return fail(WQ4_EINVAL, "null argument");
  if ((records || temperature) && !logprob_dev) return fail(WQ4_EINVAL, "this mode needs logprob_dev");
  if (n_rows < 1 || n_rows > 32 || V < 1 || ts0 < 0 || ts0 > V || (records && ts0 < 1))
    return fail(WQ4_EINVAL, "bad sizes");
  if (!sup_ok(ids, n_ids, sup_bound(ts0, V))) return fail(WQ4_EINVAL, "suppressed id outside [0, ts0)");
  if (temperature && bad_temperatures(temperature, n_rows))
    return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  return WQ4_OK;
}

}  // namespace

extern "C" {

// ---- attention -------------------------------------------------------------
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
                                   const int32_t* anc_dev, const int32_t* pad, int n_rows, int Tq, int H, int ctx,
                                   int kv_len, wq4_precision prec, int f32_out, float* out_dev) {
  if (!qkv_dev || !cache_k_dev || !cache_v_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || Tq < 1 || Tq > 4 || H < 1 || ctx < 1 || ctx > 448 || kv_len < 0 || kv_len + Tq > ctx)
    return fail(WQ4_EINVAL, "bad sizes");
  if (anc_dev && Tq != 1) return fail(WQ4_EINVAL, "the reindexed form has Tq = 1");
  if (!pad_ok(pad, n_rows, kv_len)) return fail(WQ4_EINVAL, "pad outside [0, kv_len]");
  WA_HIP(hipSetDevice(device));
  if (anc_dev) {  // every entry read names a cache row
    std::vector<int32_t> anc((size_t)n_rows * ctx);
    WA_HIP(hipMemcpy(anc.data(), anc_dev, anc.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_rows; ++r)
      for (int j = pad ? pad[r] : 0; j < kv_len; ++j)
        if (anc[(size_t)r * ctx + j] < 0 || anc[(size_t)r * ctx + j] >= n_rows)
          return fail(WQ4_EINVAL, "ancestor row outside [0, n_rows)");
  }
  Dev d;
  int* pad_dev = nullptr;
  WA_TRY(pad_to_device(d, pad, n_rows, &pad_dev));
  auto launch = [&](_Float16* tiled, float* out32) {
    return anc_dev ? launch_decoder_self_attention_beam(qkv_dev, cache_k_dev, cache_v_dev, n_rows, H, ctx, nullptr,
                                                        kv_len, anc_dev, tiled, planes(prec), nullptr, out32, pad_dev)
                   : launch_decoder_self_attention(qkv_dev, cache_k_dev, cache_v_dev, n_rows, Tq, H, ctx, nullptr,
                                                   kv_len, tiled, planes(prec), nullptr, out32, pad_dev);
  };
  if (f32_out) {
    WA_HIP(launch(nullptr, out_dev));
    WA_HIP(hipDeviceSynchronize());
    return WQ4_OK;
  }
  return tiled_check(d, n_rows * Tq, 64 * H, prec, out_dev, [&](_Float16* tiled) { return launch(tiled, nullptr); });
}

wq4_status wa_self_attention_prefill_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                           int n_clips, int P, const int32_t* pad, int H, int ctx,
                                           wq4_precision prec, float* out_dev) {
  if (!qkv_dev || !cache_k_dev || !cache_v_dev || !pad || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || P < 1 || H < 1 || ctx < 1 || ctx > 448 || P > ctx) return fail(WQ4_EINVAL, "bad sizes");
  if (!pad_ok(pad, n_clips, P - 1)) return fail(WQ4_EINVAL, "pad out of range");
  WA_HIP(hipSetDevice(device));
  Dev d;
  int* pad_dev = nullptr;
  WA_TRY(pad_to_device(d, pad, n_clips, &pad_dev));
  return tiled_check(d, (int64_t)n_clips * P, 64 * H, prec, out_dev, [&](_Float16* tiled) {
    return launch_prefill_self_attention(qkv_dev, cache_k_dev, cache_v_dev, n_clips, P, H, ctx, pad_dev, tiled,
                                         planes(prec), nullptr);
  });
}

wq4_status wa_cross_attention_prefill_check(int device, const float* q_dev, const float* k_dev, const float* v_dev,
                                            int n_clips, int P, int T, int H, wq4_precision prec, float* out_dev) {
  if (!q_dev || !k_dev || !v_dev || !out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || P < 1 || T < 1 || H < 1) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  return tiled_check(d, (int64_t)n_clips * P, 64 * H, prec, out_dev, [&](_Float16* tiled) {
    return launch_prefill_cross_attention(q_dev, k_dev, v_dev, n_clips, P, T, H, tiled, planes(prec), nullptr);
  });
}

// ---- conv stem and embedding -----------------------------------------------
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
  float* wt_dev = nullptr;
  WA_TRY(to_device(d, wt.data(), nw, &wt_dev));
  WA_HIP(launch_conv_gelu(in_dev, (long)in_bs, (long)in_cs, (long)in_ts, B, C, T_in, stride, wt_dev, bias_dev, pos_dev,
                          N, out_dev, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_embed_check(int device, const int32_t* tokens, const float* tok_emb_dev, int V,
                          const float* pos_emb_dev, int ctx, int B, int Tq, int D, int pos0, int use_state,
                          const int32_t* pad, const float* gamma_dev, wq4_precision prec, float* x_dev,
                          void* tiled_dev, float* stats_dev) {
  if (!tokens || !tok_emb_dev || !pos_emb_dev || !x_dev) return fail(WQ4_EINVAL, "null argument");
  if (gamma_dev && (!tiled_dev || !stats_dev)) return fail(WQ4_EINVAL, "gamma needs the operand and statistics outputs");
  if (B < 1 || Tq < 1 || D < 1 || V < 1 || ctx < 1 || (int64_t)B * Tq > 2147483647LL)
    return fail(WQ4_EINVAL, "bad sizes");
  if (gamma_dev && D % 32 != 0) return fail(WQ4_EINVAL, "the folded form needs D % 32 == 0");
  if (pos0 < 0 || (int64_t)pos0 + Tq > ctx) return fail(WQ4_EINVAL, "need 0 <= pos0 and pos0 + Tq <= ctx");
  const int R = B * Tq;
  for (int i = 0; i < R; ++i)
    if (tokens[i] < 0 || tokens[i] >= V) return fail(WQ4_EINVAL, "token id outside [0, V)");
  if (!pad_ok(pad, B, pos0)) return fail(WQ4_EINVAL, "pad out of range");
  WA_HIP(hipSetDevice(device));
  Dev d;
  int *pad_dev = nullptr, *tok = nullptr;
  WA_TRY(pad_to_device(d, pad, B, &pad_dev));
  WA_TRY(to_device<int>(d, tokens, (size_t)R, &tok));
  // through the device state the host position is a value no row may use
  DecodeState* st = nullptr;
  const DecodeState s0{pos0, 0, 0, 0};
  if (use_state) WA_TRY(to_device(d, &s0, 1, &st));
  const int pos0_host = use_state ? -1 : pos0;
  if (gamma_dev)
    WA_HIP(launch_embed_fold(tok, tok_emb_dev, pos_emb_dev, B, Tq, D, st, pos0_host, x_dev, gamma_dev,
                             static_cast<_Float16*>(tiled_dev), stats_dev, planes(prec), nullptr, pad_dev));
  else
    WA_HIP(launch_embed(tok, tok_emb_dev, pos_emb_dev, B, Tq, D, st, pos0_host, x_dev, nullptr, pad_dev));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// ---- the picks -------------------------------------------------------------
wq4_status wa_logits_pick_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                int step, wq4_precision prec, const int32_t* sup_ids, int n_sup,
                                const float* temperature, const uint64_t* seed, int ts0, const int32_t* records,
                                int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev, float* logits_dev) {
  if (!hid_dev || !emb_dev || !tok_dev) return fail(WQ4_EINVAL, "null argument");
  WA_TRY(pick_args_ok(n_clips, V, ts0, records, sup_ids, n_sup, temperature, seed, logprob_dev));
  if (!emb_tiled_supported(D) || (temperature && (step < 0 || step > 16))) return fail(WQ4_EINVAL, "bad sizes");
  const int ns = planes(prec);
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, sup_ids, n_sup, V, &sup));
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
  TsRule* rules = nullptr;
  float* temp = nullptr;
  uint64_t* sd = nullptr;
  WA_TRY(records_to_device(d, records, n_clips, &rules));
  WA_TRY(to_device(d, temperature, (size_t)n_clips, &temp));
  WA_TRY(to_device(d, seed, (size_t)n_clips, &sd));
  p.rules = rules;
  p.temp = temp;
  p.seed = sd;
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

wq4_status wa_row_pick_check(int device, const float* logits_dev, int n_rows, int V, int suppress_eot, int pick,
                             const int32_t* ids, int n_ids, const float* temperature, const uint64_t* seed, int ts0,
                             const int32_t* records, int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev) {
  if (!logits_dev || !tok_dev) return fail(WQ4_EINVAL, "null argument");
  WA_TRY(pick_args_ok(n_rows, V, ts0, records, ids, n_ids, temperature, seed, logprob_dev));
  if (pick < 0) return fail(WQ4_EINVAL, "bad sizes");
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, ids, n_ids, V, &sup));
  if (!temperature && !records) {  // the plain / scored pick of a stored row
    WA_HIP(launch_argmax(logits_dev, n_rows, V, 0, V, suppress_eot, tok_dev, 1, nullptr, nullptr, sup));
    if (logprob_dev)
      WA_HIP(launch_row_logprob(logits_dev, n_rows, V, 0, V, suppress_eot, 0, nullptr, tok_dev, 1, 0, logprob_dev, 1,
                                nullptr, sup));
    WA_HIP(hipDeviceSynchronize());
    return WQ4_OK;
  }
  TsRule* rules = nullptr;
  float* temp = nullptr;
  uint64_t* sd = nullptr;
  WA_TRY(to_device(d, temperature, (size_t)n_rows, &temp));
  WA_TRY(to_device(d, seed, (size_t)n_rows, &sd));
  WA_TRY(records_to_device(d, records, n_rows, &rules));
  WA_HIP(launch_row_pick(logits_dev, n_rows, V, V, suppress_eot, 0, nullptr, rules, ts0, temp, sd, pick, tok_dev,
                         logprob_dev, mass_dev, nullptr, nullptr, sup));
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

// ---- beam search -----------------------------------------------------------
wq4_status wa_beam_topk_check(int device, const float* logits_dev, int n_rows, int V, int kp, int suppress_eot,
                              int step, int eot_stop, int ts0, const int32_t* ids, int n_ids,
                              const int32_t* records, int32_t* tok_dev, float* lp_dev, int32_t* mass_dev,
                              int32_t* flag_out) {
  if (!logits_dev || !tok_dev || !lp_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || V < 16 || kp < 2 || kp > kBeamMaxTop || ts0 < 0 || ts0 > V ||
      ((records || n_ids != 0) && ts0 <= 50257))
    return fail(WQ4_EINVAL, "bad sizes");
  if (!sup_ok(ids, n_ids, sup_bound(ts0, V))) return fail(WQ4_EINVAL, "suppressed id outside [0, ts0)");
  WA_HIP(hipSetDevice(device));
  Dev d;
  const uint32_t* sup = nullptr;
  WA_TRY(sup_upload(d, ids, n_ids, V, &sup));
  auto* flag = d.alloc<int>(1);
  if (!flag) return fail(WQ4_ENOMEM, "allocation failed");
  TsRule* rules = nullptr;
  WA_TRY(records_to_device(d, records, n_rows, &rules));
  DecodeState* st = nullptr;
  const DecodeState s0{0, 0, step, 0};
  if (step >= 0) WA_TRY(to_device(d, &s0, 1, &st));
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

wq4_status wa_beam_select_check(int device, const int32_t* top_tok_dev, const float* top_lp_dev, float* S_dev,
                                int32_t* next_tok_dev, int32_t* parent_dev, int32_t* anc_dev, int32_t* fed_dev,
                                float* fin_sum_dev, int32_t* fin_len_dev, int32_t* fin_anc_dev, int32_t* fin_n_dev,
                                int32_t* complete_dev, int32_t* state_dev, int32_t* records_dev, int ts0, int V,
                                int n_clips, int K, int C, int ctx) {
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
  // without records the kernel reads neither ts0 nor V
  const BeamSelect a{top_tok_dev, top_lp_dev,  S_dev,       next_tok_dev, parent_dev,   anc_dev, fed_dev,
                     fin_sum_dev, fin_len_dev, fin_anc_dev, fin_n_dev,    complete_dev, ticket,
                     reinterpret_cast<DecodeState*>(state_dev), reinterpret_cast<TsRule*>(records_dev)};
  WA_HIP(launch_beam_select(a, n_clips, K, C, ctx, nullptr, ts0, V));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// ---- token alignment -------------------------------------------------------
wq4_status wa_align_matrix_check(int device, const float* q_dev, const float* k_dev, int n_clips, int P,
                                 const int32_t* pad, int T, int H, const int32_t* heads, int n_heads,
                                 const int32_t* F, int first_row, wq4_precision prec, float* matrix_out_dev) {
  if (!q_dev || !k_dev || !pad || !heads || !F || !matrix_out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || P < 1 || P > 448 || T < 4 || H < 1 || n_heads < 1 || first_row < 0)
    return fail(WQ4_EINVAL, "bad sizes");
  if (prec != WQ4_PREC_F16X2 && prec != WQ4_PREC_F16) return fail(WQ4_EINVAL, "unknown precision");
  std::set<int> seen;
  for (int i = 0; i < n_heads; ++i)
    if (heads[i] < 0 || heads[i] >= H || !seen.insert(heads[i]).second)
      return fail(WQ4_EINVAL, "heads must be distinct and in [0, H)");
  std::vector<int> r0(n_clips), N(n_clips);
  for (int c = 0; c < n_clips; ++c) {
    if (pad[c] < 0 || pad[c] >= P) return fail(WQ4_EINVAL, "pad out of range");
    if (F[c] < 4 || F[c] > T) return fail(WQ4_EINVAL, "F must be in [4, T]");
    r0[c] = pad[c] + first_row;
    N[c] = P - pad[c] - 1 - first_row;
    if (N[c] < 1) return fail(WQ4_EINVAL, "a clip needs at least one row: P - pad - 1 - first_row >= 1");
  }
  WA_HIP(hipSetDevice(device));
  Dev d;
  const int fld = align_fld(T);
  const size_t rows = (size_t)n_clips * P;
  float* w = d.alloc<float>((size_t)kAlignHeadsPerPass * rows * fld);
  float* msum = d.alloc<float>(rows * fld);
  if (!w || !msum) return fail(WQ4_ENOMEM, "allocation failed");
  int *pad_dev = nullptr, *F_dev = nullptr, *heads_dev = nullptr;
  WA_TRY(pad_to_device(d, pad, n_clips, &pad_dev));
  WA_TRY(to_device<int>(d, F, (size_t)n_clips, &F_dev));
  WA_TRY(to_device<int>(d, heads, (size_t)n_heads, &heads_dev));
  WA_HIP(hipMemset(matrix_out_dev, 0, rows * T * 4));
  for (int h0 = 0; h0 < n_heads; h0 += kAlignHeadsPerPass) {
    const int hp = std::min(kAlignHeadsPerPass, n_heads - h0);
    WA_HIP(launch_align_weights(q_dev, k_dev, n_clips, P, T, H, pad_dev, F_dev, heads_dev + h0, hp, w, fld,
                                planes(prec), nullptr));
    WA_HIP(launch_align_filter(w, n_clips, P, pad_dev, F_dev, hp, fld, msum, h0 == 0, h0 + hp == n_heads, n_heads,
                               nullptr));
  }
  for (int c = 0; c < n_clips; ++c)
    WA_HIP(copy_matrix(msum + (size_t)c * P * fld, fld, r0[c], N[c], F[c], matrix_out_dev + (size_t)c * P * T, T, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

wq4_status wa_dtw_check(int device, const float* x_dev, int n_clips, int N_ld, int F_ld, const int32_t* N,
                        const int32_t* F, int32_t* jump_out_dev, uint8_t* trace_out_dev) {
  if (!x_dev || !N || !F || !jump_out_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || N_ld < 1 || N_ld > 447 || F_ld < 1) return fail(WQ4_EINVAL, "bad sizes");
  for (int c = 0; c < n_clips; ++c)
    if (N[c] < 1 || N[c] > N_ld || F[c] < 1 || F[c] > F_ld) return fail(WQ4_EINVAL, "need 1 <= N <= N_ld, 1 <= F <= F_ld");
  WA_HIP(hipSetDevice(device));
  Dev d;
  int *N_dev = nullptr, *F_dev = nullptr;
  WA_TRY(to_device<int>(d, N, (size_t)n_clips, &N_dev));
  WA_TRY(to_device<int>(d, F, (size_t)n_clips, &F_dev));
  int* r0_dev = d.alloc<int>(n_clips);
  uint8_t* trace = trace_out_dev ? trace_out_dev : d.alloc<uint8_t>((size_t)n_clips * (N_ld + 1) * (F_ld + 1));
  if (!r0_dev || !trace) return fail(WQ4_ENOMEM, "allocation failed");
  WA_HIP(hipMemset(r0_dev, 0, (size_t)n_clips * 4));
  WA_HIP(launch_align_dtw(x_dev, (long)N_ld * F_ld, F_ld, r0_dev, N_dev, F_dev, n_clips, false, trace, N_ld, F_ld,
                          jump_out_dev, N_ld, nullptr));
  WA_HIP(hipDeviceSynchronize());
  return WQ4_OK;
}

// ---- host-only probes of the rules behind a decode's layout ----------------
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

long long wa_decode_graph_key_check(int mode, int lane, int b0, int nb, int eot, int trace, int group_kv,
                                    int range_tier, int splits, int residency) {
  return graph_key(mode, lane, b0, nb, eot, trace, group_kv, range_tier, splits, residency);
}

wq4_status wa_pipeline_unit_sizes(int n_batches, int width, int* sizes, int* n_units) {
  if (!sizes || !n_units) return fail(WQ4_EINVAL, "null argument");
  if (n_batches < 1 || width < 1 || width > kMaxLanes) return fail(WQ4_EINVAL, "n_batches >= 1, width in [1, 3]");
  const std::vector<int> s = unit_sizes(n_batches, width);
  std::copy(s.begin(), s.end(), sizes);
  *n_units = (int)s.size();
  return WQ4_OK;
}

}  // extern "C"
