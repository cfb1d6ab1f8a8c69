// wa_api.cpp -- the C ABI of include/whisper_amd.h beside the transcribe
// entries: model lifetime and queries, wa_encode / wa_prompt_logits, the
// kernel probe and the GGUF inspection calls.
#include "wa_model.hpp"

using namespace wa;

namespace {

thread_local std::string g_err;

// What both create entries do once their arguments are checked: the model
// with every weight of `src`, its activations and its stream.
wq4_status create_model(int device, int variant, int max_batch, wq4_precision prec, int weight_type, Source& src,
                        wa_model** out) {
  WA_HIP(hipSetDevice(device));
  std::unique_ptr<wa_model> m(new wa_model());
  m->device = device;
  m->cfg = preset(variant);
  m->prec = prec;
  m->ns = prec == WQ4_PREC_F16 ? 1 : 2;
  m->bmax = max_batch;
  kv_config(m.get(), max_batch);
  m->wtype = weight_type;
  WA_TRY(build_model(m.get(), src));
  WA_TRY(build_ln_fold(m.get()));
  WA_TRY(alloc_activations(m.get()));
  WA_HIP(hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking));
  WA_HIP(hipDeviceSynchronize());
  *out = m.release();
  return WQ4_OK;
}

}  // namespace

wq4_status wa::fail(wq4_status s, const std::string& m) {
  g_err = m;
  return s;
}

// ================================================================= C ABI ==
extern "C" {

const char* wa_last_error(void) { return g_err.c_str(); }

wq4_status wa_model_create_synthetic_ex(int device, int variant, uint64_t seed, int max_batch, wq4_precision prec,
                                        int weight_type, wa_model** out) {
  if (!out) return fail(WQ4_EINVAL, "out is null");
  *out = nullptr;
  if (variant < 0 || variant > 2) return fail(WQ4_EINVAL, "unknown variant");
  if (max_batch < 1 || max_batch > 256) return fail(WQ4_EINVAL, "max_batch must be in [1, 256]");
  if (prec != WQ4_PREC_F16X2 && prec != WQ4_PREC_F16) return fail(WQ4_EINVAL, "unknown precision");
  if (weight_type != 0 && weight_type != 1) return fail(WQ4_EINVAL, "weight_type must be 0 (Q4_0) or 1 (F16)");
  return create_model(device, variant, max_batch, prec, weight_type, *synth_source(seed), out);
}

wq4_status wa_model_create_synthetic(int device, int variant, uint64_t seed, int max_batch, wq4_precision prec,
                                     wa_model** out) {
  return wa_model_create_synthetic_ex(device, variant, seed, max_batch, prec, 0, out);
}

wq4_status wa_model_create_from_gguf(int device, const char* path, int variant, int max_batch, wq4_precision prec,
                                     wa_model** out) {
  if (!out || !path) return fail(WQ4_EINVAL, "null argument");
  *out = nullptr;
  if (variant < 0 || variant > 2) return fail(WQ4_EINVAL, "unknown variant");
  if (max_batch < 1 || max_batch > 256) return fail(WQ4_EINVAL, "max_batch must be in [1, 256]");
  if (prec != WQ4_PREC_F16X2 && prec != WQ4_PREC_F16) return fail(WQ4_EINVAL, "unknown precision");
  GgufFile file;
  if (!file.open(path)) return fail(WQ4_EINVAL, "Failed to parse GGUF: " + file.error());
  const GgufTensor* probe = file.find("encoder.blocks.0.attn.query.weight");
  const int wtype = probe && probe->type == kGgmlF16 ? 1 : 0;  // an F16 checkpoint (config 5)
  return create_model(device, variant, max_batch, prec, wtype, *gguf_source(file), out);
}

void wa_model_destroy(wa_model* m) { delete m; }

wq4_status wa_gguf_open(const char* path, wa_gguf** out) {
  if (!path || !out) return fail(WQ4_EINVAL, "null argument");
  *out = nullptr;
  auto* f = new GgufFile();
  if (!f->open(path)) {
    const std::string e = f->error();
    delete f;
    return fail(WQ4_EINVAL, "Failed to parse GGUF: " + e);
  }
  *out = reinterpret_cast<wa_gguf*>(f);
  return WQ4_OK;
}

void wa_gguf_close(wa_gguf* g) { delete reinterpret_cast<GgufFile*>(g); }

int wa_gguf_version(const wa_gguf* g) { return g ? (int)reinterpret_cast<const GgufFile*>(g)->version() : -1; }

int64_t wa_gguf_tensor_count(const wa_gguf* g) {
  return g ? (int64_t)reinterpret_cast<const GgufFile*>(g)->tensors().size() : -1;
}

wq4_status wa_gguf_tensor_info(const wa_gguf* g, int64_t index, char* name, size_t name_cap, int* ndims,
                               uint64_t* dims, int* type, uint64_t* offset, uint64_t* nbytes) {
  if (!g) return fail(WQ4_EINVAL, "null gguf");
  const auto& ts = reinterpret_cast<const GgufFile*>(g)->tensors();
  if (index < 0 || index >= (int64_t)ts.size()) return fail(WQ4_EINVAL, "tensor index out of range");
  const GgufTensor& t = ts[(size_t)index];
  if (name && name_cap) {
    const size_t n = std::min(name_cap - 1, t.name.size());
    std::memcpy(name, t.name.data(), n);
    name[n] = 0;
  }
  if (ndims) *ndims = (int)t.dims.size();
  if (dims)
    for (size_t i = 0; i < t.dims.size(); ++i) dims[i] = t.dims[i];
  if (type) *type = (int)t.type;
  if (offset) *offset = t.offset;
  if (nbytes) *nbytes = t.nbytes();
  return WQ4_OK;
}

wq4_status wa_gguf_tensor_data(const wa_gguf* g, const char* name, uint8_t* out, size_t cap) {
  if (!g || !name || !out) return fail(WQ4_EINVAL, "null argument");
  const auto* f = reinterpret_cast<const GgufFile*>(g);
  const GgufTensor* t = f->find(name);
  if (!t) return fail(WQ4_EINVAL, std::string("Tensor '") + name + "' not found in GGUF");
  const uint8_t* p = f->data(*t);
  if (!p) return fail(WQ4_EINVAL, std::string("Tensor '") + name + "' data lies outside the file");
  if (cap < t->nbytes()) return fail(WQ4_ENOMEM, "output buffer too small");
  std::memcpy(out, p, t->nbytes());
  return WQ4_OK;
}

int wa_model_weight_type(const wa_model* m) { return m ? m->wtype : -1; }

int wa_model_wide_range(const wa_model* m) { return m ? m->range_tier : -1; }

wq4_status wa_model_config(const wa_model* m, int32_t* cfg) {
  if (!m || !cfg) return fail(WQ4_EINVAL, "null argument");
  const Config& c = m->cfg;
  const int32_t v[WA_CFG_COUNT] = {c.n_mels,       c.n_audio_ctx,  c.n_audio_state, c.n_audio_head,
                                   c.n_audio_layer, c.n_text_ctx,   c.n_text_state,  c.n_text_head,
                                   c.n_text_layer,  c.n_vocab,      c.n_lang};
  std::memcpy(cfg, v, sizeof(v));
  return WQ4_OK;
}

size_t wa_model_device_bytes(const wa_model* m) { return m ? m->bytes : 0; }

// The validity rule of the suppress-token lists (host only).
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

wq4_status wa_model_set_suppress(wa_model* m, const int32_t* always, int n_always, const int32_t* first, int n_first) {
  if (!m) return fail(WQ4_EINVAL, "null model");
  WA_TRY(wa_suppress_check(always, n_always, first, n_first, m->ts0()));  // host only: nothing is set on failure
  WA_HIP(hipSetDevice(m->device));
  const int V = m->cfg.n_vocab;
  const size_t W = (size_t)sup_mask_words(V);
  if (n_always + n_first > 0) {
    if (!m->sup_buf) {
      m->sup_buf = m->dev.alloc<uint32_t>(2 * W);
      if (!m->sup_buf) return fail(WQ4_ENOMEM, "suppress mask allocation failed");
      m->bytes += 2 * W * sizeof(uint32_t);
    }
    // [0, W): always; [W, 2 W): always | first
    std::vector<int32_t> both(always, always + n_always);
    both.insert(both.end(), first, first + n_first);
    std::vector<uint32_t> words(2 * W);
    sup_mask_build(always, n_always, V, words.data());
    sup_mask_build(both.data(), (int)both.size(), V, words.data() + W);
    WA_HIP(hipDeviceSynchronize());  // no earlier call still reads the masks
    WA_HIP(hipMemcpy(m->sup_buf, words.data(), 2 * W * sizeof(uint32_t), hipMemcpyHostToDevice));
    m->sup_mask = m->sup_buf;
    m->sup_mask0 = m->sup_buf + W;
  } else {
    m->sup_mask = m->sup_mask0 = nullptr;
  }
  m->sup_always.assign(always, always + n_always);
  m->sup_first.assign(first, first + n_first);
  m->drop_graphs();
  return WQ4_OK;
}

wq4_status wa_model_suppress_ids(const wa_model* m, int which, int32_t* out, int cap, int* n) {
  if (!m || !n || (which != 0 && which != 1)) return fail(WQ4_EINVAL, "bad arguments");
  const std::vector<int32_t>& ids = which ? m->sup_first : m->sup_always;
  *n = (int)ids.size();
  if (cap < *n || (*n > 0 && !out)) return fail(WQ4_EINVAL, "out holds fewer ids than the list");
  std::copy(ids.begin(), ids.end(), out);
  return WQ4_OK;
}

wq4_status wa_last_timings(const wa_model* m, float* out) {
  if (!m || !out) return fail(WQ4_EINVAL, "null argument");
  std::memcpy(out, m->timings, sizeof(m->timings));
  return WQ4_OK;
}

wq4_status wa_profile_enable(wa_model* m, int enable) {
  if (!m) return fail(WQ4_EINVAL, "null model");
  m->profile = enable != 0;
  return WQ4_OK;
}

wq4_status wa_profile_read(wa_model* m, double* out, int reset) {
  if (!m || !out) return fail(WQ4_EINVAL, "null argument");
  m->resolve_profile();
  std::memcpy(out, m->prof, sizeof(m->prof));
  if (reset) std::memset(m->prof, 0, sizeof(m->prof));
  return WQ4_OK;
}

wq4_status wa_encode(wa_model* m, const float* mel_dev, int n_clips, float* enc_out_dev, void* stream) {
  if (!m || !mel_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > m->bmax) return fail(WQ4_EINVAL, "n_clips out of range");
  WA_HIP(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  WA_TRY(encoder_forward(m, mel_dev, n_clips, st, enc_out_dev));
  return cross_kv_forward(m, n_clips, st, false);
}

wq4_status wa_prompt_logits(wa_model* m, const int32_t* prompt_dev, int n_clips, int plen, float* logits_dev,
                            void* stream) {
  if (!m || !prompt_dev || !logits_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > m->bmax || plen < 1 || plen > 4) return fail(WQ4_EINVAL, "bad n_clips / plen");
  if (n_clips > m->kv_batch) return fail(WQ4_EINVAL, "wa_encode the clips first");
  WA_HIP(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  DecGroup& g = m->groups[0];
  g.lane = 0;
  g.b0 = 0;
  g.nb = n_clips;
  g.xres = xattn_residency(n_clips, m->cfg.n_audio_ctx, m->ns, m->cfg.n_audio_state);
  g.xplan = xattn_plan(m->cfg.n_audio_ctx, n_clips);
  WA_TRY(decoder_forward(m, g, DecodeCall(), prompt_dev, plen, nullptr, 0, 0, st));
  WA_HIP(hipMemcpyAsync(logits_dev, g.logits, (size_t)n_clips * m->cfg.n_vocab * 4, hipMemcpyDeviceToDevice, st));
  return WQ4_OK;
}

long long wa_decode_graph_key(const wa_model* m, int group) {
  if (!m || group < 0 || group >= (int)m->groups.size()) return -1;
  return m->groups[group].graph_key;
}

int wa_decode_group_rows(int n_clips) {
  if (n_clips < 1) return 0;
  const int G = decode_groups(n_clips);
  return (n_clips + G - 1) / G;  // the largest group (groups split [0, B) evenly, run_decode)
}

constexpr int kProbeOut = WA_PROBE_OUT;

wq4_status wa_probe_kernels(wa_model* m, int n_clips, int iters, double* out, int out_len) {
  if (!m || !out) return fail(WQ4_EINVAL, "null argument");
  if (out_len < kProbeOut) return fail(WQ4_EINVAL, "out holds fewer than 6 doubles");
  if (n_clips < 1 || n_clips > m->bmax || iters < 1) return fail(WQ4_EINVAL, "bad n_clips / iters");
  if (n_clips > m->kv_batch) return fail(WQ4_EINVAL, "run wa_transcribe / wa_encode on n_clips clips first");
  WA_HIP(hipSetDevice(m->device));
  hipStream_t st = m->own_stream;
  const Config& c = m->cfg;
  const int B = n_clips, D = c.n_text_state, T = c.n_audio_ctx, H = c.n_text_head;
  DecLayer& L = m->dec[0];
  DecGroup g = m->groups[0];  // group 0's buffers, a clip range of its own
  const _Float16* enc = m->lanes[0].planes;
  hipEvent_t a, b;
  WA_HIP(hipEventCreate(&a));
  WA_HIP(hipEventCreate(&b));
  float ms = 0.0f;
  // cross-attention of one decode step (Tq = 1) in the form a decode group of
  // n_clips clips runs: over the cached K / V (few clips) or streaming every
  // clip's encoder output
  g.b0 = 0;
  g.nb = B;
  const bool kv = m->group_kv(g);
  const XattnResidency res = xattn_residency(B, T, m->ns, D);  // the launch alone: its own clips are all that is live
  const XattnPlan plan = xattn_plan(T, B);                     // and nothing runs beside it
  auto xattn = [&]() -> hipError_t {
    if (kv)
      return launch_cross_attention_kv(g.qd, L.xk, L.xv, B, 1, T, H, g.xkv_part, g.xkv_ctr, g.atd_dec, m->ns, st);
    return launch_xattn(g.qd, L.ck_raw, L.cv_raw, L.cv_p, L.cv_b, m->wtype, enc, B, 1, T, H, D, g.xqt, g.xattn_part,
                        g.atd_dec, m->ns, res, plan, st);
  };
  WA_HIP(xattn());
  WA_HIP(hipEventRecord(a, st));
  for (int i = 0; i < iters; ++i) WA_HIP(xattn());
  WA_HIP(hipEventRecord(b, st));
  WA_HIP(hipEventSynchronize(b));
  WA_HIP(hipEventElapsedTime(&ms, a, b));
  out[0] = ms * 1e3 / iters;
  // algorithmic bytes: the cached K and V (f32) of every clip, or the
  // encoder output planes of every clip + Wk, Wv (raw); + q + output operand
  const double wbytes = m->wtype == 1 ? 2.0 * D * D * 2 : 2.0 * D * D * 18 / 32;
  out[1] = kv ? (double)B * T * D * 4 * 2 + (double)B * D * (4 + 2 * m->ns)
              : (double)B * T * D * 2 * m->ns + wbytes + (double)B * D * (4 + 2 * m->ns);
  out[5] = kv ? 1.0 : 0.0;
  // fc1 of one decode step (M = n_clips rows, decode kernel, GELU + tiled out)
  const int F = 4 * D;
  WA_WQ4(wq4_gemm_tiled(L.fc1, L.fc1_b, g.atd_dec, nullptr, nullptr, g.atf_dec, B, WQ4_EPI_GELU | WQ4_EPI_TILED_OUT,
                        m->prec, 2, st));
  WA_HIP(hipEventRecord(a, st));
  for (int i = 0; i < iters; ++i)
    WA_WQ4(wq4_gemm_tiled(L.fc1, L.fc1_b, g.atd_dec, nullptr, nullptr, g.atf_dec, B,
                          WQ4_EPI_GELU | WQ4_EPI_TILED_OUT, m->prec, 2, st));
  WA_HIP(hipEventRecord(b, st));
  WA_HIP(hipEventSynchronize(b));
  WA_HIP(hipEventElapsedTime(&ms, a, b));
  out[2] = ms * 1e3 / iters;
  out[3] = (double)F * D * 18 / 32 + (double)B * D * 2 * m->ns + (double)B * F * 2 * m->ns;
  out[4] = 2.0 * B * F * D;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return WQ4_OK;
}

}  // extern "C"
