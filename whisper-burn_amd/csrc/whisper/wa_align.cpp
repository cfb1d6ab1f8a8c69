// wa_align.cpp -- token-level alignment (wa_align): the capture hook of the
// prefill pass (align_layer), the model's alignment buffers and the entries.
// Kernels: wa_align.hip.
#include <set>

#include "wa_model.hpp"

using namespace wa;

namespace {

// the alignment heads grouped by layer (ascending), the caller's order inside
// a layer: the order the prefill meets them in, which is the order of the sums
std::vector<std::pair<int, int>> ordered_heads(const wa_model* m) {
  std::vector<std::pair<int, int>> v = m->al.pairs;
  if (v.empty())  // OpenAI's default: every head of the upper half of the layers
    for (int l = m->cfg.n_text_layer / 2; l < m->cfg.n_text_layer; ++l)
      for (int h = 0; h < m->cfg.n_text_head; ++h) v.emplace_back(l, h);
  std::stable_sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  return v;
}

// The alignment buffers (wa_model::Align), once, all or nothing.
wq4_status ensure_align(wa_model* m) {
  wa_model::Align& al = m->al;
  if (al.ok) return WQ4_OK;
  const Config& c = m->cfg;
  const size_t B = (size_t)m->bmax, ctx = (size_t)c.n_text_ctx, fld = (size_t)align_fld(c.n_audio_ctx);
  const size_t nw = kAlignHeadsPerPass * B * ctx * fld, nm = B * ctx * fld, nt = B * ctx * (c.n_audio_ctx + 1);
  const size_t nh = (size_t)c.n_text_layer * c.n_text_head;
  al.fld = (int)fld;
  al.w = m->dev.alloc<float>(nw);
  al.msum = m->dev.alloc<float>(nm);
  al.trace = m->dev.alloc<uint8_t>(nt);
  al.F = m->dev.alloc<int>(B);
  al.row0 = m->dev.alloc<int>(B);
  al.N = m->dev.alloc<int>(B);
  al.heads = m->dev.alloc<int>(nh);
  al.jump = m->dev.alloc<int>(B * ctx);
  if (!al.w || !al.msum || !al.trace || !al.F || !al.row0 || !al.N || !al.heads || !al.jump) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (void* p : {(void*)al.w, (void*)al.msum, (void*)al.trace, (void*)al.F, (void*)al.row0, (void*)al.N,
                    (void*)al.heads, (void*)al.jump})
      m->dev.release(p);
    al.w = al.msum = nullptr;
    al.trace = nullptr;
    al.F = al.row0 = al.N = al.heads = al.jump = nullptr;
    return fail(WQ4_ENOMEM, "alignment buffer allocation failed");
  }
  m->bytes += (nw + nm) * 4 + nt + (3 * B + nh + B * ctx) * 4;
  al.ok = true;
  return WQ4_OK;
}

struct Events {
  std::vector<hipEvent_t> all;
  ~Events() {
    for (hipEvent_t e : all) (void)hipEventDestroy(e);
  }
  hipError_t make(hipEvent_t* e) {
    const hipError_t r = hipEventCreate(e);
    if (r == hipSuccess) all.push_back(*e);
    return r;
  }
};

}  // namespace

namespace wa {

// The rows [row0, row0 + N) x [0, F) of a clip's msum [.][fld] -> dst [.][dst_ld], on st
hipError_t copy_matrix(const float* msum, int fld, int row0, int N, int F, float* dst, int dst_ld, hipStream_t st) {
  return hipMemcpy2DAsync(dst, (size_t)dst_ld * 4, msum + (size_t)row0 * fld, (size_t)fld * 4, (size_t)F * 4, (size_t)N,
                          hipMemcpyDeviceToDevice, st);
}

wq4_status align_layer(wa_model* m, DecGroup& g, int li, const float* xk, int P, hipStream_t st, bool* done) {
  const Config& c = m->cfg;
  const wa_model::Align& al = m->al;
  const std::vector<std::pair<int, int>> heads = ordered_heads(m);  // as wa_align uploaded them to al.heads
  const int total = (int)heads.size();
  int first = 0;
  while (first < total && heads[first].first < li) ++first;
  int end = first;
  while (end < total && heads[end].first == li) ++end;
  *done = end == total;
  for (int h0 = first; h0 < end; h0 += kAlignHeadsPerPass) {
    const int hp = std::min(kAlignHeadsPerPass, end - h0);
    WA_HIP(launch_align_weights(m->pf.q, xk, g.nb, P, c.n_audio_ctx, c.n_text_head, g.pad, al.F + g.b0, al.heads + h0, hp,
                                al.w, al.fld, m->ns, st));
    WA_HIP(launch_align_filter(al.w, g.nb, P, g.pad, al.F + g.b0, hp, al.fld, al.msum, h0 == 0, h0 + hp == total, total,
                               st));
  }
  return WQ4_OK;
}

}  // namespace wa

extern "C" {

wq4_status wa_alignment_heads_check(const int32_t* layer_head, int n, int n_text_layer, int n_text_head) {
  if (n < 0 || (n > 0 && !layer_head)) return fail(WQ4_EINVAL, "bad alignment head list");
  std::set<std::pair<int, int>> seen;
  for (int i = 0; i < n; ++i) {
    const int l = layer_head[2 * i], h = layer_head[2 * i + 1];
    if (l < 0 || l >= n_text_layer || h < 0 || h >= n_text_head)
      return fail(WQ4_EINVAL, "alignment head outside [0, n_text_layer) x [0, n_text_head)");
    if (!seen.insert({l, h}).second) return fail(WQ4_EINVAL, "alignment head listed twice");
  }
  return WQ4_OK;
}

wq4_status wa_model_set_alignment_heads(wa_model* m, const int32_t* layer_head, int n) {
  if (!m) return fail(WQ4_EINVAL, "null model");
  WA_TRY(wa_alignment_heads_check(layer_head, n, m->cfg.n_text_layer, m->cfg.n_text_head));
  std::vector<std::pair<int, int>> pairs;
  for (int i = 0; i < n; ++i) pairs.emplace_back(layer_head[2 * i], layer_head[2 * i + 1]);
  m->al.pairs = pairs;  // empty: the default
  return WQ4_OK;
}

wq4_status wa_align_check(const wa_prompt* tokens, int n_clips, const int32_t* first_row, const int32_t* n_frames,
                          int n_vocab, int n_text_ctx, int n_audio_ctx) {
  if (!tokens || !first_row || !n_frames) return fail(WQ4_EINVAL, "null argument");
  WA_TRY(wa_prompt_check(tokens, n_clips, n_vocab, n_text_ctx, 0));
  if (n_audio_ctx < 4) return fail(WQ4_EINVAL, "bad sizes");
  for (int i = 0; i < n_clips; ++i) {
    if (first_row[i] < 0) return fail(WQ4_EINVAL, "first_row must be >= 0");
    if (tokens->n_tokens[i] - 1 - first_row[i] < 1)
      return fail(WQ4_EINVAL, "a clip needs at least one row: n_tokens - 1 - first_row >= 1");
    if (n_frames[i] < 8 || n_frames[i] > 2 * n_audio_ctx)
      return fail(WQ4_EINVAL, "n_frames must be in [8, 2 * n_audio_ctx]");
  }
  return WQ4_OK;
}

wq4_status wa_align(wa_model* m, const float* mel_dev, int n_clips, const wa_prompt* tokens, const int32_t* first_row,
                    const int32_t* n_frames, int32_t* jump_out, int32_t* n_rows_out, float* matrix_out_dev,
                    void* stream) {
  if (!m || !mel_dev || !tokens || !first_row || !n_frames || !jump_out || !n_rows_out)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > m->bmax) return fail(WQ4_EINVAL, "n_clips out of range");
  const Config& c = m->cfg;
  WA_TRY(wa_align_check(tokens, n_clips, first_row, n_frames, c.n_vocab, c.n_text_ctx, c.n_audio_ctx));
  WA_HIP(hipSetDevice(m->device));
  WA_TRY(ensure_prefill(m));
  WA_TRY(ensure_align(m));
  wa_model::Align& al = m->al;
  const int B = n_clips, ctx = c.n_text_ctx, T = c.n_audio_ctx, ld = tokens->ld;
  hipStream_t st = m->own_stream;  // the model's own stream, ordered after the caller's
  Events ev;
  hipEvent_t e_in, e_enc, e_ready, e_end;
  for (hipEvent_t* e : {&e_in, &e_enc, &e_ready, &e_end}) WA_HIP(ev.make(e));
  WA_HIP(hipEventRecord(e_in, static_cast<hipStream_t>(stream)));
  WA_HIP(hipStreamWaitEvent(st, e_in, 0));
  std::vector<int> hd;  // the heads in the order align_layer walks them
  for (const auto& p : ordered_heads(m)) hd.push_back(p.second);
  WA_HIP(hipMemcpyAsync(al.heads, hd.data(), hd.size() * 4, hipMemcpyHostToDevice, st));
  if (matrix_out_dev) WA_HIP(hipMemsetAsync(matrix_out_dev, 0, (size_t)B * ld * T * 4, st));
  WA_HIP(hipEventRecord(e_enc, st));
  WA_TRY(encoder_forward(m, mel_dev, B, st, nullptr));
  WA_TRY(cross_kv_forward(m, B, st, true));
  WA_HIP(hipEventRecord(e_ready, st));
  // the decode groups of a transcribe of B clips, one after another on st
  const int G = decode_groups(B);
  std::vector<int> jump((size_t)B * ctx, -1), Fh(B), Nh(B), r0(B);
  std::vector<hipEvent_t> e_pf(G), e_dtw(G);
  for (int i = 0; i < G; ++i) {
    WA_HIP(ev.make(&e_pf[i]));
    WA_HIP(ev.make(&e_dtw[i]));
    DecGroup& g = m->groups[i];
    g.lane = 0;
    g.b0 = (int)((int64_t)B * i / G);
    g.nb = (int)((int64_t)B * (i + 1) / G) - g.b0;
    g.clip0 = g.b0;
    int P = 0;
    for (int b = 0; b < g.nb; ++b) P = std::max(P, tokens->n_tokens[g.b0 + b]);
    for (int b = g.b0; b < g.b0 + g.nb; ++b) {
      Fh[b] = n_frames[b] / 2;
      Nh[b] = tokens->n_tokens[b] - 1 - first_row[b];
      r0[b] = P - tokens->n_tokens[b] + first_row[b];  // the clip's pad + its first matrix row
    }
    WA_HIP(hipMemcpyAsync(al.F + g.b0, Fh.data() + g.b0, (size_t)g.nb * 4, hipMemcpyHostToDevice, st));
    WA_HIP(hipMemcpyAsync(al.N + g.b0, Nh.data() + g.b0, (size_t)g.nb * 4, hipMemcpyHostToDevice, st));
    WA_HIP(hipMemcpyAsync(al.row0 + g.b0, r0.data() + g.b0, (size_t)g.nb * 4, hipMemcpyHostToDevice, st));
    DecodeCall call;
    call.prompt = tokens;
    call.align = true;
    int Pg = 0;
    WA_TRY(prefill_group(m, g, call, st, &Pg));
    WA_HIP(hipEventRecord(e_pf[i], st));
    WA_HIP(launch_align_dtw(al.msum, (long)Pg * al.fld, al.fld, al.row0 + g.b0, al.N + g.b0, al.F + g.b0, g.nb, true,
                            al.trace, ctx - 1, T, al.jump + (size_t)g.b0 * ctx, ctx, st));
    WA_HIP(hipEventRecord(e_dtw[i], st));
    if (matrix_out_dev)
      for (int b = 0; b < g.nb; ++b)
        WA_HIP(copy_matrix(al.msum + (size_t)b * Pg * al.fld, al.fld, r0[g.b0 + b], Nh[g.b0 + b], Fh[g.b0 + b],
                           matrix_out_dev + (size_t)(g.b0 + b) * ld * T, T, st));
    WA_HIP(hipMemcpyAsync(jump.data() + (size_t)g.b0 * ctx, al.jump + (size_t)g.b0 * ctx, (size_t)g.nb * ctx * 4,
                          hipMemcpyDeviceToHost, st));
  }
  WA_HIP(hipEventRecord(e_end, st));
  WA_HIP(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    n_rows_out[b] = Nh[b];
    for (int i = 0; i < ld; ++i) jump_out[(size_t)b * ld + i] = i < Nh[b] ? jump[(size_t)b * ctx + i] : -1;
  }
  float t_enc = 0.0f, t_pf = 0.0f, t_dtw = 0.0f, t_all = 0.0f;
  WA_HIP(hipEventElapsedTime(&t_enc, e_enc, e_ready));
  WA_HIP(hipEventElapsedTime(&t_all, e_enc, e_end));
  for (int i = 0; i < G; ++i) {
    float a = 0.0f, d = 0.0f;
    WA_HIP(hipEventElapsedTime(&a, i == 0 ? e_ready : e_dtw[i - 1], e_pf[i]));
    WA_HIP(hipEventElapsedTime(&d, e_pf[i], e_dtw[i]));
    t_pf += a;
    t_dtw += d;
  }
  const float t[4] = {t_enc, t_pf, t_dtw, t_all};
  std::memcpy(al.timings, t, sizeof(t));
  return WQ4_OK;
}

wq4_status wa_last_align_timings(const wa_model* m, float* out) {
  if (!m || !out) return fail(WQ4_EINVAL, "null argument");
  std::memcpy(out, m->al.timings, sizeof(m->al.timings));
  return WQ4_OK;
}

wq4_status wa_align_words(const int32_t* jump, int n_rows, const int32_t* word_len, int n_words, float* start_s,
                          float* end_s) {
  if (!jump || !word_len || !start_s || !end_s) return fail(WQ4_EINVAL, "null argument");
  if (n_rows < 1 || n_words < 0) return fail(WQ4_EINVAL, "bad sizes");
  int64_t sum = 0;
  for (int k = 0; k < n_words; ++k) {
    if (word_len[k] < 0) return fail(WQ4_EINVAL, "negative word length");
    sum += word_len[k];
  }
  if (sum != n_rows - 1) return fail(WQ4_EINVAL, "word lengths must sum to n_rows - 1");
  int bnd = 0;
  for (int k = 0; k < n_words; ++k) {
    start_s[k] = (float)jump[bnd] / 50.0f;
    bnd += word_len[k];
    end_s[k] = (float)jump[bnd] / 50.0f;
  }
  return WQ4_OK;
}

}  // extern "C"
