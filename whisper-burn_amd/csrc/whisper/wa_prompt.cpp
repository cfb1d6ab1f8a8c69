// wa_prompt.cpp -- caller prompts of any length (wa_transcribe_prompted): the
// prefill pass of a decode group over ragged, right-aligned prompts, and its
// entries.  The decode steps after it are wa_forward.cpp's, in the pad forms of
// the embedding and self-attention.
#include <cmath>

#include "wa_model.hpp"

using namespace wa;

namespace {

constexpr int kSOT = 50258;

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace

namespace wa {

wq4_status check_prompt(const wa_model* m, const wa_prompt* p, int n_clips, int max_tokens) {
  return static_cast<wq4_status>(wa_prompt_check(p, n_clips, m->cfg.n_vocab, m->cfg.n_text_ctx, max_tokens));
}

// The prefill's buffers (wa_model::Prefill), once: carved from the encoder's
// where they fit (the released models: 448 decoder rows per clip against 1500
// encoder rows), else allocated.
wq4_status ensure_prefill(wa_model* m) {
  if (m->pf.ok) return WQ4_OK;
  const Config& c = m->cfg;
  const int64_t rows = (int64_t)m->bmax * c.n_text_ctx, renc = (int64_t)m->bmax * c.n_audio_ctx;
  const int64_t D = c.n_text_state, Da = c.n_audio_state;
  wa_model::Prefill pf;
  size_t own = 0;
  std::vector<void*> owned;  // what this call allocated (a failure releases it, never a borrowed buffer)
  auto f32 = [&](int64_t n) {
    own += (size_t)n * 4;
    float* p = m->dev.alloc<float>((size_t)n);
    owned.push_back(p);
    return p;
  };
  if (3 * rows * D <= renc * 2 * Da) {
    pf.x = m->h1;
    pf.q = m->h1 + rows * D;
    pf.hid = m->h1 + 2 * rows * D;
  } else {
    pf.x = f32(rows * D);
    pf.q = f32(rows * D);
    pf.hid = f32(rows * D);
  }
  pf.qkv = rows * 3 * D <= renc * 3 * Da ? m->qkv : f32(rows * 3 * D);
  const size_t nf = align256(wq4_atiled_bytes(rows, 4 * D, m->prec)), nd = wq4_atiled_bytes(rows, D, m->prec);
  if (nf + nd <= wq4_atiled_bytes(renc, 4 * Da, m->prec)) {
    pf.atf = m->at_f;
    pf.atd = reinterpret_cast<_Float16*>(reinterpret_cast<uint8_t*>(m->at_f) + nf);
  } else {
    pf.atf = m->dev.alloc<_Float16>(nf / 2);
    pf.atd = m->dev.alloc<_Float16>(nd / 2);
    own += nf + nd;
    owned.push_back(pf.atf);
    owned.push_back(pf.atd);
    if (pf.atf && pf.atd) {  // padded rows stay finite
      WA_HIP(hipMemset(pf.atf, 0, nf));
      WA_HIP(hipMemset(pf.atd, 0, nd));
    }
  }
  pf.tok = m->dev.alloc<int>((size_t)rows);
  own += (size_t)rows * 4;
  owned.push_back(pf.tok);
  bool ok = pf.x && pf.q && pf.hid && pf.qkv && pf.atf && pf.atd && pf.tok;
  for (DecGroup& g : m->groups) {
    if (!g.pad) g.pad = m->dev.alloc<int>((size_t)m->bmax);
    ok = ok && g.pad;
  }
  if (!ok) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (void* p : owned) m->dev.release(p);
    for (DecGroup& g : m->groups) {
      m->dev.release(g.pad);
      g.pad = nullptr;
    }
    return fail(WQ4_ENOMEM, "prefill buffer allocation failed");
  }
  m->bytes += own + m->groups.size() * (size_t)m->bmax * 4;
  pf.ok = true;
  m->pf = pf;
  return WQ4_OK;
}

// One layer's cross-attention K / V for max_batch clips: allocated by the
// first prefill of a group without the few-clip caches.
static wq4_status ensure_prefill_kv(wa_model* m) {
  if (m->pf.xk) return WQ4_OK;
  if (!m->dec.front().ck || !m->dec.front().cv)
    return fail(WQ4_EINVAL, "a prompted call needs the cross K / V projections (WA_XATTN_KV_CLIPS=0 drops them)");
  const size_t n = (size_t)m->bmax * m->cfg.n_audio_ctx * m->cfg.n_text_state;
  float* k = m->dev.alloc<float>(n);
  float* v = m->dev.alloc<float>(n);
  if (!k || !v) {
    (void)hipGetLastError();
    m->dev.release(k);
    m->dev.release(v);
    return fail(WQ4_ENOMEM, "prefill cross K / V allocation failed");
  }
  m->pf.xk = k;
  m->pf.xv = v;
  m->bytes += n * 8;
  return WQ4_OK;
}

wq4_status prefill_group(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st, int* P_out) {
  const Config& c = m->cfg;
  const wa_prompt& pr = *call.prompt;
  const int D = c.n_text_state, H = c.n_text_head, T = c.n_audio_ctx, B = g.nb, V = c.n_vocab;
  WA_TRY(ensure_prefill(m));
  const wa_model::Prefill& pf = m->pf;
  // right-align the group's prompts to its longest; a pad row carries the
  // clip's first id (valid; its activations are never read by a real row)
  int P = 0;
  for (int b = 0; b < B; ++b) P = std::max(P, pr.n_tokens[g.clip0 + b]);
  const int64_t rows = (int64_t)B * P;
  std::vector<int> tok((size_t)rows), pad(B), sot_row(B), lang(B);
  for (int b = 0; b < B; ++b) {
    const int n = pr.n_tokens[g.clip0 + b];
    const int32_t* src = pr.tokens + (size_t)(g.clip0 + b) * pr.ld;
    pad[b] = P - n;
    for (int t = 0; t < P; ++t) tok[(size_t)b * P + t] = src[std::max(0, t - pad[b])];
    // the scores' positions: the last SOT and the id after it
    int sot = -1;
    for (int i = 0; i < n; ++i)
      if (src[i] == kSOT) sot = i;
    sot_row[b] = sot < 0 ? -1 : pad[b] + sot;
    const int nxt = sot >= 0 && sot + 1 < n ? src[sot + 1] : -1;
    lang[b] = nxt >= 50259 && nxt < 50259 + c.n_lang ? nxt : -1;
  }
  WA_HIP(hipMemcpyAsync(pf.tok, tok.data(), (size_t)rows * 4, hipMemcpyHostToDevice, st));  // pageable: staged
  WA_HIP(hipMemcpyAsync(g.pad, pad.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));

  const Lane& lane = m->lanes[g.lane];
  const size_t self_ofs = (size_t)g.b0 * H * c.n_text_ctx * 64;
  const bool kv = m->group_kv(g);
  if (!kv) {
    // ln_post of this group's clips as the K / V GEMMs' operand (m->x still
    // holds its input; m->at_d is free: cross_kv_forward fills it the same way)
    WA_TRY(ensure_prefill_kv(m));
    const int64_t kv_rows = (int64_t)B * T;
    WA_WQ4(wq4_layernorm(m->x + (size_t)g.b0 * T * c.n_audio_state, m->lnp_w, m->lnp_b, kv_rows, c.n_audio_state,
                         m->prec, m->at_d, nullptr, st));
  }
  void* ffn_ws = nullptr;
  size_t ffn_ws_bytes = 0;
  if (m->abi_ffn()) {  // range tier 2: the encoder's workspace (idle, and sized for more rows)
    ffn_ws_bytes = wq4_ffn_workspace_bytes(m->dec.front().fc1, m->dec.front().fc2, rows);
    if (ffn_ws_bytes == 0 || ffn_ws_bytes > m->ffn_ws_bytes) return fail(WQ4_EINVAL, "prefill FFN workspace size");
    ffn_ws = m->ffn_ws;
  }
  float* const a32 = m->f32_attn() ? pf.hid : nullptr;  // range tier 3, as decoder_forward
  const size_t atd_bytes = wq4_atiled_bytes(rows, D, m->prec);
  // every GEMM on the tile kernel: a row's bits do not depend on the row count
  auto ln_gemm = [&](const wq4_tensor* w, const float* bias, const float* lw, const float* lb, float* y, void* yt,
                     unsigned flags) -> wq4_status {
    WA_WQ4(wq4_layernorm(pf.x, lw, lb, rows, D, m->prec, pf.atd, nullptr, st));
    WA_WQ4(wq4_gemm_tiled(w, bias, pf.atd, nullptr, y, yt, rows, flags, m->prec, 1, st));
    return WQ4_OK;
  };
  auto resid_gemm = [&](const wq4_tensor* w, const float* bias, const void* at, const float* x32) -> wq4_status {
    if (x32)
      WA_WQ4(wq4_linear_forward_ws(w, bias, x32, pf.x, pf.x, rows, D, WQ4_EPI_RESIDUAL, m->prec, pf.atd, atd_bytes, st));
    else
      WA_WQ4(wq4_gemm_tiled(w, bias, at, pf.x, pf.x, nullptr, rows, WQ4_EPI_RESIDUAL, m->prec, 1, st));
    return WQ4_OK;
  };
  WA_HIP(launch_embed(pf.tok, m->tok_emb, m->dec_pos, B, P, D, nullptr, 0, pf.x, st, g.pad));
  for (DecLayer& L : m->dec) {  // DecoderBlock::forward_prompt (decoder.rs:77-112) over P rows per clip
    WA_TRY(ln_gemm(L.qkv, L.qkv_b, L.ln1_w, L.ln1_b, pf.qkv, nullptr, 0u));
    const size_t li = (size_t)(&L - m->dec.data());
    WA_HIP(launch_prefill_self_attention(pf.qkv, lane.cache_k[li] + self_ofs, lane.cache_v[li] + self_ofs, B, P, H,
                                         c.n_text_ctx, g.pad, pf.atd, m->ns, st, a32));
    WA_TRY(resid_gemm(L.out, L.out_b, pf.atd, a32));
    WA_TRY(ln_gemm(L.cq, L.cq_b, L.ln2_w, L.ln2_b, pf.q, nullptr, 0u));
    const float *xk, *xv;
    if (kv) {
      xk = L.xk + (size_t)g.b0 * T * D;
      xv = L.xv + (size_t)g.b0 * T * D;
    } else {  // this layer's K / V of the group's clips, as cross_kv_forward forms the caches
      WA_WQ4(wq4_gemm_tiled_headmajor(L.ck, nullptr, m->at_d, pf.xk, (int64_t)B * T, T, D, m->prec, 0, st));
      WA_WQ4(wq4_gemm_tiled_headmajor(L.cv, L.cv_b, m->at_d, pf.xv, (int64_t)B * T, T, D, m->prec, 0, st));
      xk = pf.xk;
      xv = pf.xv;
    }
    if (call.align) {
      bool done = false;
      WA_TRY(align_layer(m, g, (int)li, xk, P, st, &done));
      if (done) break;
    }
    WA_HIP(launch_prefill_cross_attention(pf.q, xk, xv, B, P, T, H, pf.atd, m->ns, st, a32));
    WA_TRY(resid_gemm(L.cout, L.cout_b, pf.atd, a32));
    if (m->abi_ffn()) {
      WA_WQ4(wq4_layernorm(pf.x, L.ln3_w, L.ln3_b, rows, D, WQ4_PREC_F16X2, nullptr, pf.hid, st));
      WA_WQ4(wq4_ffn_forward_ws(L.fc1, L.fc1_b, L.fc2, L.fc2_b, pf.hid, pf.x, pf.x, rows, WQ4_EPI_RESIDUAL, m->prec,
                                ffn_ws, ffn_ws_bytes, st));
      continue;
    }
    WA_TRY(ln_gemm(L.fc1, L.fc1_b, L.ln3_w, L.ln3_b, nullptr, pf.atf, WQ4_EPI_GELU | WQ4_EPI_TILED_OUT));
    WA_TRY(resid_gemm(L.fc2, L.fc2_b, pf.atf, nullptr));
  }
  *P_out = P;
  if (call.align) return WQ4_OK;  // the capture is all an alignment call takes from the pass
  // final LN; the logits of every clip's last row (right-aligned: row P - 1)
  WA_WQ4(wq4_layernorm(pf.x, m->dln_w, m->dln_b, rows, D, WQ4_PREC_F16X2, nullptr, pf.hid, st));
  WA_HIP(launch_logits(pf.hid + (size_t)(P - 1) * D, B, D, (int64_t)P * D, m->tok_emb, V, g.logits, st));
  if (call.score) {
    // the SOT rows, gathered into g.hid (a clip without SOT: its last row, the score overwritten below)
    for (int b = 0; b < B; ++b) {
      const int r = sot_row[b] < 0 ? P - 1 : sot_row[b];
      WA_HIP(hipMemcpyAsync(g.hid + (size_t)b * D, pf.hid + ((size_t)b * P + r) * D, (size_t)D * 4,
                            hipMemcpyDeviceToDevice, st));
    }
    WA_HIP(launch_logits(g.hid, B, D, D, m->tok_emb, V, g.z0, st));
    // the language ids through lang_tok (an id outside the language range: NaN)
    WA_HIP(hipMemcpyAsync(g.lang_tok, lang.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    WA_TRY(score_sot(m, g, g.z0, g.lang_tok, 1, 0, st));
    const float nan = std::nanf("");
    for (int b = 0; b < B; ++b)
      if (sot_row[b] < 0) WA_HIP(hipMemcpyAsync(g.no_speech + b, &nan, 4, hipMemcpyHostToDevice, st));
  }
  return WQ4_OK;
}

}  // namespace wa

extern "C" {

wq4_status wa_prompt_check(const wa_prompt* p, int n_clips, int n_vocab, int n_text_ctx, int max_tokens) {
  if (!p || !p->tokens || !p->n_tokens) return fail(WQ4_EINVAL, "null prompt");
  if (n_clips < 1 || n_vocab < 1 || n_text_ctx < 1 || max_tokens < 0) return fail(WQ4_EINVAL, "bad sizes");
  if (p->ld < 1) return fail(WQ4_EINVAL, "prompt ld must be >= 1");
  int longest = 0;
  for (int c = 0; c < n_clips; ++c) {
    const int n = p->n_tokens[c];
    if (n < 1 || n > p->ld) return fail(WQ4_EINVAL, "every prompt has 1 .. ld tokens");
    for (int i = 0; i < n; ++i) {
      const int32_t t = p->tokens[(size_t)c * p->ld + i];
      if (t < 0 || t >= n_vocab) return fail(WQ4_EINVAL, "prompt token id outside [0, n_vocab)");
    }
    longest = std::max(longest, n);
  }
  if (longest + max_tokens > n_text_ctx)
    return fail(WQ4_EINVAL, "the longest prompt + max_tokens must not exceed n_text_ctx");
  return WQ4_OK;
}

wq4_status wa_transcribe_prompted(wa_model* m, const float* mel_dev, int n_clips, const wa_prompt* prompt,
                                  int max_tokens, int eot_stop, const wa_sampling* sampling, int32_t* tokens_out,
                                  int32_t* n_tokens_out, const wa_scores* scores, void* stream) {
  const bool ok = mel_dev && tokens_out && n_tokens_out && prompt && (!sampling || (sampling->temperature && sampling->seed));
  WA_TRY(check_args(m, ok, 1, max_tokens, n_clips, ok && sampling ? sampling->temperature : nullptr));
  WA_TRY(check_prompt(m, prompt, n_clips, max_tokens));
  DecodeCall call = sampling ? DecodeCall(-1, max_tokens, eot_stop, true, sampling->timestamps != 0,
                                          sampling->max_initial, true)
                                   .with_clips(sampling->temperature, sampling->seed, nullptr)
                             : DecodeCall(-1, max_tokens, eot_stop, scores != nullptr);
  call.prompt = prompt;
  WA_TRY(prepare_call(m, call));
  WA_TRY(ensure_prefill(m));
  return transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, scores);
}

wq4_status wa_transcribe_fallback_prompted(wa_model* m, const float* mel_dev, int n_clips, const wa_prompt* prompt,
                                           int max_tokens, int eot_stop, const wa_fallback* fb, int32_t* tokens_out,
                                           int32_t* n_tokens_out, const wa_scores* scores, int32_t* rung_out,
                                           void* stream) {
  const bool ok = mel_dev && tokens_out && n_tokens_out && prompt && fb && fb->temperatures && fb->seed;
  WA_TRY(check_args(m, ok, 1, max_tokens, n_clips, ok ? fb->temperatures : nullptr, ok ? &fb->n_temperatures : nullptr));
  WA_TRY(check_prompt(m, prompt, n_clips, max_tokens));
  DecodeCall call(-1, max_tokens, eot_stop, true, fb->timestamps != 0, fb->max_initial, true);
  call.prompt = prompt;
  WA_TRY(prepare_call(m, call));
  WA_TRY(ensure_prefill(m));
  return transcribe_ladder(m, call, mel_dev, n_clips, fb, tokens_out, n_tokens_out, scores, rung_out, stream);
}

wq4_status wa_prompt_logits_ragged(wa_model* m, const wa_prompt* prompt, int n_clips, float* logits_dev,
                                   void* stream) {
  if (!m || !prompt || !logits_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > m->bmax) return fail(WQ4_EINVAL, "n_clips out of range");
  WA_TRY(check_prompt(m, prompt, n_clips, 0));
  if (n_clips > m->kv_batch) return fail(WQ4_EINVAL, "wa_encode the clips first");
  WA_HIP(hipSetDevice(m->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  DecGroup& g = m->groups[0];
  g.lane = 0;
  g.b0 = 0;
  g.nb = n_clips;
  g.clip0 = 0;
  DecodeCall call;
  call.prompt = prompt;
  int P = 0;
  WA_TRY(prefill_group(m, g, call, st, &P));
  WA_HIP(hipMemcpyAsync(logits_dev, g.logits, (size_t)n_clips * m->cfg.n_vocab * 4, hipMemcpyDeviceToDevice, st));
  WA_HIP(hipStreamSynchronize(st));
  return WQ4_OK;
}

}  // extern "C"
