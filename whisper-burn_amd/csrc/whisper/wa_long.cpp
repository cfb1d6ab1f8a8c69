// wa_long.cpp -- long-form transcription (wa_transcribe_long): OpenAI
// transcribe.py's seek-driven loop over many recordings at once, its host
// rules (wa_long_advance, wa_long_round) and the result handle.  The windows
// come from wa_long_mel_max / wa_long_mel_windows (wa_mel.hip), every round's
// batch goes through the ladder of wa_transcribe_fallback (transcribe_ladder).
#include <cmath>

#include "wa_mel.hpp"
#include "wa_model.hpp"

using namespace wa;

struct wa_long_result {
  struct Window {
    wa_long_window w;
    std::vector<int32_t> tokens;  // n_tokens
    std::vector<float> logprob;   // max_tokens + 1 slots
    int prompt_len = 0;           // previous-text tokens in the window's prompt (wa_transcribe_long_prompted)
  };
  struct Stream {
    std::vector<Window> windows;
    std::vector<wa_long_segment> segments;
    bool truncated = false;
  };
  int max_tokens = 0;
  std::vector<Stream> streams;
};

namespace {

// content frames of a recording (C); at most 2^31 - 3002 (the entries check n_samples)
int32_t content_frames(int64_t n_samples) { return (int32_t)(n_samples / kMelHop); }

// room in a caller's array: the count is always written, too little room is an error
template <class T>
wq4_status copy_out(const std::vector<T>& v, T* out, int cap, int* n, const char* what) {
  *n = (int)v.size();
  if ((int)v.size() > cap) return fail(WQ4_EINVAL, std::string(what) + " too small: the count written is needed");
  std::copy(v.begin(), v.end(), out);
  return WQ4_OK;
}

const wa_long_result::Stream* stream_of(const wa_long_result* r, int stream) {
  return r && stream >= 0 && stream < (int)r->streams.size() ? &r->streams[stream] : nullptr;
}

}  // namespace

extern "C" {

wq4_status wa_long_advance(const int32_t* tokens, int n, int ts0, int size, float no_speech_prob, double avg_logprob,
                           float logprob_threshold, float no_speech_threshold, int* skipped, int* advance) {
  if (!skipped || !advance || n < 0 || (n > 0 && !tokens)) return fail(WQ4_EINVAL, "bad arguments");
  if (size < 1 || size > kMelFrames) return fail(WQ4_EINVAL, "size must be in [1, 3000]");
  const bool rescued = !std::isnan(logprob_threshold) && avg_logprob > (double)logprob_threshold;
  const bool skip = !std::isnan(no_speech_threshold) && no_speech_prob > no_speech_threshold && !rescued;
  int adv = size;
  if (!skip) {
    int n_segs = 0, seek_frames = 0;
    std::vector<wa_segment> segs(std::max(1, n));  // a window of n tokens has at most n segments
    WA_TRY(wa_segments_from_tokens(tokens, n, ts0, segs.data(), (int)segs.size(), &n_segs, &seek_frames));
    adv = std::min(seek_frames, size);
    if (adv < 1) adv = size;  // OpenAI's loop would not advance (<|0.00|> a <|0.00|><|0.00|>)
  }
  *skipped = skip ? 1 : 0;
  *advance = adv;
  return WQ4_OK;
}

wq4_status wa_long_round(const int32_t* content, const int32_t* seek, const int32_t* windows, int n_streams,
                         int max_batch, int max_windows, int* streams_out, int* n_out) {
  if (!content || !seek || !windows || !streams_out || !n_out) return fail(WQ4_EINVAL, "null argument");
  if (n_streams < 1 || max_batch < 1 || max_windows < 1)
    return fail(WQ4_EINVAL, "n_streams, max_batch and max_windows must be >= 1");
  int n = 0;
  for (int r = 0; r < n_streams && n < max_batch; ++r)
    if (seek[r] < content[r] && windows[r] < max_windows) streams_out[n++] = r;
  *n_out = n;
  return WQ4_OK;
}

wq4_status wa_long_prompt_window(const int32_t* prev, int n_prev, int reset, int n_text_ctx, int max_tokens,
                                 int startofprev, int lang_token, int task_token, int32_t* prompt, int cap, int* n,
                                 int* k_out) {
  if (!n || !k_out || n_prev < 0 || (n_prev > 0 && !prev) || reset < 0 || reset > n_prev || cap < 0 ||
      (cap > 0 && !prompt))
    return fail(WQ4_EINVAL, "bad arguments");
  if (n_text_ctx < 8 || max_tokens < 1 || max_tokens > n_text_ctx - 4)
    return fail(WQ4_EINVAL, "need n_text_ctx >= 8 and max_tokens in [1, n_text_ctx - 4]");
  const int k = std::max(0, std::min({n_prev - reset, n_text_ctx / 2 - 1, n_text_ctx - 4 - max_tokens}));
  std::vector<int32_t> p;
  if (k > 0) {
    p.push_back(startofprev);
    p.insert(p.end(), prev + n_prev - k, prev + n_prev);
  }
  p.insert(p.end(), {50258, lang_token, task_token});
  *k_out = k;
  return copy_out(p, prompt, cap, n, "prompt");
}

wq4_status wa_long_prompt_next(int32_t* prev, int* n_prev, int* reset, const int32_t* tokens, int n, int ts0,
                               int skipped, float temperature, int condition_on_previous_text,
                               float reset_temperature) {
  if (!n_prev || !reset || *n_prev < 0 || n < 0 || (n > 0 && !tokens) || (*n_prev + n > 0 && !prev))
    return fail(WQ4_EINVAL, "bad arguments");
  if (skipped) return WQ4_OK;
  int n_segs = 0, seek_frames = 0;
  std::vector<wa_segment> segs(std::max(1, n));
  WA_TRY(wa_segments_from_tokens(tokens, n, ts0, segs.data(), (int)segs.size(), &n_segs, &seek_frames));
  for (int i = 0; i < n_segs; ++i)
    for (int t = segs[i].tok_begin; t < segs[i].tok_end; ++t) prev[(*n_prev)++] = tokens[t];
  if (!condition_on_previous_text || temperature > reset_temperature) *reset = *n_prev;
  return WQ4_OK;
}

// wa_transcribe_long; lp non-null: with the prompt handling of wa_transcribe_long_prompted.
static wq4_status long_run(wa_model* m, const float* audio_dev, int n_streams, const int64_t* offset,
                           const int64_t* n_samples, const wa_long_options* o, const wa_long_prompt* lp,
                           wa_long_result** out, void* stream) {
  if (out) *out = nullptr;
  if (!m || !audio_dev || !offset || !n_samples || !o || !out || !o->temperatures || !o->seed)
    return fail(WQ4_EINVAL, "null argument");
  if (n_streams < 1) return fail(WQ4_EINVAL, "n_streams must be >= 1");
  if (o->max_tokens < 1 || o->max_tokens > kMaxTokens) return fail(WQ4_EINVAL, "max_tokens must be in [1, 224]");
  if (o->max_windows < 1) return fail(WQ4_EINVAL, "max_windows must be >= 1");
  if (o->n_temperatures < 1 || o->n_temperatures > 8) return fail(WQ4_EINVAL, "the ladder has 1 .. 8 rungs");
  if (bad_temperatures(o->temperatures, o->n_temperatures))
    return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  for (int r = 0; r < n_streams; ++r)
    if (offset[r] < 0 || n_samples[r] < 0 || n_samples[r] >= kMelLongMaxSamples)
      return fail(WQ4_EINVAL, "need offset >= 0 and 0 <= n_samples < 160 * (2^31 - 3001)");
  const int ctx = m->cfg.n_text_ctx, V = m->cfg.n_vocab;
  if (lp) {
    if (o->lang_token < 0 || o->lang_token >= V)
      return fail(WQ4_EINVAL, "a prompted long-form call needs lang_token in [0, n_vocab)");
    if (lp->ld < 0 || (lp->ld > 0 && (!lp->initial || !lp->n_initial))) return fail(WQ4_EINVAL, "bad initial prompts");
    if (!std::isfinite(lp->reset_temperature)) return fail(WQ4_EINVAL, "reset_temperature must be finite");
    if (o->max_tokens > ctx - 4) return fail(WQ4_EINVAL, "max_tokens + the 3-token prompt must fit n_text_ctx");
    for (int r = 0; lp->ld > 0 && r < n_streams; ++r) {
      if (lp->n_initial[r] < 0 || lp->n_initial[r] > lp->ld) return fail(WQ4_EINVAL, "n_initial must be in [0, ld]");
      for (int i = 0; i < lp->n_initial[r]; ++i)
        if (lp->initial[(size_t)r * lp->ld + i] < 0 || lp->initial[(size_t)r * lp->ld + i] >= V)
          return fail(WQ4_EINVAL, "initial prompt token id outside [0, n_vocab)");
    }
  }

  const int S = n_streams, T = o->max_tokens, n_mels = m->cfg.n_mels, ts0 = m->ts0();
  const size_t slots = (size_t)T + 1;
  const int bmax = std::min(m->bmax, S);
  // every round's ladder: sampled, with timestamps, stopping at EOT
  DecodeCall call(o->lang_token, T, 1, true, true, o->max_initial, true);
  // the recordings' previous text and reset marks, and one round's prompts
  // ([startofprev] + at most ctx / 2 - 1 ids + [SOT, lang, TRANSCRIBE])
  const int pld = ctx / 2 + 3;
  std::vector<std::vector<int32_t>> prev(lp ? S : 0);
  std::vector<int> reset(S, 0);
  for (int r = 0; lp && lp->ld > 0 && r < S; ++r)
    prev[r].assign(lp->initial + (size_t)r * lp->ld, lp->initial + (size_t)r * lp->ld + lp->n_initial[r]);
  std::vector<int32_t> p_tok(lp ? (size_t)std::min(m->bmax, S) * pld : 0), p_n(lp ? std::min(m->bmax, S) : 0);
  std::vector<int> p_k(std::min(m->bmax, S), 0);
  const wa_prompt round_prompt{p_tok.data(), p_n.data(), pld};
  if (lp) call.prompt = &round_prompt;
  WA_HIP(hipSetDevice(m->device));
  Dev d;
  float* max_dev = d.alloc<float>(S);
  float* mel_dev = d.alloc<float>((size_t)bmax * n_mels * kMelFrames);
  if (!max_dev || !mel_dev) return fail(WQ4_ENOMEM, "allocation failed");
  WA_TRY(wa_long_mel_max(m->device, audio_dev, S, offset, n_samples, n_mels, max_dev, stream));

  std::unique_ptr<wa_long_result> res(new wa_long_result);
  res->max_tokens = T;
  res->streams.resize(S);
  std::vector<int32_t> content(S), seek(S, 0), nwin(S, 0);
  for (int r = 0; r < S; ++r) content[r] = content_frames(n_samples[r]);
  // one round's batch: the clips' recordings and windows, and the ladder's results
  std::vector<int> rec(bmax);
  std::vector<int64_t> c_off(bmax), c_n(bmax);
  std::vector<int32_t> c_seek(bmax), c_max(bmax), tok((size_t)bmax * T), nt(bmax), lt(bmax), rung(bmax);
  std::vector<uint64_t> c_seed(bmax);
  std::vector<float> lpv((size_t)bmax * slots), ns(bmax), lpr(bmax);
  const wa_scores scores{lpv.data(), ns.data(), lt.data(), lpr.data()};
  wa_fallback fb{};
  fb.temperatures = o->temperatures;
  fb.n_temperatures = o->n_temperatures;
  fb.logprob_threshold = o->logprob_threshold;
  fb.no_speech_threshold = o->no_speech_threshold;
  fb.seed = c_seed.data();  // (timestamps and max_initial: the call's)
  std::vector<wa_segment> segs(T);
  float sums[5] = {0, 0, 0, 0, 0};
  for (;;) {
    int B = 0;
    WA_TRY(wa_long_round(content.data(), seek.data(), nwin.data(), S, bmax, o->max_windows, rec.data(), &B));
    if (B == 0) break;
    for (int c = 0; c < B; ++c) {
      const int r = rec[c];
      c_off[c] = offset[r];
      c_n[c] = n_samples[r];
      c_seek[c] = seek[r];
      c_max[c] = r;
      c_seed[c] = o->seed[r] + 8ull * (uint64_t)nwin[r];
    }
    WA_TRY(wa_long_mel_windows(m->device, audio_dev, B, c_off.data(), c_n.data(), c_seek.data(), c_max.data(),
                               max_dev, n_mels, mel_dev, stream));
    for (int c = 0; lp && c < B; ++c) {
      const int r = rec[c];
      int n = 0;
      WA_TRY(wa_long_prompt_window(prev[r].data(), (int)prev[r].size(), reset[r], ctx, T,
                                   m->cfg.no_timestamps_token() - 2, o->lang_token, m->cfg.transcribe_token(),
                                   p_tok.data() + (size_t)c * pld, pld, &n, &p_k[c]));
      p_n[c] = n;
    }
    WA_TRY(prepare_call(m, call));  // the first round allocates the mode's buffers
    if (lp) WA_TRY(ensure_prefill(m));
    WA_TRY(transcribe_ladder(m, call, mel_dev, B, &fb, tok.data(), nt.data(), &scores, rung.data(), stream));
    for (int i = 0; i < 5; ++i) sums[i] += m->timings[i];
    for (int c = 0; c < B; ++c) {
      const int r = rec[c];
      wa_long_result::Stream& rs = res->streams[r];
      wa_long_result::Window win;
      const int32_t* toks = tok.data() + (size_t)c * T;
      const float* lps = lpv.data() + c * slots;
      double sum = 0.0;
      int cnt = 0;
      for (size_t i = 0; i < slots; ++i)
        if (!std::isnan(lps[i])) {
          sum += lps[i];
          ++cnt;
        }
      wa_long_window& w = win.w;
      w.stream = r;
      w.index = nwin[r];
      w.seek = seek[r];
      w.size = std::min(kMelFrames, content[r] - seek[r]);
      w.rung = rung[c];
      w.lang_token = lt[c];
      w.n_tokens = nt[c];
      w.temperature = o->temperatures[rung[c]];
      w.no_speech_prob = ns[c];
      w.lang_prob = lpr[c];
      w.avg_logprob = cnt ? sum / cnt : 0.0;
      int skipped = 0, advance = 0;
      WA_TRY(wa_long_advance(toks, nt[c], ts0, w.size, ns[c], w.avg_logprob, o->logprob_threshold,
                             o->no_speech_threshold, &skipped, &advance));
      w.skipped = skipped;
      w.advance = advance;
      if (!skipped) {
        int n_segs = 0, seek_frames = 0;
        WA_TRY(wa_segments_from_tokens(toks, nt[c], ts0, segs.data(), (int)segs.size(), &n_segs, &seek_frames));
        for (int i = 0; i < n_segs; ++i)
          rs.segments.push_back(wa_long_segment{r, w.index, segs[i].tok_begin, segs[i].tok_end,
                                                w.seek * 0.01 + (double)segs[i].start_s,
                                                w.seek * 0.01 + (double)segs[i].end_s});
      }
      if (lp) {
        std::vector<int32_t>& pv = prev[r];
        int np = (int)pv.size();
        pv.resize((size_t)np + nt[c]);
        WA_TRY(wa_long_prompt_next(pv.data(), &np, &reset[r], toks, nt[c], ts0, skipped, w.temperature,
                                   lp->condition_on_previous_text, lp->reset_temperature));
        pv.resize(np);
        win.prompt_len = p_k[c];
      }
      win.tokens.assign(toks, toks + nt[c]);
      win.logprob.assign(lps, lps + slots);
      rs.windows.push_back(std::move(win));
      seek[r] += advance;
      ++nwin[r];
    }
  }
  for (int r = 0; r < S; ++r) res->streams[r].truncated = seek[r] < content[r];
  std::memcpy(m->timings, sums, sizeof(sums));
  *out = res.release();
  return WQ4_OK;
}

wq4_status wa_transcribe_long(wa_model* m, const float* audio_dev, int n_streams, const int64_t* offset,
                              const int64_t* n_samples, const wa_long_options* o, wa_long_result** out, void* stream) {
  return long_run(m, audio_dev, n_streams, offset, n_samples, o, nullptr, out, stream);
}

wq4_status wa_transcribe_long_prompted(wa_model* m, const float* audio_dev, int n_streams, const int64_t* offset,
                                       const int64_t* n_samples, const wa_long_options* o, const wa_long_prompt* lp,
                                       wa_long_result** out, void* stream) {
  // no prompt at all: the existing path (once the prompted call's own arguments are checked)
  bool any = lp && lp->condition_on_previous_text;
  for (int r = 0; lp && !any && lp->ld > 0 && lp->n_initial && r < n_streams; ++r) any = lp->n_initial[r] > 0;
  if (lp && !any && o && o->lang_token < 0) {
    if (out) *out = nullptr;
    return fail(WQ4_EINVAL, "a prompted long-form call needs lang_token >= 0");
  }
  return long_run(m, audio_dev, n_streams, offset, n_samples, o, any ? lp : nullptr, out, stream);
}

wq4_status wa_long_result_prompt_len(const wa_long_result* r, int stream, int index, int* k) {
  const wa_long_result::Stream* s = stream_of(r, stream);
  if (!s || index < 0 || index >= (int)s->windows.size() || !k) return fail(WQ4_EINVAL, "bad arguments");
  *k = s->windows[index].prompt_len;
  return WQ4_OK;
}

void wa_long_result_free(wa_long_result* r) { delete r; }

int wa_long_result_streams(const wa_long_result* r) { return r ? (int)r->streams.size() : 0; }

int wa_long_result_max_tokens(const wa_long_result* r) { return r ? r->max_tokens : 0; }

wq4_status wa_long_result_stream(const wa_long_result* r, int stream, int* n_windows, int* truncated,
                                 int* n_segments) {
  const wa_long_result::Stream* s = stream_of(r, stream);
  if (!s || !n_windows || !truncated || !n_segments) return fail(WQ4_EINVAL, "bad arguments");
  *n_windows = (int)s->windows.size();
  *truncated = s->truncated ? 1 : 0;
  *n_segments = (int)s->segments.size();
  return WQ4_OK;
}

wq4_status wa_long_result_windows(const wa_long_result* r, int stream, wa_long_window* out, int cap, int* n_windows) {
  const wa_long_result::Stream* s = stream_of(r, stream);
  if (!s || !n_windows || cap < 0 || (cap > 0 && !out)) return fail(WQ4_EINVAL, "bad arguments");
  std::vector<wa_long_window> v;
  for (const auto& w : s->windows) v.push_back(w.w);
  return copy_out(v, out, cap, n_windows, "out");
}

wq4_status wa_long_result_window(const wa_long_result* r, int stream, int index, int32_t* tokens, int cap_tokens,
                                 int* n_tokens, float* logprob, int cap_logprob) {
  const wa_long_result::Stream* s = stream_of(r, stream);
  if (!s || index < 0 || index >= (int)s->windows.size() || !n_tokens || cap_tokens < 0)
    return fail(WQ4_EINVAL, "bad arguments");
  const wa_long_result::Window& w = s->windows[index];
  if (logprob && cap_logprob < (int)w.logprob.size())
    return fail(WQ4_EINVAL, "logprob too small: max_tokens + 1 slots are needed");
  if (logprob) std::copy(w.logprob.begin(), w.logprob.end(), logprob);
  if (!tokens) {
    *n_tokens = (int)w.tokens.size();
    return WQ4_OK;
  }
  return copy_out(w.tokens, tokens, cap_tokens, n_tokens, "tokens");
}

wq4_status wa_long_result_segments(const wa_long_result* r, int stream, wa_long_segment* out, int cap,
                                   int* n_segments) {
  const wa_long_result::Stream* s = stream_of(r, stream);
  if (!s || !n_segments || cap < 0 || (cap > 0 && !out)) return fail(WQ4_EINVAL, "bad arguments");
  return copy_out(s->segments, out, cap, n_segments, "out");
}

}  // extern "C"
