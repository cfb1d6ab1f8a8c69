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

wq4_status wa_transcribe_long(wa_model* m, const float* audio_dev, int n_streams, const int64_t* offset,
                              const int64_t* n_samples, const wa_long_options* o, wa_long_result** out, void* stream) {
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

  const int S = n_streams, T = o->max_tokens, n_mels = m->cfg.n_mels, ts0 = m->ts0();
  const size_t slots = (size_t)T + 1;
  const int bmax = std::min(m->bmax, S);
  // every round's ladder: sampled, with timestamps, stopping at EOT
  const DecodeCall call(o->lang_token, T, 1, true, true, o->max_initial, true);
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
  std::vector<float> lp((size_t)bmax * slots), ns(bmax), lpr(bmax);
  const wa_scores scores{lp.data(), ns.data(), lt.data(), lpr.data()};
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
    WA_TRY(prepare_call(m, call));  // the first round allocates the mode's buffers
    WA_TRY(transcribe_ladder(m, call, mel_dev, B, &fb, tok.data(), nt.data(), &scores, rung.data(), stream));
    for (int i = 0; i < 5; ++i) sums[i] += m->timings[i];
    for (int c = 0; c < B; ++c) {
      const int r = rec[c];
      wa_long_result::Stream& rs = res->streams[r];
      wa_long_result::Window win;
      const int32_t* toks = tok.data() + (size_t)c * T;
      const float* lps = lp.data() + c * slots;
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
