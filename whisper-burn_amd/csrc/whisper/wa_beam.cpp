// wa_beam.cpp -- beam-search decoding (wa_transcribe_beam; the semantics:
// include/whisper_amd.h, "Beam search"): the call's buffers, its step graph,
// the decode loop and the host's finalize + rank.
//
// Reference semantics: openai/whisper decoding.py BeamSearchDecoder (update,
// finalize) and MaximumLikelihoodRanker.
//
// A beam call is one decode group on lane 0 whose rows are clip * K + beam.
// The encoder runs over the clips; its last residual stream is then repeated
// per beam row and ln_post, the planes and (few rows) the head-major K / V run
// over the rows, so both cross-attention paths see a batch of `rows` clips and
// run unchanged.  A step is decoder_forward (self-attention through the
// ancestor table, stored logits), beam_topk and beam_select, captured once; the
// host only polls the count of complete clips through the pinned ring.
//
// wa_transcribe_beam_ex adds the two modes of the greedy entries to it: under
// the timestamp rules the rows' rule records (the group's, as in a greedy
// timestamp decode) are read by the rules form of the top-k and follow the
// reindexing in the merge; after caller prompts every row of a clip carries the
// clip's prompt through the group's prefill and the steps run the pad forms.
#include <cmath>

#include "wa_model.hpp"

using namespace wa;

namespace {

struct EventSet {
  std::vector<hipEvent_t> e;
  EventSet() = default;
  EventSet(const EventSet&) = delete;
  EventSet& operator=(const EventSet&) = delete;
  ~EventSet() {
    for (hipEvent_t x : e) (void)hipEventDestroy(x);
  }
  hipError_t make(hipEvent_t* out, bool timing = true) {
    hipError_t r = hipEventCreateWithFlags(out, timing ? hipEventDefault : hipEventDisableTiming);
    if (r == hipSuccess) e.push_back(*out);
    return r;
  }
};

wq4_status check_beam(const wa_beam* b, int n_clips, int max_batch) {
  if (!b) return fail(WQ4_EINVAL, "null argument");
  if (b->beam_size < 1 || b->beam_size > kBeamMaxK) return fail(WQ4_EINVAL, "beam_size must be in [1, 8]");
  if (b->max_candidates < b->beam_size || b->max_candidates > kBeamMaxCand)
    return fail(WQ4_EINVAL, "max_candidates must be in [beam_size, 16]");
  if (n_clips < 1) return fail(WQ4_EINVAL, "n_clips out of range");
  if ((int64_t)n_clips * b->beam_size > max_batch) return fail(WQ4_EINVAL, "n_clips * beam_size exceeds max_batch");
  return WQ4_OK;
}

int rank_best(const float* sum, const int32_t* len, int n, float length_penalty) {
  int best = 0;
  double bs = 0.0;
  for (int i = 0; i < n; ++i) {
    const double l = std::max(1, (int)len[i]);
    const double pen = std::isnan(length_penalty) ? l : std::pow((5.0 + l) / 6.0, (double)length_penalty);
    const double s = (double)sum[i] / pen;
    if (i == 0 || s > bs) {
      best = i;
      bs = s;
    }
  }
  return best;
}

// The beam buffers: allocated by the first beam call, all or nothing.
wq4_status ensure_beam(wa_model* m) {
  wa_model::Beam& b = m->bm;
  if (b.ok) return WQ4_OK;
  const size_t R = (size_t)m->bmax, ctx = (size_t)m->cfg.n_text_ctx, Cn = kBeamMaxCand;
  Dev& d = m->dev;
  b.top_tok = d.alloc<int>(R * kBeamMaxTop);
  b.top_lp = d.alloc<float>(R * kBeamMaxTop);
  b.S = d.alloc<float>(R);
  b.parent = d.alloc<int>(R);
  b.anc = d.alloc<int>(2 * R * ctx);
  b.fed = d.alloc<int>(ctx * R);
  b.fin_sum = d.alloc<float>(R * Cn);
  b.fin_len = d.alloc<int>(R * Cn);
  b.fin_anc = d.alloc<int>(R * Cn * ctx);
  b.fin_n = d.alloc<int>(R);
  b.complete = d.alloc<int>(R);
  b.ticket = d.alloc<int>(1);
  void* all[] = {b.top_tok, b.top_lp, b.S, b.parent, b.anc, b.fed, b.fin_sum, b.fin_len, b.fin_anc, b.fin_n,
                 b.complete, b.ticket};
  bool ok = true;
  for (void* p : all) ok = ok && p;
  if (!ok) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (void* p : all) d.release(p);
    b = wa_model::Beam{};
    return fail(WQ4_ENOMEM, "beam buffer allocation failed");
  }
  m->bytes += 4 * (R * (2 * kBeamMaxTop + 4) + 3 * R * ctx + R * Cn * (2 + ctx) + 1);
  b.ok = true;
  return WQ4_OK;
}

// (a timestamp call's rows keep their rule records where a greedy timestamp
// decode keeps its clips': the group's, reset by prompt_group)
BeamSelect select_args(const wa_model* m, const DecGroup& g, const DecodeCall& call) {
  const wa_model::Beam& b = m->bm;
  return BeamSelect{b.top_tok, b.top_lp,  b.S,       g.next_tok, b.parent,   b.anc,    b.fed,  b.fin_sum,
                    b.fin_len, b.fin_anc, b.fin_n,   b.complete, b.ticket,   g.state,  call.ts ? g.ts_rules : nullptr};
}

// The top-(K + 1) of the group's stored logit rows and the per-clip merge, in
// the call's mode: pick 0 (state null: EOT suppressed, whisper.rs:97-99) or a
// step's (EOT by the state); under the suppress mask of that pick (pick 0: the
// union), if the model has lists.
wq4_status beam_pick(wa_model* m, DecGroup& g, const DecodeCall& call, const DecodeState* state, hipStream_t st) {
  const int V = m->cfg.n_vocab, K = call.beam_k, ts0 = m->ts0();
  const uint32_t* sup = state ? m->sup_mask : m->sup_mask0;
  if (call.ts)
    WA_HIP(launch_beam_topk_rules(g.logits, g.nb, V, V, K + 1, state ? 0 : 1, state ? kMinTokens : 0, call.eot_stop,
                                  state, g.ts_rules, ts0, m->bm.top_tok, m->bm.top_lp, nullptr, m->range_flag, st,
                                  sup));
  else
    WA_HIP(launch_beam_topk(g.logits, g.nb, V, V, K + 1, state ? 0 : 1, state ? kMinTokens : 0, call.eot_stop, state,
                            m->bm.top_tok, m->bm.top_lp, m->range_flag, st, sup));
  WA_HIP(launch_beam_select(select_args(m, g, call), g.nb / K, K, call.beam_c, m->cfg.n_text_ctx, st, ts0, V));
  return WQ4_OK;
}

// One beam step on `st`: the decoder pass over the rows' last tokens, the
// top-(K + 1) of every stored logit row, the per-clip merge (which advances
// the state for the next step).
wq4_status beam_step(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st) {
  WA_TRY(decoder_forward(m, g, call, g.next_tok, 1, g.state, 0, 0, st));
  return beam_pick(m, g, call, g.state, st);
}

// The beam step graph of group g: everything the capture bakes in is the key.
wq4_status ensure_beam_graph(wa_model* m, DecGroup& g, const DecodeCall& call) {
  constexpr int kKey = sizeof(g.beam_key) / sizeof(g.beam_key[0]);
  const int key[kKey] = {call.beam_k,   call.beam_c,            g.nb,           call.eot_stop ? 1 : 0,
                         m->range_tier, m->group_kv(g) ? 1 : 0, g.xplan.splits, g.xres.q,
                         call.ts ? 1 : 0, call.prompt ? 1 : 0};
  if (g.beam_graph && std::equal(key, key + kKey, g.beam_key)) return WQ4_OK;
  if (g.beam_graph) {
    (void)hipGraphExecDestroy(g.beam_graph);
    g.beam_graph = nullptr;
  }
  WA_WQ4(wq4_prepare_stream(m->device, g.st));  // split-K workspace exists before capture
  hipGraph_t gr;
  WA_HIP(hipStreamBeginCapture(g.st, hipStreamCaptureModeThreadLocal));
  wq4_status s = beam_step(m, g, call, g.st);
  hipError_t ce = hipStreamEndCapture(g.st, &gr);
  if (s != WQ4_OK) return s;
  if (ce != hipSuccess) return fail(WQ4_EHIP, std::string("graph capture: ") + hipGetErrorString(ce));
  ce = hipGraphInstantiate(&g.beam_graph, gr, nullptr, nullptr, 0);
  (void)hipGraphDestroy(gr);
  if (ce != hipSuccess) return fail(WQ4_EHIP, std::string("graph instantiate: ") + hipGetErrorString(ce));
  std::copy(key, key + kKey, g.beam_key);
  return WQ4_OK;
}

// What one run leaves on the host: per clip the candidate list (finished
// first, then the live beams finalize added), at most C entries.
struct Candidates {
  std::vector<std::vector<int32_t>> tokens;
  std::vector<float> sum;
};

// One beam transcribe at the model's range tier; *overflow = its range flag.
wq4_status beam_once(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips, void* stream,
                     bool* overflow, std::vector<Candidates>& out, const wa_scores* scores) {
  hipStream_t st = m->own_stream;
  const Config& c = m->cfg;
  const int K = call.beam_k, C = call.beam_c, rows = n_clips * K, ctx = c.n_text_ctx;
  const int T = c.n_audio_ctx, D = c.n_audio_state;
  wa_model::Beam& bm = m->bm;
  DecGroup& g = m->groups[0];
  EventSet ev;
  hipEvent_t e_in, e_enc, e_kv, e_ready, e_prompt, e_done, e_end;
  for (hipEvent_t* e : {&e_in, &e_enc, &e_kv, &e_ready, &e_prompt, &e_done, &e_end}) WA_HIP(ev.make(e));
  WA_HIP(hipEventRecord(e_in, static_cast<hipStream_t>(stream)));
  WA_HIP(hipStreamWaitEvent(st, e_in, 0));
  WA_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(int), st));
  WA_HIP(hipEventRecord(e_enc, st));
  WA_TRY(encoder_front(m, mel_dev, n_clips, st));
  WA_TRY(encoder_layers(m, n_clips, 0, (int)m->enc.size(), st));
  WA_HIP(hipEventRecord(e_kv, st));
  // clip r / K's residual stream at row r, last row first: a row's source is
  // never behind a row already written (m->x holds bmax >= rows clips)
  const size_t clip_floats = (size_t)T * D;
  for (int r = rows - 1; r > 0; --r)
    if (r / K != r)
      WA_HIP(hipMemcpyAsync(m->x + r * clip_floats, m->x + (r / K) * clip_floats, clip_floats * 4,
                            hipMemcpyDeviceToDevice, st));
  WA_TRY(encoder_post(m, rows, st, nullptr));
  WA_TRY(cross_kv_forward(m, rows, st, true));
  WA_HIP(hipEventRecord(e_ready, st));

  // the decode group: all rows on lane 0, nothing beside it
  if (m->dev_cus <= 0) WA_HIP(hipDeviceGetAttribute(&m->dev_cus, hipDeviceAttributeMultiprocessorCount, m->device));
  g.xres = xattn_residency(rows, T, m->ns, D);
  g.xplan = xattn_plan(T, rows, std::max(1, m->dev_cus));
  g.lane = 0;
  g.b0 = 0;
  g.nb = rows;
  g.clip0 = 0;
  hipStream_t gs = g.st;
  WA_HIP(hipStreamWaitEvent(gs, e_ready, 0));
  WA_TRY(prompt_group(m, g, call, gs));  // the prompt's logits in g.logits, the state one step before the first
  // S = [0, -inf, ...] per clip; both tables the identity; nothing fed, nothing finished (pageable: staged)
  std::vector<float> s0(rows, -INFINITY);
  for (int cl = 0; cl < n_clips; ++cl) s0[(size_t)cl * K] = 0.0f;
  std::vector<int> ident((size_t)rows * ctx);
  for (int r = 0; r < rows; ++r) std::fill(ident.begin() + (size_t)r * ctx, ident.begin() + (size_t)(r + 1) * ctx, r);
  WA_HIP(hipMemcpyAsync(bm.S, s0.data(), (size_t)rows * 4, hipMemcpyHostToDevice, gs));
  for (int t = 0; t < 2; ++t)
    WA_HIP(hipMemcpyAsync(bm.anc + (size_t)t * rows * ctx, ident.data(), ident.size() * 4, hipMemcpyHostToDevice, gs));
  WA_HIP(hipMemsetAsync(bm.fed, 0, (size_t)ctx * rows * 4, gs));
  WA_HIP(hipMemsetAsync(bm.fin_n, 0, (size_t)n_clips * 4, gs));
  WA_HIP(hipMemsetAsync(bm.complete, 0, (size_t)n_clips * 4, gs));
  WA_HIP(hipMemsetAsync(bm.ticket, 0, sizeof(int), gs));
  // pick 0: EOT suppressed (whisper.rs:97-99), then the first merge
  WA_TRY(beam_pick(m, g, call, nullptr, gs));
  WA_HIP(hipEventRecord(e_prompt, gs));
  WA_TRY(ensure_beam_graph(m, g, call));

  // picks 1 .. max_tokens - 1; stops early once every clip is complete (polled with a lag)
  hipEvent_t ring[8];
  if (call.eot_stop)
    for (auto& e : ring) WA_HIP(ev.make(&e, false));
  const int lag = 4;
  int steps = 0;
  for (int step = 0; step + 1 < call.max_tokens; ++step) {
    WA_HIP(hipGraphLaunch(g.beam_graph, gs));
    ++steps;
    if (!call.eot_stop) continue;
    const int slot = step % 8;
    WA_HIP(hipMemcpyAsync(&g.host_ndone[slot], &g.state->n_done, sizeof(int), hipMemcpyDeviceToHost, gs));
    WA_HIP(hipEventRecord(ring[slot], gs));
    if (step >= lag) {
      const int old = (step - lag) % 8;
      WA_HIP(hipEventSynchronize(ring[old]));
      if (g.host_ndone[old] >= n_clips) break;
    }
  }
  WA_HIP(hipEventRecord(e_done, gs));
  WA_HIP(hipStreamWaitEvent(st, e_done, 0));

  // collect
  DecodeState fin_state{};
  std::vector<int> anc(2 * (size_t)rows * ctx), fed((size_t)ctx * rows), fin_len((size_t)n_clips * C),
      fin_anc((size_t)n_clips * C * ctx), fin_n(n_clips);
  std::vector<float> S(rows), fin_sum((size_t)n_clips * C), sc_ns(rows), sc_lp(rows);
  std::vector<int> sc_lt(rows);
  int flag = 0;
  WA_HIP(hipMemcpyAsync(&fin_state, g.state, sizeof(fin_state), hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(anc.data(), bm.anc, anc.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(fed.data(), bm.fed, fed.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(S.data(), bm.S, S.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(fin_sum.data(), bm.fin_sum, fin_sum.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(fin_len.data(), bm.fin_len, fin_len.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(fin_anc.data(), bm.fin_anc, fin_anc.size() * 4, hipMemcpyDeviceToHost, st));
  WA_HIP(hipMemcpyAsync(fin_n.data(), bm.fin_n, fin_n.size() * 4, hipMemcpyDeviceToHost, st));
  if (scores) {
    WA_HIP(hipMemcpyAsync(sc_ns.data(), g.no_speech, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    WA_HIP(hipMemcpyAsync(sc_lt.data(), g.lang_tok, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    WA_HIP(hipMemcpyAsync(sc_lp.data(), g.lang_prob, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
  }
  WA_HIP(hipMemcpyAsync(&flag, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  WA_HIP(hipEventRecord(e_end, st));
  WA_HIP(hipStreamSynchronize(st));
  *overflow = flag != 0;
  float t_enc = 0, t_kv = 0, t_p = 0, t_all = 0;
  WA_HIP(hipEventElapsedTime(&t_enc, e_enc, e_kv));
  WA_HIP(hipEventElapsedTime(&t_kv, e_kv, e_ready));
  WA_HIP(hipEventElapsedTime(&t_p, e_ready, e_prompt));
  WA_HIP(hipEventElapsedTime(&t_all, e_ready, e_end));
  m->timings[0] = t_enc;
  m->timings[1] = t_kv;
  m->timings[2] = t_p;
  m->timings[3] = t_all - t_p;
  m->timings[4] = (float)steps;
  if (*overflow) return WQ4_OK;

  // Finalize.  The merge ran steps + 1 times; the token of pick p was fed at
  // cache slot kv0 + p by the row the sequence's ancestor table names there.
  const int picks = steps + 1, kv0 = fin_state.kv_len - steps;
  const int* live = anc.data() + (size_t)((fin_state.step + 1) & 1) * rows * ctx;
  out.assign(n_clips, Candidates{});
  for (int cl = 0; cl < n_clips; ++cl) {
    Candidates& cd = out[cl];
    auto add = [&](const int* table, int len, float sum) {
      std::vector<int32_t> t(len);
      for (int p = 0; p < len; ++p) t[p] = fed[(size_t)(kv0 + p) * rows + table[kv0 + p]];
      cd.tokens.push_back(std::move(t));
      cd.sum.push_back(sum);
    };
    for (int e = 0; e < fin_n[cl]; ++e) {
      const size_t f = (size_t)cl * C + e;
      add(fin_anc.data() + f * ctx, fin_len[f], fin_sum[f]);
    }
    // fewer than K finished: the live beams, S descending then index ascending (dead ones, S = -inf, never)
    std::vector<int> order;
    for (int j = 0; j < K; ++j)
      if (S[(size_t)cl * K + j] > -INFINITY) order.push_back(j);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return S[(size_t)cl * K + a] > S[(size_t)cl * K + b]; });
    for (size_t i = 0; i < order.size() && (int)cd.sum.size() < K; ++i) {
      const int r = cl * K + order[i];
      add(live + (size_t)r * ctx, picks, S[r]);
    }
    if (scores) {
      const size_t r0 = (size_t)cl * K;
      if (scores->no_speech_prob) scores->no_speech_prob[cl] = sc_ns[r0];
      if (scores->lang_token) scores->lang_token[cl] = sc_lt[r0];
      if (scores->lang_prob) scores->lang_prob[cl] = sc_lp[r0];
    }
  }
  return WQ4_OK;
}

}  // namespace

extern "C" {

wq4_status wa_beam_check(const wa_beam* beam, int n_clips, int max_batch) { return check_beam(beam, n_clips, max_batch); }

wq4_status wa_beam_rank(const float* sum_logprob, const int32_t* n_tokens, int n, float length_penalty,
                        int32_t* best_out) {
  if (!sum_logprob || !n_tokens || !best_out) return fail(WQ4_EINVAL, "null argument");
  if (n < 1) return fail(WQ4_EINVAL, "n must be >= 1");
  *best_out = rank_best(sum_logprob, n_tokens, n, length_penalty);
  return WQ4_OK;
}

wq4_status wa_transcribe_beam(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                              int eot_stop, const wa_beam* beam, int32_t* tokens_out, int32_t* n_tokens_out,
                              const wa_scores* scores, wa_beam_result* result, void* stream) {
  return wa_transcribe_beam_ex(m, mel_dev, n_clips, lang_token, max_tokens, eot_stop, beam, nullptr, tokens_out,
                               n_tokens_out, scores, result, stream);
}

wq4_status wa_transcribe_beam_ex(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                                 int eot_stop, const wa_beam* beam, const wa_beam_options* options,
                                 int32_t* tokens_out, int32_t* n_tokens_out, const wa_scores* scores,
                                 wa_beam_result* result, void* stream) {
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out && beam, 1, max_tokens, n_clips));
  WA_TRY(check_beam(beam, n_clips, m->bmax));
  const wa_prompt* prompt = options ? options->prompt : nullptr;
  if (prompt) WA_TRY(check_prompt(m, prompt, n_clips, max_tokens));
  const bool ts = options && options->timestamps != 0;
  // (a timestamp call is a scored one, like every pick under the rules)
  DecodeCall call(prompt ? -1 : lang_token, max_tokens, eot_stop, scores != nullptr, ts,
                  ts ? options->max_initial : 50);
  call.beam_k = beam->beam_size;
  call.beam_c = beam->max_candidates;
  // clip c's prompt on each of its K rows: the prefill is the group's, over the rows
  const int K = call.beam_k;
  std::vector<int32_t> row_tok, row_n;
  wa_prompt row_prompt{};
  if (prompt) {
    row_tok.resize((size_t)n_clips * K * prompt->ld);
    row_n.resize((size_t)n_clips * K);
    for (int r = 0; r < n_clips * K; ++r) {
      row_n[r] = prompt->n_tokens[r / K];
      std::copy_n(prompt->tokens + (size_t)(r / K) * prompt->ld, prompt->ld, row_tok.begin() + (size_t)r * prompt->ld);
    }
    row_prompt = wa_prompt{row_tok.data(), row_n.data(), prompt->ld};
    call.prompt = &row_prompt;
  }
  WA_TRY(prepare_call(m, call));
  if (prompt) WA_TRY(ensure_prefill(m));
  WA_TRY(ensure_beam(m));
  const int C = call.beam_c;
  std::vector<Candidates> cands;
  for (;;) {  // the range tiers, as transcribe_tiers
    bool overflow = false;
    WA_TRY(beam_once(m, call, mel_dev, n_clips, stream, &overflow, cands, scores));
    if (!overflow) break;
    WA_TRY(raise_tier(m));
  }
  if (result) {
    if (result->cand_tokens) std::memset(result->cand_tokens, 0, (size_t)n_clips * C * max_tokens * 4);
    if (result->cand_n_tokens) std::memset(result->cand_n_tokens, 0, (size_t)n_clips * C * 4);
    if (result->cand_sum_logprob) std::memset(result->cand_sum_logprob, 0, (size_t)n_clips * C * 4);
  }
  for (int cl = 0; cl < n_clips; ++cl) {
    const Candidates& cd = cands[cl];
    const int n = (int)cd.sum.size();
    std::vector<int32_t> len(std::max(n, 1), 0);
    for (int i = 0; i < n; ++i) len[i] = (int32_t)cd.tokens[i].size();
    const int best = n ? rank_best(cd.sum.data(), len.data(), n, beam->length_penalty) : 0;
    std::memset(tokens_out + (size_t)cl * max_tokens, 0, (size_t)max_tokens * 4);
    n_tokens_out[cl] = n ? len[best] : 0;
    if (n) std::memcpy(tokens_out + (size_t)cl * max_tokens, cd.tokens[best].data(), (size_t)len[best] * 4);
    if (!result) continue;
    for (int i = 0; i < n; ++i) {
      const size_t at = (size_t)cl * C + i;
      if (result->cand_tokens)
        std::memcpy(result->cand_tokens + at * max_tokens, cd.tokens[i].data(), (size_t)len[i] * 4);
      if (result->cand_n_tokens) result->cand_n_tokens[at] = len[i];
      if (result->cand_sum_logprob) result->cand_sum_logprob[at] = cd.sum[i];
    }
    if (result->n_candidates) result->n_candidates[cl] = n;
    if (result->best) result->best[cl] = best;
  }
  return WQ4_OK;
}

}  // extern "C"
