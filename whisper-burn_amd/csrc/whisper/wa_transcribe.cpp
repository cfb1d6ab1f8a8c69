// wa_transcribe.cpp -- the transcribe drivers (WhisperModel::transcribe,
// src/model/whisper.rs:51-128): one batch, software-pipelined batches, and
// the range-tier retries around them.
#include <cmath>

#include "wa_model.hpp"

using namespace wa;

namespace {

// Pipelined transcribes (transcribe_pipelined): CUs of the encoder stream
// that runs beside a decode, the encoder layers it covers in the first
// overlapped batch, and the share of the last decode's length its part is
// sized to afterwards (WA_ENC_CUS / WA_ENC_OVERLAP / WA_ENC_FILL override).
// Fill measured at 32 clips (scripts/r05ad.sh): RTF 959 at 0.92, 966 at 0.98
// / 1.0 / 1.02, 948 at 1.04 (the masked part then outlasts the decode);
// 0.98 keeps ~30 ms of slack.
// The masked CUs and the cross-attention's frame split are one decision
// (xattn_plan, run_decode): swept together on the paired bench
// (profiles/split_sweep.json), 32 CUs won -- RTF 1280 with 6 splits beside 32
// CUs against 1273 beside 64, and 1260 / 1255 beside 48 / 64 with the rule's
// 6 splits on all but the last pair.
constexpr int kEncOverlapCUs = 32;
constexpr int kEncOverlapLayers0 = 16;
constexpr double kEncOverlapFill = 0.98;
// CUs an xattn_main launch leaves to the other decode groups of its unit.
// The main holds every CU it lands on for the whole launch, so a main on all
// the CUs the decode has stalls the other group's chain of small GEMMs for
// its length; the main itself is HBM-bound and as fast on fewer CUs.  Paired
// bench, 32-row groups (profiles/split_gate.json, split_sweep.json,
// split_bench_before.json): decode per batch with nothing beside it 626 /
// 608 / 590 ms at 8 / 7 / 6 splits (0 / 32 / 64 CUs left), beside the 32-CU
// masked stream 691 / 653 / 631 / 632 / 632 ms at 8 / 7 / 6 / 5 / 4 (none /
// none / 32 / 64 / 96 left).
constexpr int kXattnPeerCUs = 64;

// HIP events destroyed with the set.
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

// Paired decode (transcribe_pipelined): two consecutive batches of 16 .. 32
// clips decode at once, one decode group per batch, group 1 on the model's
// second lane.  WA_PAIR_BATCHES=0 disables (A/B runs).
// The masked stream keeps its adapted depth beside a paired decode (it
// reaches all L layers of the pair's first batch): at 32-row groups
// xattn_main wants all 256 CUs and the decode slows by about what the hidden
// layers save, but a little is left.  Large-V3 Q4_0, 32 clips, 10 steps,
// three interleaved runs each (profiles/pair_overlap_ab.json): RTF 1146.6 /
// 1146.2 / 1144.1 adapted (decode 721 ms, encoder exposed 106 ms per batch)
// against 1138.0 / 1132.1 / 1134.8 with the conv stem only (673 / 161 ms).
// Three at a time (the width below) from 17 clips on: there a group's
// xattn_main is the HBM-bound 32-row form, and while it streams its planes
// the two other groups walk their chains of small launches, so the planes of
// a third batch fill what a pair leaves of the HBM time (DESIGN.md section
// 10, profiles/lanes_gate.json).  Batches of exactly 16 clips keep the paired
// schedule: their main is the 16-row latency form, which more groups only
// multiply.
constexpr int kPairMinClips = 16, kPairMaxClips = 32;
constexpr int kTripleMinClips = 17;

bool pair_enabled() {
  static const bool enabled = [] {
    const char* e = getenv("WA_PAIR_BATCHES");
    return e ? atoi(e) != 0 : true;
  }();
  return enabled;
}

// Most batches one unit decodes at once: WA_LANES = 1 .. kMaxLanes caps it (A/B runs).
int lanes_cap() {
  static const int cap = [] {
    const char* e = getenv("WA_LANES");
    return e ? std::max(1, std::min(kMaxLanes, atoi(e))) : kMaxLanes;
  }();
  return cap;
}

// Decode groups of one run_decode: one per batch of a unit of n > 1 batches, or one batch's groups.
int unit_groups(int B, int n) { return n > 1 ? n : decode_groups(B); }

// Prompt + greedy loop (whisper.rs:60-125) of every decode group of a batch
// of B clips -- or, n > 1, of a unit of n batches of B clips, group i
// decoding the batch in lane i -- each group's stream first waiting on
// `ready` (the encoder planes).  masked_cus: the CUs of the masked stream
// that runs beside this decode (0: nothing does).  Records gprompt[i] after
// group i's prompt and gdone[i] after its last step, gsteps[i] = the steps it
// ran; the host blocks only for the lagged EOT polls (eot_stop).
// With three groups of 32 rows there is a main to run most of the time: one
// group's xattn_main streams planes while the other two walk their chains on
// the CUs it leaves them (kXattnPeerCUs), so HBM idles less than beside one
// chain (measurements and the sweeps of kXattnPeerCUs and the residency
// budget at three lanes: DESIGN.md section 10).
// batch0: the index, among the call's batches, of the batch in lane 0 -- where
// the groups' clips sit in the call's per-clip host arrays (DecGroup::clip0).
wq4_status run_decode(wa_model* m, const DecodeCall& call, int B, int n, int masked_cus, hipEvent_t ready,
                      const hipEvent_t* gprompt, const hipEvent_t* gdone, int* gsteps, int batch0 = 0) {
  const int eot_stop = call.eot_stop;
  const int G = unit_groups(B, n);
  // the groups decode concurrently: the planes of all their clips are live
  // (every lane of a unit), which decides the share each keeps cached
  const XattnResidency xres = xattn_residency(n * B, m->cfg.n_audio_ctx, m->ns, m->cfg.n_audio_state);
  // one frame split for the unit: its largest group's rows on the CUs a main
  // has -- the device's less the masked stream's and, when other groups decode
  // beside it, what it leaves to them
  if (m->dev_cus <= 0) WA_HIP(hipDeviceGetAttribute(&m->dev_cus, hipDeviceAttributeMultiprocessorCount, m->device));
  const int rows = n > 1 ? B : (B + G - 1) / G;
  const int free_cus = std::max(1, m->dev_cus - masked_cus - (G > 1 ? kXattnPeerCUs : 0));
  const XattnPlan xplan = xattn_plan(m->cfg.n_audio_ctx, rows, free_cus);
  for (int i = 0; i < G; ++i) {
    DecGroup& g = m->groups[i];
    g.xres = xres;
    g.xplan = xplan;
    g.lane = n > 1 ? i : 0;
    g.b0 = n > 1 ? 0 : (int)((int64_t)B * i / G);
    g.nb = n > 1 ? B : (int)((int64_t)B * (i + 1) / G) - g.b0;
    g.clip0 = (batch0 + g.lane) * B + g.b0;
    WA_HIP(hipStreamWaitEvent(g.st, ready, 0));
    // the prefills of a prompted call share one set of activations: one group after another
    if (call.prompt && i > 0) WA_HIP(hipStreamWaitEvent(g.st, gprompt[i - 1], 0));
    WA_TRY(prompt_group(m, g, call, g.st));
    WA_HIP(hipEventRecord(gprompt[i], g.st));
    WA_TRY(ensure_graph(m, g, call));
  }
  // greedy loop (whisper.rs:104-125): each step replays every live group's
  // graph; a group stops once all its clips emitted EOT (polled with a lag)
  EventSet ev;
  hipEvent_t ring[kMaxGroups][8];
  if (eot_stop)
    for (int i = 0; i < G; ++i)
      for (auto& e : ring[i]) WA_HIP(ev.make(&e, false));
  const int lag = 4;
  bool live[kMaxGroups] = {};
  int nlive = G;
  for (int i = 0; i < G; ++i) {
    live[i] = true;
    gsteps[i] = 0;
  }
  for (int step = 0; step < call.max_tokens && nlive > 0; ++step) {
    for (int i = 0; i < G; ++i) {
      if (!live[i]) continue;
      DecGroup& g = m->groups[i];
      WA_HIP(hipGraphLaunch(g.graph, g.st));
      ++gsteps[i];
      if (eot_stop) {
        const int slot = step % 8;
        WA_HIP(hipMemcpyAsync(&g.host_ndone[slot], &g.state->n_done, sizeof(int), hipMemcpyDeviceToHost, g.st));
        WA_HIP(hipEventRecord(ring[i][slot], g.st));
      }
    }
    if (eot_stop && step >= lag) {
      const int old = (step - lag) % 8;
      for (int i = 0; i < G; ++i) {
        if (!live[i]) continue;
        WA_HIP(hipEventSynchronize(ring[i][old]));
        if (m->groups[i].host_ndone[old] >= m->groups[i].nb) {  // every clip had emitted EOT by then
          live[i] = false;
          --nlive;
        }
      }
    }
  }
  // the loop's bookkeeping for tokens chosen by the last step happens at the
  // top of a step that the reference never runs: nothing to add.
  for (int i = 0; i < G; ++i) WA_HIP(hipEventRecord(gdone[i], m->groups[i].st));
  return WQ4_OK;
}

constexpr size_t kLpSlots = kMaxTokens + 1;  // log-probability slots per clip on the device
// staged scores of a batch of B clips: [B][kLpSlots] log-probabilities, then
// [B] no-speech probabilities, [B] language tokens (int32), [B] language probabilities
size_t score_words(int B) { return (size_t)B * (kLpSlots + 3); }

// `st` waits for every group of the run_decode, then copies the groups'
// tokens / counts (kMaxTokens per clip) and the range flag to (pinned) host
// memory: tok / nt / flag of the batch in lane 0; the batch in lane j of a
// unit of n has its own j * lane_stride int32 further on in each.  sc (a
// scored transcribe; null otherwise): the batch's score_words(B) words of
// scores, with the same lane stride.
wq4_status collect_batch(wa_model* m, int B, int n, const hipEvent_t* gdone, hipStream_t st, int32_t* tok,
                         int32_t* nt, int* flag, size_t lane_stride, float* sc = nullptr) {
  const int G = unit_groups(B, n);
  for (int i = 0; i < G; ++i) WA_HIP(hipStreamWaitEvent(st, gdone[i], 0));
  for (int i = 0; i < G; ++i) {
    const DecGroup& g = m->groups[i];
    const size_t ofs = g.lane * lane_stride;
    WA_HIP(hipMemcpyAsync(tok + ofs + (size_t)g.b0 * kMaxTokens, g.tokens, (size_t)g.nb * kMaxTokens * 4,
                          hipMemcpyDeviceToHost, st));
    WA_HIP(hipMemcpyAsync(nt + ofs + g.b0, g.ntok, (size_t)g.nb * 4, hipMemcpyDeviceToHost, st));
    if (sc) {
      float* s = sc + ofs;
      const size_t nb4 = (size_t)g.nb * 4;
      WA_HIP(hipMemcpyAsync(s + (size_t)g.b0 * kLpSlots, g.logprob, nb4 * kLpSlots, hipMemcpyDeviceToHost, st));
      s += (size_t)B * kLpSlots;
      WA_HIP(hipMemcpyAsync(s + g.b0, g.no_speech, nb4, hipMemcpyDeviceToHost, st));
      WA_HIP(hipMemcpyAsync(s + B + g.b0, g.lang_tok, nb4, hipMemcpyDeviceToHost, st));
      WA_HIP(hipMemcpyAsync(s + 2 * B + g.b0, g.lang_prob, nb4, hipMemcpyDeviceToHost, st));
    }
  }
  // one flag word, set by any lane: a flagged unit flags all its batches
  for (int i = 0; i < n; ++i)
    WA_HIP(hipMemcpyAsync(flag + i * lane_stride, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  return WQ4_OK;
}

void copy_tokens(const int32_t* tok, const int32_t* nt, int B, int max_tokens, int32_t* tokens_out,
                 int32_t* n_tokens_out) {
  for (int b = 0; b < B; ++b) {
    n_tokens_out[b] = std::min(nt[b], max_tokens);
    std::memcpy(tokens_out + (size_t)b * max_tokens, tok + (size_t)b * kMaxTokens, (size_t)max_tokens * 4);
  }
}

// The staged scores `sc` of one batch (collect_batch) into the caller's
// arrays at clip `clip0` of them: max_tokens + 1 slots per clip.
void copy_scores(const float* sc, int B, int max_tokens, const wa_scores* out, size_t clip0) {
  const float* s = sc + (size_t)B * kLpSlots;
  if (out->token_logprob)
    for (int b = 0; b < B; ++b)
      std::memcpy(out->token_logprob + (clip0 + b) * (max_tokens + 1), sc + (size_t)b * kLpSlots,
                  (size_t)(max_tokens + 1) * 4);
  if (out->no_speech_prob) std::memcpy(out->no_speech_prob + clip0, s, (size_t)B * 4);
  if (out->lang_token) std::memcpy(out->lang_token + clip0, s + B, (size_t)B * 4);
  if (out->lang_prob) std::memcpy(out->lang_prob + clip0, s + 2 * B, (size_t)B * 4);
}

// One transcribe (whisper.rs:51-128 for a batch of clips); *overflow = the
// range flag of this run (see wa_model::range_flag).  scores (a scored call;
// null otherwise): this run's scores too.
// reuse_enc (the fallback ladder's re-decodes): no encoder pass -- the prompt
// and the loop run again over the planes (and few-clip caches) the last pass
// left, and the prompt / decode times and steps are added to the timings.
wq4_status transcribe_once(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips, int32_t* tokens_out,
                           int32_t* n_tokens_out, void* stream, bool* overflow, const wa_scores* scores,
                           bool reuse_enc = false) {
  // all work on the model's own stream, ordered after the caller's stream
  hipStream_t st = m->own_stream;
  const int B = n_clips, max_tokens = call.max_tokens;
  const int G = decode_groups(B);
  EventSet ev;
  hipEvent_t e_in, e_enc, e_kv, e_ready, e_end, gprompt[kMaxGroups], gdone[kMaxGroups];
  for (hipEvent_t* e : {&e_in, &e_enc, &e_kv, &e_ready, &e_end}) WA_HIP(ev.make(e));
  for (int i = 0; i < G; ++i) {
    WA_HIP(ev.make(&gprompt[i]));
    WA_HIP(ev.make(&gdone[i]));
  }
  WA_HIP(hipEventRecord(e_in, static_cast<hipStream_t>(stream)));
  WA_HIP(hipStreamWaitEvent(st, e_in, 0));
  WA_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(int), st));

  WA_HIP(hipEventRecord(e_enc, st));
  if (!reuse_enc) WA_TRY(encoder_forward(m, mel_dev, B, st, nullptr));
  WA_HIP(hipEventRecord(e_kv, st));
  if (!reuse_enc) WA_TRY(cross_kv_forward(m, B, st, true));
  WA_HIP(hipEventRecord(e_ready, st));
  // decode groups: contiguous clip ranges on their own streams, started
  // after the encoder-planes pass, joined back into `st` at the end
  int gsteps[kMaxGroups] = {};
  WA_TRY(run_decode(m, call, B, 1, 0, e_ready, gprompt, gdone, gsteps));
  const int steps = *std::max_element(gsteps, gsteps + G);  // the last group to stop
  std::vector<int32_t> tok((size_t)B * kMaxTokens), nt(B);
  int flag = 0;
  std::vector<float> sc(scores ? score_words(B) : 0);
  WA_TRY(collect_batch(m, B, 1, gdone, st, tok.data(), nt.data(), &flag, 0, scores ? sc.data() : nullptr));
  WA_HIP(hipEventRecord(e_end, st));
  WA_HIP(hipStreamSynchronize(st));
  *overflow = flag != 0;
  copy_tokens(tok.data(), nt.data(), B, max_tokens, tokens_out, n_tokens_out);
  if (scores) copy_scores(sc.data(), B, max_tokens, scores, 0);
  // phases: encoder, encoder planes (the cross-attention state), prompt (slowest group), decode loop
  float t_enc = 0.0f, t_kv = 0.0f, tp = 0.0f, tall = 0.0f;
  WA_HIP(hipEventElapsedTime(&t_enc, e_enc, e_kv));
  WA_HIP(hipEventElapsedTime(&t_kv, e_kv, e_ready));
  for (int i = 0; i < G; ++i) {
    float t = 0.0f;
    WA_HIP(hipEventElapsedTime(&t, e_ready, gprompt[i]));
    tp = std::max(tp, t);
  }
  WA_HIP(hipEventElapsedTime(&tall, e_ready, e_end));
  if (reuse_enc) {
    m->timings[2] += tp;
    m->timings[3] += tall - tp;
    m->timings[4] += (float)steps;
    return WQ4_OK;
  }
  m->timings[0] = t_enc;
  m->timings[1] = t_kv;
  m->timings[2] = tp;
  m->timings[3] = tall - tp;
  m->timings[4] = (float)steps;
  return WQ4_OK;
}

// The CU-masked stream of the pipelined transcribe's overlapped encoder
// part: bits 0 .. n-1 of the mask, which the driver spreads over the XCDs
// (bit i -> XCD i mod 8), n / 8 CUs of each; created on first use.
wq4_status ensure_enc_stream(wa_model* m) {
  if (m->enc_stream) return WQ4_OK;
  hipDeviceProp_t prop;
  WA_HIP(hipGetDeviceProperties(&prop, m->device));
  const int total = prop.multiProcessorCount;
  int n = kEncOverlapCUs;
  if (const char* e = getenv("WA_ENC_CUS")) n = atoi(e);
  n = std::max(8, std::min(total, n));
  std::vector<uint32_t> mask((total + 31) / 32, 0u);
  for (int i = 0; i < n; ++i) mask[i / 32] |= 1u << (i % 32);
  WA_HIP(hipExtStreamCreateWithCUMask(&m->enc_stream, (uint32_t)mask.size(), mask.data()));
  m->enc_cus = n;
  return WQ4_OK;
}

// wa_transcribe over n_batches batches of n_clips clips, software-pipelined:
// while batch i decodes (its groups' streams), the conv stem and the first
// k encoder layers of batch i + 1 run on the CU-masked stream (a few CUs of
// every XCD; the decode keeps the rest), and once batch i's decode is done
// the remaining layers, ln_post and the encoder planes of batch i + 1 run
// at full width on the model stream.  The encoder buffers are free during a
// decode (it reads only the planes, rewritten after the decode it serves),
// so nothing is double-buffered.  k adapts per batch to the last decode's
// length over the masked stream's measured time per layer.  Every kernel
// computes what it computes in wa_transcribe, with one exception: a unit
// sizes the cross-attention's frame split to the CUs the masked stream and
// its other group leave a launch (run_decode, xattn_plan: a pair of 32-row
// groups gets 5 ranges beside the stream and 6 alone, where the sequential
// call's 16-row groups get 8), so a pipelined unit may use a different split
// than the sequential call -- the same tokens, the partials merged in a
// different grouping.  flags[i] = batch i's range flag (the caller re-runs
// flagged batches).
//
// Batches of 16 .. 32 clips decode in pairs (see kPairMinClips): the decode
// step is a chain of dependent launches whose cost barely grows with the
// rows, so group i of a pair decodes ALL of batch 2p + i (32-row MFMA tiles
// filled, one pass over the decoder weights and the logits table per 32
// clips instead of per 16) from lane i of the planes and self-attention
// caches.  The schedule then runs over units of two batches: beside pair
// p - 1's decode the masked stream takes the conv stem and first k layers
// of batch 2p (k adapts as before and may reach L); after that
// decode the model stream finishes batch 2p's encoder into lane 0 and runs
// all of batch 2p + 1's into lane 1 (the one set of encoder activations
// serves both, in turn), and one `ready` event starts both groups.  An odd
// last batch is a unit of its own on today's groups.  The same four streams
// as unpaired; a batch's tokens are complete when its unit is.
//
// Batches of 17 .. 32 clips decode up to three at a time (kTripleMinClips,
// WA_LANES): a unit of n batches is the same loop at n lanes -- group j
// decodes batch first + j from lane j, the model stream runs the unit's
// encoders one after another into their lanes (all but the first exposed),
// the plane residency is sized to the n * B live clips and the frame split,
// as for a pair, to the CUs the masked stream and the peer groups leave.  A
// call is cut into units by unit_sizes: widest first, and two units of two
// in place of a unit of three and a lone batch.  One more group stream.
wq4_status transcribe_pipelined(wa_model* m, const DecodeCall& call, const float* mel_dev, int NB, int B,
                                int32_t* tokens_out, int32_t* n_tokens_out, void* stream, int* flags,
                                const wa_scores* scores) {
  const int max_tokens = call.max_tokens, eot_stop = call.eot_stop;
  WA_TRY(ensure_enc_stream(m));
  hipStream_t st = m->own_stream, es = m->enc_stream;
  const int L = (int)m->enc.size();
  const size_t mel_stride = (size_t)B * m->cfg.n_mels * 2 * m->cfg.n_audio_ctx;
  // units of several batches need the encoder-plane groups (not the few-clip
  // K/V caches), the default two groups per batch and room for their lanes:
  // only the lanes the widest unit of this call uses are allocated, and a
  // device without room for them gets the units it has lanes for
  int width = 1;
  if (pair_enabled() && B >= kPairMinClips && B <= kPairMaxClips && B > m->kv_small && decode_groups(B) == 2)
    width = std::min(lanes_cap(), B >= kTripleMinClips ? kMaxLanes : 2);
  std::vector<int> sizes = unit_sizes(NB, width);
  const int widest = *std::max_element(sizes.begin(), sizes.end());
  const int lanes = ensure_lanes(m, widest);
  if (lanes < widest) sizes = unit_sizes(NB, lanes);
  // pinned result staging: per batch the groups' tokens, counts and range
  // flag, then (a scored call) its scores
  int32_t* host = nullptr;
  const size_t per0 = (size_t)B * kMaxTokens + B + 1;
  const size_t per = per0 + (scores ? score_words(B) : 0);
  WA_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), (size_t)NB * per * 4, 0));
  struct HostGuard {  // an early error return may leave copies into `p` queued: drain this model's streams first
    wa_model* m;
    int32_t* p;
    bool done = false;  // success: the model stream was synchronised after the last copy
    ~HostGuard() {
      if (!done) {
        (void)hipStreamSynchronize(m->own_stream);
        if (m->enc_stream) (void)hipStreamSynchronize(m->enc_stream);
        for (DecGroup& g : m->groups)
          if (g.st) (void)hipStreamSynchronize(g.st);
      }
      (void)hipHostFree(p);
    }
  } hg{m, host};
  EventSet ev;
  // a unit: the batches [first, first + n) decoded by one run_decode
  struct Unit {
    int first = 0, n = 1;
    hipEvent_t ready, mstart, mend, pstart, gprompt[kMaxGroups], gdone[kMaxGroups];
    int k = 0, gsteps[kMaxGroups] = {};
  };
  std::vector<Unit> ut(sizes.size());
  const int NU = (int)ut.size();
  for (int i = 0, first = 0; i < NU; first += sizes[i++]) {
    ut[i].first = first;
    ut[i].n = sizes[i];
  }
  for (Unit& u : ut) {
    for (hipEvent_t* e : {&u.ready, &u.mstart, &u.mend, &u.pstart}) WA_HIP(ev.make(e));
    for (int i = 0; i < unit_groups(B, u.n); ++i) {
      WA_HIP(ev.make(&u.gprompt[i]));
      WA_HIP(ev.make(&u.gdone[i]));
    }
  }
  // On the model stream: the encoder of unit u's batches at full width, each
  // followed by the planes pass into its lane, then u.ready.  The first
  // batch continues after the k0 layers the masked stream ran (k0 < 0: none
  // of it ran, the conv stem neither).
  auto unit_encoder = [&](Unit& u, int k0) -> wq4_status {
    for (int j = 0; j < u.n; ++j) {
      if (j == 0 && k0 >= 0) {
        WA_TRY(encoder_layers(m, B, k0, L, st));
        WA_TRY(encoder_post(m, B, st, nullptr));
      } else {
        WA_TRY(encoder_forward(m, mel_dev + (u.first + j) * mel_stride, B, st, nullptr));
      }
      WA_TRY(cross_kv_forward(m, B, st, true, j));
    }
    WA_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(int), st));
    WA_HIP(hipEventRecord(u.ready, st));
    return WQ4_OK;
  };
  hipEvent_t e_in, e_enc0;
  WA_HIP(ev.make(&e_in));
  WA_HIP(ev.make(&e_enc0));
  WA_HIP(hipEventRecord(e_in, static_cast<hipStream_t>(stream)));
  WA_HIP(hipStreamWaitEvent(st, e_in, 0));
  // unit 0: the whole encoder(s) at full width
  WA_HIP(hipEventRecord(e_enc0, st));
  WA_TRY(unit_encoder(ut[0], -1));
  // the adapted depth belongs to a batch shape: a call with another clip
  // count or EOT mode starts again from the default
  if (m->overlap_k < 0 || m->overlap_b != B || m->overlap_eot != eot_stop) m->overlap_k = std::min(L, kEncOverlapLayers0);
  m->overlap_b = B;
  m->overlap_eot = eot_stop;
  double t_exposed = 0.0, t_masked = 0.0, t_decode = 0.0, t_prompt = 0.0, k_sum = 0.0;
  int32_t steps_all = 0;
  for (int i = 0; i < NU; ++i) {
    Unit& u = ut[i];
    if (i >= 1) {
      // unit i - 1 is decoded (and unit i's masked part done) before unit
      // i's decode is enqueued: the GPU meanwhile runs unit i's remaining
      // encoder work; adapt k to the finished decode
      Unit& p = ut[i - 1];
      const int PG = unit_groups(B, p.n);
      for (int g = 0; g < PG; ++g) WA_HIP(hipEventSynchronize(p.gdone[g]));
      WA_HIP(hipEventSynchronize(p.mend));
      float td = 0.0f, tm = 0.0f;
      for (int g = 0; g < PG; ++g) {
        float t = 0.0f;
        WA_HIP(hipEventElapsedTime(&t, p.ready, p.gdone[g]));
        td = std::max(td, t);
      }
      WA_HIP(hipEventElapsedTime(&tm, p.mstart, p.mend));
      if (!getenv("WA_ENC_OVERLAP")) {
        const double per_layer = tm / (double)(p.k + 1);  // the conv stem counts as one layer
        double fill = kEncOverlapFill;
        if (const char* e = getenv("WA_ENC_FILL")) fill = atof(e);  // A/B only
        m->overlap_k = std::max(0, std::min(L, (int)(fill * td / per_layer) - 1));
      }
    }
    if (const char* e = getenv("WA_ENC_OVERLAP")) m->overlap_k = std::max(0, std::min(L, atoi(e)));
    if (i + 1 < NU) {  // the masked part of the next unit's first batch, beside unit i's decode
      u.k = m->overlap_k;
      WA_HIP(hipStreamWaitEvent(es, u.ready, 0));
      WA_HIP(hipEventRecord(u.mstart, es));
      WA_TRY(encoder_front(m, mel_dev + ut[i + 1].first * mel_stride, B, es));
      WA_TRY(encoder_layers(m, B, 0, u.k, es));
      WA_HIP(hipEventRecord(u.mend, es));
    }
    // the masked part above takes its CUs from this decode; the last unit has them all
    WA_TRY(run_decode(m, call, B, u.n, i + 1 < NU ? m->enc_cus : 0, u.ready, u.gprompt, u.gdone, u.gsteps, u.first));
    int32_t* hb = host + (size_t)u.first * per;
    WA_TRY(collect_batch(m, B, u.n, u.gdone, st, hb, hb + (size_t)B * kMaxTokens, hb + (size_t)B * kMaxTokens + B,
                         per, scores ? reinterpret_cast<float*>(hb + per0) : nullptr));
    if (i + 1 < NU) {  // the rest of the next unit's encoder work at full width
      WA_HIP(hipStreamWaitEvent(st, u.mend, 0));
      WA_HIP(hipEventRecord(u.pstart, st));
      WA_TRY(unit_encoder(ut[i + 1], u.k));
    }
  }
  WA_HIP(hipStreamSynchronize(st));
  hg.done = true;
  for (int i = 0; i < NB; ++i) {
    const int32_t* hb = host + (size_t)i * per;
    copy_tokens(hb, hb + (size_t)B * kMaxTokens, B, max_tokens, tokens_out + (size_t)i * B * max_tokens,
                n_tokens_out + (size_t)i * B);
    flags[i] = hb[(size_t)B * kMaxTokens + B];
    if (scores) copy_scores(reinterpret_cast<const float*>(hb + per0), B, max_tokens, scores, (size_t)i * B);
  }
  // per-unit phases, averaged over the batches below: the exposed encoder,
  // prompt and decode times of a unit of n count 1 / n for each of its batches
  int pairs = 0, units3 = 0;
  for (int i = 0; i < NU; ++i) {
    Unit& u = ut[i];
    const int UG = unit_groups(B, u.n);
    pairs += u.n == 2;
    units3 += u.n == 3;
    float t = 0.0f, tp = 0.0f, td = 0.0f;
    if (i == 0) {
      WA_HIP(hipEventElapsedTime(&t, e_enc0, u.ready));
    } else {
      WA_HIP(hipEventElapsedTime(&t, ut[i - 1].pstart, u.ready));
      float tm = 0.0f;
      WA_HIP(hipEventElapsedTime(&tm, ut[i - 1].mstart, ut[i - 1].mend));
      t_masked += tm;
      k_sum += ut[i - 1].k;
    }
    t_exposed += t;
    for (int g = 0; g < UG; ++g) {
      float a = 0.0f, d = 0.0f;
      WA_HIP(hipEventElapsedTime(&a, u.ready, u.gprompt[g]));
      WA_HIP(hipEventElapsedTime(&d, u.ready, u.gdone[g]));
      tp = std::max(tp, a);
      td = std::max(td, d);
    }
    t_prompt += tp;
    t_decode += td - tp;
    // steps of a batch: its group's in a unit of several, else the last group's to stop
    if (u.n > 1)
      for (int g = 0; g < u.n; ++g) steps_all += u.gsteps[g];
    else
      steps_all += *std::max_element(u.gsteps, u.gsteps + UG);
  }
  m->timings[0] = (float)(t_exposed / NB);
  m->timings[1] = 0.0f;
  m->timings[2] = (float)(t_prompt / NB);
  m->timings[3] = (float)(t_decode / NB);
  m->timings[4] = (float)steps_all / NB;
  m->pipe[0] = (float)NB;
  m->pipe[1] = NU > 1 ? (float)(k_sum / (NU - 1)) : 0.0f;  // per masked part
  m->pipe[2] = NU > 1 ? (float)(t_masked / (NU - 1)) : 0.0f;
  m->pipe[3] = (float)m->enc_cus;
  m->pipe_pairs = pairs;
  m->pipe_units3 = units3;
  return WQ4_OK;
}

}  // namespace

// Sizes of the units a call over NB batches decodes at up to `width` batches
// at once: widest first, and no lone last batch where taking one batch fewer
// leaves a unit of two (4 -> 2 + 2, 7 -> 3 + 2 + 2) -- a lone batch of 17 ..
// 32 clips decodes in two groups of half its rows, the slowest form there is.
std::vector<int> wa::unit_sizes(int NB, int width) {
  std::vector<int> sizes;
  for (int rem = NB; rem > 0; rem -= sizes.back()) {
    int n = std::min(width, rem);
    if (rem - n == 1 && n > 2) --n;
    sizes.push_back(n);
  }
  return sizes;
}

bool wa::bad_temperatures(const float* t, int n) {
  for (int i = 0; i < n; ++i)
    if (!(t[i] >= 0.0f) || !std::isfinite(t[i])) return true;
  return false;
}

// One range tier up after a flagged run (see transcribe_tiers); WQ4_ERANGE at the last.
wq4_status wa::raise_tier(wa_model* m) {
  if (m->range_tier == 3)
    return fail(WQ4_ERANGE,
                "activation overflow: an MFMA operand left the f16-pair range (|x| >= 4094 after every range tier: "
                "LayerNorm path, per-call FFN and attention-projection operand scales) and the logits are not finite");
  if (m->range_tier == 1) WA_TRY(ensure_ffn_ws(m));  // entering tier 2
  ++m->range_tier;
  return WQ4_OK;
}

// The temperature ladder of wa_transcribe_fallback (and of every round of
// wa_transcribe_long), its arguments checked by the entry: one encoder pass,
// then per rung a prompt + decode over the same planes with the clips that
// have passed frozen.
wq4_status wa::transcribe_ladder(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips,
                                 const wa_fallback* fb, int32_t* tokens_out, int32_t* n_tokens_out,
                                 const wa_scores* scores, int32_t* rung_out, void* stream) {
  const int B = n_clips, R = fb->n_temperatures, max_tokens = call.max_tokens;
  const size_t slots = (size_t)max_tokens + 1;
  std::vector<float> temp(B);
  std::vector<uint64_t> seed(B);
  // one rung's results; the clips it was run for are copied to the caller's arrays
  std::vector<int32_t> tok((size_t)B * max_tokens), nt(B), lt(B);
  std::vector<float> lp((size_t)B * slots), ns(B), lpr(B);
  const wa_scores rung_scores{lp.data(), ns.data(), lt.data(), lpr.data()};
  for (;;) {  // the range tiers: a flagged rung restarts the ladder one tier up
    bool overflow = false;
    std::vector<uint8_t> frozen(B, 0);
    int n_frozen = 0;
    for (int r = 0; r < R && n_frozen < B && !overflow; ++r) {
      for (int c = 0; c < B; ++c) {
        temp[c] = fb->temperatures[r];
        seed[c] = fb->seed[c] + (uint64_t)r;
      }
      const DecodeCall rung = call.with_clips(temp.data(), seed.data(), r > 0 ? frozen.data() : nullptr);
      WA_TRY(transcribe_once(m, rung, mel_dev, B, tok.data(), nt.data(), stream, &overflow, &rung_scores, r > 0));
      if (overflow) break;
      for (int c = 0; c < B; ++c) {
        if (frozen[c]) continue;
        std::memcpy(tokens_out + (size_t)c * max_tokens, tok.data() + (size_t)c * max_tokens, (size_t)max_tokens * 4);
        n_tokens_out[c] = nt[c];
        if (rung_out) rung_out[c] = r;
        if (scores) {
          if (scores->token_logprob) std::memcpy(scores->token_logprob + c * slots, lp.data() + c * slots, slots * 4);
          if (scores->no_speech_prob) scores->no_speech_prob[c] = ns[c];
          if (scores->lang_token) scores->lang_token[c] = lt[c];
          if (scores->lang_prob) scores->lang_prob[c] = lpr[c];
        }
        // the ladder rule: the mean of the stored log-probabilities below the
        // threshold, unless the no-speech score calls the clip silence
        // (comparisons with a NaN threshold are false: that test is off)
        double sum = 0.0;
        int cnt = 0;
        for (size_t i = 0; i < slots; ++i) {
          const float v = lp[c * slots + i];
          if (!std::isnan(v)) {
            sum += v;
            ++cnt;
          }
        }
        const double mean = cnt ? sum / cnt : 0.0;
        const bool needs = mean < (double)fb->logprob_threshold && !(ns[c] > fb->no_speech_threshold);
        if (!needs) {
          frozen[c] = 1;
          ++n_frozen;
        }
      }
    }
    if (!overflow) return WQ4_OK;
    WA_TRY(raise_tier(m));
  }
}

// A transcribe through the range tiers; the scores are those of the run whose
// tokens are returned.
wq4_status wa::transcribe_tiers(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips,
                                int32_t* tokens_out, int32_t* n_tokens_out, void* stream, const wa_scores* scores) {
  // A flagged run is retried one range tier up (wa_model::range_tier), sticky
  // for the model: its activations evidently exceed the range below.
  //   0 -> 1  the LayerNorm fold feeds the raw residual stream to the MFMAs
  //   1 -> 2  the FFN hidden layer (fc1 + GELU) feeds fc2 unnormalised
  //   2 -> 3  an attention output feeds its output projection unnormalised
  //           (tier 3 needs tier 2's workspaces, already allocated)
  for (;;) {
    bool overflow = false;
    WA_TRY(transcribe_once(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, &overflow, scores));
    if (!overflow) return WQ4_OK;
    WA_TRY(raise_tier(m));
  }
}

// The pipelined batches of a call, then the flagged ones through the tiers.
static wq4_status transcribe_batches(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_batches,
                                     int n_clips, int32_t* tokens_out, int32_t* n_tokens_out, void* stream,
                                     const wa_scores* scores) {
  const int max_tokens = call.max_tokens;
  std::vector<int> flags(n_batches, 0);
  WA_TRY(transcribe_pipelined(m, call, mel_dev, n_batches, n_clips, tokens_out, n_tokens_out, stream, flags.data(),
                              scores));
  const size_t mel_stride = (size_t)n_clips * m->cfg.n_mels * 2 * m->cfg.n_audio_ctx;
  // the pipeline decoded every batch at the tier the model had on entry
  const int tier0 = m->range_tier;
  for (int i = 0; i < n_batches; ++i) {
    // a flagged batch goes through wa_transcribe's range tiers on its own;
    // once that raised the (sticky) tier, the later batches are re-run at it
    // too -- one wa_transcribe per batch would have decoded them there
    if (!flags[i] && m->range_tier == tier0) continue;
    const size_t c0 = (size_t)i * n_clips;
    wa_scores at{};  // batch i's part of the caller's arrays
    if (scores) {
      at.token_logprob = scores->token_logprob ? scores->token_logprob + c0 * (max_tokens + 1) : nullptr;
      at.no_speech_prob = scores->no_speech_prob ? scores->no_speech_prob + c0 : nullptr;
      at.lang_token = scores->lang_token ? scores->lang_token + c0 : nullptr;
      at.lang_prob = scores->lang_prob ? scores->lang_prob + c0 : nullptr;
    }
    // (a sampled call: batch i's temperatures and seeds lead the re-run's per-clip arrays)
    WA_TRY(transcribe_tiers(m, call.at_clip(c0), mel_dev + i * mel_stride, n_clips, tokens_out + c0 * max_tokens,
                            n_tokens_out + c0, stream, scores ? &at : nullptr));
  }
  return WQ4_OK;
}

// The transcribe entries' argument check, in one order.  ptrs_ok: no pointer
// the entry needs is null.  temps (nullable): a ladder's temperatures, one per
// rung (`rungs` set), or a sampled call's, one per clip.
wq4_status wa::check_args(const wa_model* m, bool ptrs_ok, int n_batches, int max_tokens, int n_clips,
                          const float* temps, const int* rungs) {
  if (!m || !ptrs_ok) return fail(WQ4_EINVAL, "null argument");
  if (n_batches < 1) return fail(WQ4_EINVAL, "n_batches must be >= 1");
  if (rungs && (*rungs < 1 || *rungs > 8)) return fail(WQ4_EINVAL, "the ladder has 1 .. 8 rungs");
  if (max_tokens < 1 || max_tokens > kMaxTokens) return fail(WQ4_EINVAL, "max_tokens must be in [1, 224]");
  if (temps && bad_temperatures(temps, rungs ? *rungs : n_clips >= 1 ? n_batches * n_clips : 0))
    return fail(WQ4_EINVAL, "every temperature must be finite and >= 0");
  if (n_clips < 1 || n_clips > m->bmax) return fail(WQ4_EINVAL, "n_clips out of range");  // last: the only read of *m
  return WQ4_OK;
}

static DecodeCall sampled_call(int lang_token, int max_tokens, int eot_stop, const wa_sampling& s) {
  return DecodeCall(lang_token, max_tokens, eot_stop, true, s.timestamps != 0, s.max_initial, true)
      .with_clips(s.temperature, s.seed, nullptr);
}

extern "C" {

// Every entry: build the call, check the arguments, prepare the model, run.

wq4_status wa_transcribe(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                         int eot_stop, int32_t* tokens_out, int32_t* n_tokens_out, void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, false);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out, 1, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, nullptr);
}

wq4_status wa_transcribe_scored(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                                int eot_stop, int32_t* tokens_out, int32_t* n_tokens_out, const wa_scores* scores,
                                void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, true);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out && scores, 1, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, scores);
}

wq4_status wa_transcribe_batches(wa_model* m, const float* mel_dev, int n_batches, int n_clips, int lang_token,
                                 int max_tokens, int eot_stop, int32_t* tokens_out, int32_t* n_tokens_out,
                                 void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, false);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out, n_batches, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_batches(m, call, mel_dev, n_batches, n_clips, tokens_out, n_tokens_out, stream, nullptr);
}

wq4_status wa_transcribe_batches_scored(wa_model* m, const float* mel_dev, int n_batches, int n_clips,
                                        int lang_token, int max_tokens, int eot_stop, int32_t* tokens_out,
                                        int32_t* n_tokens_out, const wa_scores* scores, void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, true);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out && scores, n_batches, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_batches(m, call, mel_dev, n_batches, n_clips, tokens_out, n_tokens_out, stream, scores);
}

wq4_status wa_transcribe_timestamps(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                                    int eot_stop, int max_initial, int32_t* tokens_out, int32_t* n_tokens_out,
                                    const wa_scores* scores, void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, true, true, max_initial);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out, 1, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, scores);
}

wq4_status wa_transcribe_batches_timestamps(wa_model* m, const float* mel_dev, int n_batches, int n_clips,
                                            int lang_token, int max_tokens, int eot_stop, int max_initial,
                                            int32_t* tokens_out, int32_t* n_tokens_out, const wa_scores* scores,
                                            void* stream) {
  const DecodeCall call(lang_token, max_tokens, eot_stop, true, true, max_initial);
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out, n_batches, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  return transcribe_batches(m, call, mel_dev, n_batches, n_clips, tokens_out, n_tokens_out, stream, scores);
}

// (the sampled entries and the ladder read their struct to build the call: they check first)
wq4_status wa_transcribe_sampled(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                                 int eot_stop, const wa_sampling* sampling, int32_t* tokens_out,
                                 int32_t* n_tokens_out, const wa_scores* scores, void* stream) {
  const bool ok = mel_dev && tokens_out && n_tokens_out && sampling && sampling->temperature && sampling->seed;
  WA_TRY(check_args(m, ok, 1, max_tokens, n_clips, ok ? sampling->temperature : nullptr));
  const DecodeCall call = sampled_call(lang_token, max_tokens, eot_stop, *sampling);
  WA_TRY(prepare_call(m, call));
  return transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, scores);
}

wq4_status wa_transcribe_batches_sampled(wa_model* m, const float* mel_dev, int n_batches, int n_clips,
                                         int lang_token, int max_tokens, int eot_stop, const wa_sampling* sampling,
                                         int32_t* tokens_out, int32_t* n_tokens_out, const wa_scores* scores,
                                         void* stream) {
  const bool ok = mel_dev && tokens_out && n_tokens_out && sampling && sampling->temperature && sampling->seed;
  WA_TRY(check_args(m, ok, n_batches, max_tokens, n_clips, ok ? sampling->temperature : nullptr));
  const DecodeCall call = sampled_call(lang_token, max_tokens, eot_stop, *sampling);
  WA_TRY(prepare_call(m, call));
  return transcribe_batches(m, call, mel_dev, n_batches, n_clips, tokens_out, n_tokens_out, stream, scores);
}

// The temperature fallback ladder: one encoder pass, then per rung a prompt +
// decode over the same planes with the clips that have passed frozen.
wq4_status wa_transcribe_fallback(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                                  int eot_stop, const wa_fallback* fb, int32_t* tokens_out, int32_t* n_tokens_out,
                                  const wa_scores* scores, int32_t* rung_out, void* stream) {
  const bool ok = mel_dev && tokens_out && n_tokens_out && fb && fb->temperatures && fb->seed;
  WA_TRY(check_args(m, ok, 1, max_tokens, n_clips, ok ? fb->temperatures : nullptr, ok ? &fb->n_temperatures : nullptr));
  const DecodeCall call(lang_token, max_tokens, eot_stop, true, fb->timestamps != 0, fb->max_initial, true);
  WA_TRY(prepare_call(m, call));
  return transcribe_ladder(m, call, mel_dev, n_clips, fb, tokens_out, n_tokens_out, scores, rung_out, stream);
}

wq4_status wa_timestamp_rule(const int32_t* tokens, int n, int ts0, int V, int max_initial, int32_t* record_out) {
  if (!record_out || n < 0 || (n > 0 && !tokens) || ts0 < 1 || V < ts0) return fail(WQ4_EINVAL, "bad arguments");
  TsRule r = ts_rule_first(ts0, V, max_initial);
  for (int i = 0; i < n; ++i) r = ts_rule_next(r, tokens[i], ts0, V);
  std::memcpy(record_out, &r, sizeof(r));
  return WQ4_OK;
}

wq4_status wa_sample_noise(uint64_t seed, int pick, int id0, int n, float* u_out, float* g_out) {
  if (pick < 0 || id0 < 0 || n < 0 || (n > 0 && !u_out && !g_out)) return fail(WQ4_EINVAL, "bad arguments");
  sample_noise(seed, pick, id0, n, u_out, g_out);
  return WQ4_OK;
}

// OpenAI transcribe.py's slicing of one window's tokens at consecutive
// timestamp pairs (host only).
wq4_status wa_segments_from_tokens(const int32_t* tokens, int n, int ts0, wa_segment* segs, int cap, int* n_segs,
                                   int* seek_frames) {
  if (!n_segs || !seek_frames || n < 0 || cap < 0 || (n > 0 && !tokens) || (cap > 0 && !segs))
    return fail(WQ4_EINVAL, "bad arguments");
  std::vector<wa_segment> out;
  int seek = 3000;
  auto is_ts = [&](int i) { return tokens[i] >= ts0; };
  auto secs = [&](int i) { return (float)((tokens[i] - ts0) * 0.02); };
  if (n > 0) {
    const bool single_end = n >= 2 && !is_ts(n - 2) && is_ts(n - 1);
    std::vector<int> cuts;
    for (int i = 1; i < n; ++i)
      if (is_ts(i - 1) && is_ts(i)) cuts.push_back(i);
    if (!cuts.empty()) {
      if (single_end) cuts.push_back(n);
      int last = 0;
      for (int c : cuts) {
        out.push_back(wa_segment{secs(last), secs(c - 1), last, c});
        last = c;
      }
      if (!single_end) seek = (tokens[last - 1] - ts0) * 2;
    } else {
      float end = 30.0f;
      for (int i = n - 1; i >= 0; --i)
        if (is_ts(i)) {  // the last timestamp, when it is not <|0.00|>
          if (tokens[i] != ts0) end = secs(i);
          break;
        }
      out.push_back(wa_segment{0.0f, end, 0, n});
    }
  }
  *n_segs = (int)out.size();
  *seek_frames = seek;
  if ((int)out.size() > cap) return fail(WQ4_EINVAL, "segs too small: *n_segs segments are needed");
  std::copy(out.begin(), out.end(), segs);
  return WQ4_OK;
}

wq4_status wa_last_pipeline_stats(const wa_model* m, float* out) {
  if (!m || !out) return fail(WQ4_EINVAL, "null argument");
  std::memcpy(out, m->pipe, sizeof(m->pipe));
  return WQ4_OK;
}

int wa_last_pipeline_pairs(const wa_model* m) { return m ? m->pipe_pairs : 0; }

int wa_last_pipeline_units3(const wa_model* m) { return m ? m->pipe_units3 : 0; }

wq4_status wa_transcribe_trace(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                               int eot_stop, int32_t* tokens_out, int32_t* n_tokens_out, const int32_t* trace_ids_dev,
                               int trace_k, float* trace_out_dev, void* stream) {
  if (!m || !trace_ids_dev || !trace_out_dev || trace_k < 1) return fail(WQ4_EINVAL, "bad trace arguments");
  DecodeCall call(lang_token, max_tokens, eot_stop, false);
  call.trace_ids = trace_ids_dev;
  call.trace_out = trace_out_dev;
  call.trace_s1 = max_tokens + 1;
  call.trace_k = trace_k;
  WA_TRY(check_args(m, mel_dev && tokens_out && n_tokens_out, 1, max_tokens, n_clips));
  WA_TRY(prepare_call(m, call));
  const wq4_status s = transcribe_tiers(m, call, mel_dev, n_clips, tokens_out, n_tokens_out, stream, nullptr);
  for (DecGroup& g : m->groups) {  // the trace graphs bake in the caller's buffers: never replay them again
    if (g.graph) (void)hipGraphExecDestroy(g.graph);
    g.graph = nullptr;
    g.graph_key = -1;
    for (DecGroup::KeptGraph& k : g.kept) {
      if (k.exec) (void)hipGraphExecDestroy(k.exec);
      k = DecGroup::KeptGraph{};
    }
  }
  return s;
}

}  // extern "C"
