// wa_model.hpp -- internal: the Whisper model runtime's state (struct
// wa_model) and what its translation units (wa_weights, wa_forward,
// wa_transcribe, wa_long, wa_prompt, wa_align, wa_beam, wa_mel, wa_api,
// wa_checks .cpp) need from one another.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/whisper_amd_checks.h"
#include "../../../include/wq4.h"
#include "wa_align.hpp"
#include "wa_beam.hpp"
#include "wa_gguf.hpp"
#include "wa_kernels.hpp"
#include "wa_pick.hpp"

namespace wa {

// records the calling thread's error string (wa_last_error) and returns s
wq4_status fail(wq4_status s, const std::string& m);

#define WA_HIP(expr)                                                                                \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return wa::fail(WQ4_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define WA_WQ4(expr)                                                                    \
  do {                                                                                  \
    wq4_status s_ = (expr);                                                             \
    if (s_ != WQ4_OK) return wa::fail(s_, std::string(#expr) + ": " + wq4_last_error()); \
  } while (0)
// a call that has already recorded its error
#define WA_TRY(expr)             \
  do {                           \
    wq4_status s_ = (expr);      \
    if (s_ != WQ4_OK) return s_; \
  } while (0)

constexpr int kMaxTokens = 224;  // whisper.rs:20
constexpr int kMinTokens = 3;    // whisper.rs:97

struct Config {  // WhisperConfig, src/model/config.rs:5-30
  int n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int n_text_ctx, n_text_state, n_text_head, n_text_layer, n_vocab, n_lang;
  int transcribe_token() const { return 50260 + n_lang; }      // config.rs:66-69
  int no_timestamps_token() const { return transcribe_token() + 4; }  // config.rs:72-74
  int no_speech_token() const { return no_timestamps_token() - 1; }   // <|nospeech|>, the token before it
};

struct Dev {
  std::vector<void*> ptrs;
  ~Dev() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(T) + 256) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
  // frees one pointer alloc() returned (null: no-op)
  void release(void* p) {
    if (!p) return;
    for (void*& q : ptrs)
      if (q == p) {
        (void)hipFree(q);
        q = ptrs.back();
        ptrs.pop_back();
        return;
      }
  }
};

struct EncLayer {
  float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *qkv_b, *out_b, *fc1_b, *fc2_b;
  wq4_tensor *qkv = nullptr, *out = nullptr, *fc1 = nullptr, *fc2 = nullptr;
};
struct DecLayer {
  float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
  float *qkv_b, *out_b, *cq_b, *cv_b, *cout_b, *fc1_b, *fc2_b;
  wq4_tensor *qkv = nullptr, *out = nullptr, *cq = nullptr, *cout = nullptr, *fc1 = nullptr, *fc2 = nullptr;
  // LayerNorm fold (wq4_gemm_tiled_lnfold) of the GEMMs that read a
  // LayerNorm: W gamma and W beta + bias of qkv (attn_ln), cq
  // (cross_attn_ln), fc1 (mlp_ln)
  float *qkv_wg = nullptr, *qkv_b2 = nullptr, *cq_wg = nullptr, *cq_b2 = nullptr, *fc1_wg = nullptr,
        *fc1_b2 = nullptr;
  // cross-attention key / value weights in raw GGUF form (Q4_0 blocks or
  // f16), read by the K/V-cache-free cross-attention (wa_xattn.hip)
  uint8_t *ck_raw = nullptr, *cv_raw = nullptr;
  uint32_t* cv_p = nullptr;  // Q4_0: cv_raw in the projection's lane order (wa::launch_wv_pack)
  // (the self-attention caches are per lane: wa::Lane)
  // few-clip decode groups (wa_model::kv_clips): the reference's per-layer
  // cross K / V caches, head-major [clip][head][T][64] f32, written by the
  // head-major GEMMs of ck / cv over the encoder output (cross_kv_forward)
  wq4_tensor *ck = nullptr, *cv = nullptr;
  float *xk = nullptr, *xv = nullptr;
};

// One lane of per-clip decode state, bmax clips: the encoder output as f16
// planes [clip][T][ns][D] (the cross-attention's only per-clip state, no
// per-layer K/V caches) and every decoder layer's self-attention caches
// [clip][ctx][D] f32.  Lane 0 always exists; a wa_transcribe_batches that
// decodes n batches at once, one decode group per batch, puts batch j in lane
// j (ensure_lanes: allocated by the first call that needs them, all or
// nothing per lane, never released).
constexpr int kMaxLanes = 3;
struct Lane {
  _Float16* planes = nullptr;
  std::vector<float*> cache_k, cache_v;  // per decoder layer
};

// One decode group: a contiguous range of clips [b0, b0 + nb) of one lane
// (wa_model::lanes) decoded on its own stream with its own activations, DecodeState and step graph.  The
// decode step is a chain of ~350 small dependent kernels (latency-bound);
// groups on separate streams overlap one another's launch gaps and let the
// HBM-bound cross-attention of one group run beside the latency-bound GEMMs
// of another.  Per-clip results do not depend on the grouping (every
// kernel's per-row arithmetic is independent of the batch).
constexpr int kMaxGroups = 4;
constexpr int kKeptGraphs = 4;
struct DecGroup {
  hipStream_t st = nullptr;
  int b0 = 0, nb = 0;
  int lane = 0;
  // cache residency of the encoder planes for the decode this group is part
  // of (run_decode: from the clips of every group that decodes beside it);
  // baked into the captured step graph
  XattnResidency xres;
  // the cross-attention's frame split for that decode (run_decode: one plan
  // for all its groups, prompt and steps); baked into the step graph too
  XattnPlan xplan{0, 0};
  float *xd, *qkvd, *qd, *hid, *logits;
  _Float16 *atd_dec, *atf_dec;
  int *prompt_tok, *next_tok, *tokens, *ntok, *done;
  _Float16* xqt;    // cross-attention Wk^T q operands [rows][ns][16*ceil(H/16)][D]
  float* xattn_part;  // cross-attention split partials (Z, max, sum)
  float* xkv_part;    // cross-attention over cached K / V: split partials
  int* xkv_ctr;       //   and the per-(clip, head) arrival counters
  _Float16* atd_ln;   // LayerNorm fold: A-tiled x * gamma of the next LayerNorm
  float* ln_stats;    //                 its per (row, 32-column tile) mean / M2
  _Float16* hid_t;    // fused logits + pick: the final LN, A-tiled (m-tile 0)
  float* lg_scr;      //                      the workgroups' candidates (PickArgs::scratch)
  int* lg_ctr;
  // scored transcribes (wa_transcribe_scored; allocated by the first one,
  // ensure_score_buffers): the log-probability of next_tok, every stored
  // pick's [nb][kMaxTokens + 1] (NaN where nothing was stored), the prompt's
  // no-speech and language probabilities with the language token, and the SOT
  // position's logit rows [nb][n_vocab] of an explicit-language prompt
  float *next_lp = nullptr, *logprob = nullptr;
  float *no_speech = nullptr, *lang_prob = nullptr, *z0 = nullptr;
  int* lang_tok = nullptr;
  // timestamp transcribes (wa_transcribe_timestamps; allocated by the first
  // one, ensure_ts_buffers): every clip's rule record, advanced by the
  // bookkeeping kernel
  TsRule* ts_rules = nullptr;
  // sampled transcribes (wa_transcribe_sampled; allocated by the first one,
  // ensure_sample_buffers): the clips' temperatures and seeds, uploaded by
  // every prompt from the caller's arrays at clip `clip0` of them
  float* smp_temp = nullptr;
  uint64_t* smp_seed = nullptr;
  int clip0 = 0;  // this group's first clip in the call's per-clip host arrays (run_decode)
  // prompted transcribes (wa_transcribe_prompted; allocated by the first one,
  // ensure_prefill): the clips' first cache slots [nb] -- prompts are
  // right-aligned to the group's longest -- read by the prefill and by the pad
  // forms of the step's embedding and self-attention
  int* pad = nullptr;
  DecodeState* state;
  void* ffn_ws = nullptr;  // range tier 2: wq4_ffn_forward_ws workspace (4 * nb rows)
  size_t ffn_ws_bytes = 0;
  int* host_ndone = nullptr;  // pinned ring
  hipGraphExec_t graph = nullptr;
  int64_t graph_key = -1;  // wa::graph_key of the layout and mode the graph was captured for
  bool graph_prompted = false;  // beside the key: the graph runs the pad forms (a prompted call's)
  // graphs of other layouts this group ran (ensure_graph): a call of units of
  // three and two, with and without the masked stream beside them, goes
  // through four keys per group and comes back to each
  struct KeptGraph {
    hipGraphExec_t exec = nullptr;
    int64_t key = -1;
    bool prompted = false;
  };
  KeptGraph kept[kKeptGraphs];
  int kept_next = 0;  // the slot the next parked graph replaces once all are taken
  // beam calls (wa_transcribe_beam): their step graph has a slot of its own,
  // re-captured when what it bakes in changes (wa_beam.cpp, BeamKey); the
  // graphs and keys above never see a beam call
  hipGraphExec_t beam_graph = nullptr;
  int beam_key[10] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
};

// One transcribe call's decode: built by its entry and passed down to every
// prompt, step and pick of the call (the model holds no mode).
struct DecodeCall {
  int lang_token = -1, max_tokens = 0, eot_stop = 0;
  // score: prompts and steps also leave the picks' log-probabilities, the
  // no-speech and the language probability in the groups' score buffers.
  // ts: the prompt drops NO_TIMESTAMPS and every pick runs under the timestamp
  // rules, the first timestamp at most ts_max_initial ids past <|0.00|> (< 0:
  // unbounded).  sample: every pick is the Gumbel-max pick at the clip's
  // temperature and seed.  ts or sample imply score (the constructor sees to
  // it): such a pick always leaves its log-probability.
  bool score = false, ts = false, sample = false;
  int ts_max_initial = 50;
  // sampled calls: host arrays over the call's clips (DecGroup::clip0 indexes
  // them), read by the prompts.  frozen (nullable): clips that start the decode
  // done -- their picks go nowhere and the decode stops once the live clips
  // emitted EOT (the fallback ladder's re-decodes).
  const float* temp = nullptr;
  const uint64_t* seed = nullptr;
  const uint8_t* frozen = nullptr;
  // prompted calls (wa_transcribe_prompted; null otherwise): the clips' own
  // prompts, host arrays over the call's clips like the ones above.  The
  // prompt of every group is then one prefill pass and its steps run the pad
  // forms; lang_token is not read.
  const wa_prompt* prompt = nullptr;
  // decode-step logit trace (wa_transcribe_trace; null otherwise): device
  // [clip][trace_s1][trace_k] ids and their logits
  const int* trace_ids = nullptr;
  float* trace_out = nullptr;
  int trace_s1 = 0, trace_k = 0;
  // alignment calls (wa_align; false otherwise): the prefill of `prompt` also
  // leaves the head mean of the filtered cross-attention weights in the
  // model's alignment buffers (wa_model::Align; the group's F uploaded by the
  // entry) and stops there -- no logits, no scores
  bool align = false;
  // beam calls (wa_transcribe_beam; 0 otherwise): beams per clip and finished
  // sequences kept per clip.  The group's rows are clip * beam_k + beam; the
  // steps read the self-attention caches through the ancestor table and keep
  // the stored logits (no fused pick)
  int beam_k = 0, beam_c = 0;

  DecodeCall() = default;
  DecodeCall(int lang, int max_tok, int eot, bool score_, bool ts_ = false, int max_initial = 50, bool sample_ = false)
      : lang_token(lang), max_tokens(max_tok), eot_stop(eot), score(score_ || ts_ || sample_), ts(ts_), sample(sample_),
        ts_max_initial(max_initial) {}
  // the same call over other per-clip arrays (a rung of the fallback ladder)
  DecodeCall with_clips(const float* t, const uint64_t* s, const uint8_t* f) const {
    DecodeCall c = *this;
    c.temp = t;
    c.seed = s;
    c.frozen = f;
    return c;
  }
  // the call whose clip 0 is this call's clip c (one batch of a call over several)
  DecodeCall at_clip(size_t c) const {
    return with_clips(temp ? temp + c : nullptr, seed ? seed + c : nullptr, frozen ? frozen + c : nullptr);
  }
};

// Everything a captured decode step bakes in, as one mixed-radix number, most
// significant digit first: the mode (score = 1, ts = 2, sample = 4; the rule's
// max_initial, the temperatures and the seeds are read at run time), the clip
// range (self-KV and encoder-plane offsets), the EOT mode, the trace buffers,
// the few-clip caches, the range tier, the cross-attention's frame split (its
// splits fix the plan of a T) and the planes' cache residency.  A digit
// outside its radix would alias another layout's key: -1, *bad naming it.
inline int64_t graph_key(int mode, int lane, int b0, int nb, int eot, int trace, int group_kv, int range_tier,
                         int splits, int q, const char** bad = nullptr) {
  const struct {
    const char* name;
    int value, radix;
  } digits[] = {{"mode", mode, 8},         {"lane", lane, kMaxLanes},     {"b0", b0, 512},
                {"nb", nb, 512},           {"eot", eot, 2},               {"trace", trace, 2},
                {"group_kv", group_kv, 2}, {"range_tier", range_tier, 4}, {"splits", splits, 16},
                {"residency", q, kXattnResDen + 1}};
  int64_t key = 0;
  for (const auto& d : digits) {
    if (d.value < 0 || d.value >= d.radix) {
      if (bad) *bad = d.name;
      return -1;
    }
    key = key * d.radix + d.value;
  }
  return key;
}

}  // namespace wa

struct wa_model {
  int device = 0;
  wa::Config cfg{};
  wq4_precision prec = WQ4_PREC_F16X2;
  int ns = 2;
  int bmax = 1;
  wa::Dev dev;
  size_t bytes = 0;
  // globals
  float *conv1_wt, *conv1_b, *conv2_wt, *conv2_b, *enc_pos, *lnp_w, *lnp_b;
  float *tok_emb, *dec_pos, *dln_w, *dln_b;
  _Float16* tok_emb2 = nullptr;  // tied embedding as fragment-tiled f16 pairs (wa::launch_emb_tiled)
  std::vector<wa::EncLayer> enc;
  std::vector<wa::DecLayer> dec;
  // encoder activations
  float *h1, *x, *qkv;
  _Float16 *at_d, *at_f;
  // per-clip decode state: lanes [0, n_lanes) are allocated (see wa::Lane)
  wa::Lane lanes[wa::kMaxLanes];
  int n_lanes = 1;
  const float* enc_f32 = nullptr;  // ln_post output of the last encoder pass
  // decode groups: the clips of a transcribe split over up to kMaxGroups
  // independent streams, each replaying its own step graph (see DecGroup)
  std::vector<wa::DecGroup> groups;
  int wtype = 0;     // linear weights: 0 Q4_0, 1 f16 (BASELINE config 5)
  int kv_batch = 0;  // clips of the last encoder pass (lane 0's planes valid for [0, kv_batch))
  // Cross K / V caches (capacity kv_clips clips) for transcribes of at most
  // kv_small clips -- their decode steps are launch-latency chains: one GEMV
  // launch over the caches replaces the cache-free cross-attention's four,
  // wa_kernels.hip.  kv_n: clips [0, kv_n) of the last encoder pass have
  // caches; a decode group entirely inside them reads the caches.
  int kv_clips = 0, kv_small = 0;
  int kv_n = 0;
  bool kv_alloc_ok = false;  // every layer's xk / xv allocated (cross_kv_forward)
  bool group_kv(const wa::DecGroup& g) const { return g.nb > 0 && g.b0 + g.nb <= kv_n; }
  hipStream_t own_stream = nullptr;  // encoder / encoder planes (graph capture needs a non-null stream)
  // pipelined transcribes (wa_transcribe_batches): the CU-masked stream of
  // the encoder part that runs beside a decode, its CU count, the encoder
  // layers that part covers (adapted per batch) and the last call's stats
  hipStream_t enc_stream = nullptr;
  int enc_cus = 0;
  int dev_cus = 0;  // the device's CUs (run_decode)
  int overlap_k = -1;
  int overlap_b = 0, overlap_eot = -1;  // the batch shape overlap_k was adapted to
  float pipe[4] = {0, 0, 0, 0};
  // units of exactly two / of three batches the last wa_transcribe_batches decoded together
  int pipe_pairs = 0, pipe_units3 = 0;
  // Activation-range guard.  Every internal producer writes MFMA operands as
  // f16 pairs of x * 2^4 (wq4_device.hpp split_act), finite for |x| < 4094;
  // beyond that the f16 half overflows and the clip's logits become inf /
  // NaN.  The pick kernels set *range_flag on any non-finite logit.  After a
  // flagged transcribe the model retries it one range tier up (wa_transcribe;
  // sticky for the model); flagged at the last tier -> WQ4_ERANGE, never NaN
  // tokens.
  int* range_flag = nullptr;
  int range_tier = 0;
  // tier 1: the LayerNorm fold is off (the fold feeds the RAW residual stream
  // x * gamma to the MFMAs, where the LayerNorm path feeds LayerNorm(x),
  // bounded by sqrt(D) |gamma| + |beta|).
  bool fold_allowed() const { return range_tier < 1; }
  // tier 2: the encoder and decoder FFNs run as Q4FFN::forward at the ABI
  // (wq4_ffn_forward_ws: LayerNorm output in f32, fc1 + GELU to f32, each
  // GEMM operand scaled by a power of two picked per call from its max |x|),
  // so fc1 / GELU outputs of any f32-finite size reach fc2 finite.
  // Workspaces allocated when the tier is entered: ffn_ws for the encoder's
  // B * T rows, g.ffn_ws per decode group.
  bool abi_ffn() const { return range_tier >= 2; }
  // tier 3: every attention output (encoder self-attention, decoder self- and
  // cross-attention) is written as f32 rows instead of the f16-pair operand,
  // and the output projections run as Q4Linear::forward at the ABI
  // (wq4_linear_forward_ws: per-call operand scale).  Scratch: m->h1 (free
  // during the encoder layers) / g.hid, with the layer's own A-tiled buffer
  // as the ABI workspace.
  bool f32_attn() const { return range_tier >= 3; }
  void* ffn_ws = nullptr;
  size_t ffn_ws_bytes = 0;
  // The prefill of prompted calls (wa_prompt.cpp): activations for bmax *
  // n_text_ctx rows.  They borrow the encoder's buffers, idle while a
  // sequential call decodes -- x / q / hid in h1, qkv in qkv, the two A-tiled
  // operands in at_f (m->x and m->at_d stay: they feed the K / V GEMMs) -- and
  // the groups of a call run their prefills one after another.  tok: the
  // right-aligned prompt ids; xk / xv: one layer's cross-attention K / V of
  // the clips of a group without the few-clip caches (allocated when first
  // needed).
  struct Prefill {
    bool ok = false;
    float *x = nullptr, *qkv = nullptr, *q = nullptr, *hid = nullptr;
    _Float16 *atd = nullptr, *atf = nullptr;
    int* tok = nullptr;
    float *xk = nullptr, *xv = nullptr;
  } pf;
  // Token alignment (wa_align.cpp; allocated by the first wa_align,
  // ensure_align): w, the weights of one pass of kAlignHeadsPerPass heads
  // [pass head][bmax][n_text_ctx][fld] f32; msum, their filtered head mean
  // [bmax][n_text_ctx][fld] f32; the DTW's trace bytes [bmax][n_text_ctx]
  // [n_audio_ctx + 1]; per-clip F, first matrix row, N, the heads of a pass and
  // the jump frames [bmax][n_text_ctx].  heads: the (layer, head) pairs in the
  // caller's order (empty: every head of the upper half of the layers).
  struct Align {
    bool ok = false;
    int fld = 0;
    float *w = nullptr, *msum = nullptr;
    uint8_t* trace = nullptr;
    int *F = nullptr, *row0 = nullptr, *N = nullptr, *heads = nullptr, *jump = nullptr;
    std::vector<std::pair<int, int>> pairs;
    float timings[4] = {0, 0, 0, 0};  // encoder, prefill with capture, DTW, total (ms) of the last wa_align
  } al;
  // Beam search (wa_beam.cpp; allocated by the first wa_transcribe_beam,
  // all or nothing): the pairs of beam_topk, the live sums, parents, the two
  // ancestor tables, the fed tokens per cache slot and the finished lists
  // (wa::BeamSelect), sized for bmax rows, kBeamMaxCand candidates, n_text_ctx.
  struct Beam {
    bool ok = false;
    int *top_tok = nullptr, *parent = nullptr, *anc = nullptr, *fed = nullptr;
    float *top_lp = nullptr, *S = nullptr, *fin_sum = nullptr;
    int *fin_len = nullptr, *fin_anc = nullptr, *fin_n = nullptr, *complete = nullptr, *ticket = nullptr;
  } bm;
  float timings[5] = {0, 0, 0, 0, 0};
  // every group's score / timestamp / sampling buffers are allocated
  // (prepare_call: by the first call in that mode, all or nothing)
  bool score_alloc_ok = false, ts_alloc_ok = false, sample_alloc_ok = false;
  int ts0() const { return cfg.no_timestamps_token() + 1; }  // <|0.00|>
  // Suppress-token lists (wa_model_set_suppress): the caller's ids and the two
  // device masks of wa::sup_mask_words(n_vocab) words each, `always` and
  // `always | first` (one allocation, made by the first set and kept); both
  // null while no list is set.  Every pick kernel takes the mask of its pick:
  // pick 0 of a clip the union, later picks `always`.
  std::vector<int32_t> sup_always, sup_first;
  uint32_t* sup_buf = nullptr;
  const uint32_t *sup_mask = nullptr, *sup_mask0 = nullptr;
  // The captured step graphs bake the mask pointers (and with them the
  // kernels' instantiations) in: a set or a clear drops every one of them.
  void drop_graphs() {
    for (auto& g : groups) {
      if (g.graph) (void)hipGraphExecDestroy(g.graph);
      g.graph = nullptr;
      g.graph_key = -1;
      for (auto& k : g.kept) {
        if (k.exec) (void)hipGraphExecDestroy(k.exec);
        k = wa::DecGroup::KeptGraph{};
      }
      if (g.beam_graph) (void)hipGraphExecDestroy(g.beam_graph);
      g.beam_graph = nullptr;
    }
  }
  // live kernel timing (wa_profile_*)
  struct Pending {
    hipEvent_t a, b;
    int cat;
    double gflop, gb;
  };
  bool profile = false;
  std::vector<Pending> pending;
  double prof[WA_PROF_CATEGORIES][4] = {};

  void resolve_profile() {
    for (auto& p : pending) {
      float ms = 0.0f;
      if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
        prof[p.cat][0] += 1;
        prof[p.cat][1] += ms;
        prof[p.cat][2] += p.gflop;
        prof[p.cat][3] += p.gb;
      }
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
    pending.clear();
  }

  ~wa_model() {
    resolve_profile();
    for (auto& g : groups) {
      if (g.graph) (void)hipGraphExecDestroy(g.graph);
      if (g.beam_graph) (void)hipGraphExecDestroy(g.beam_graph);
      for (auto& k : g.kept)
        if (k.exec) (void)hipGraphExecDestroy(k.exec);
      if (g.st) (void)hipStreamDestroy(g.st);
      if (g.host_ndone) (void)hipHostFree(g.host_ndone);
    }
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (enc_stream) (void)hipStreamDestroy(enc_stream);
    for (auto& l : enc)
      for (wq4_tensor* t : {l.qkv, l.out, l.fc1, l.fc2}) wq4_tensor_destroy(t);
    for (auto& l : dec)
      for (wq4_tensor* t : {l.qkv, l.out, l.cq, l.cout, l.fc1, l.fc2, l.ck, l.cv}) wq4_tensor_destroy(t);
  }
};

namespace wa {

// ---- wa_weights.cpp
Config preset(int variant);
// Where the weights come from: the synthetic generator (no checkpoint is
// available offline) or a GGUF file (loader.rs).  Names are the GGUF names.
struct Source {
  virtual ~Source() = default;
  // n f32 values of `name`; false (no error) when an optional tensor is absent
  virtual bool f32(const std::string& name, int64_t n, float lo, float hi, bool optional, std::vector<float>& out) = 0;
  // the [rows, k] linear weight `name` in raw GGUF form written at dst: Q4_0
  // blocks (wtype 0) or f16 halves (wtype 1, config 5)
  virtual bool linear(const std::string& name, int rows, int k, int wtype, uint8_t* dst) = 0;
  std::string err;
};
std::unique_ptr<Source> synth_source(uint64_t seed);
std::unique_ptr<Source> gguf_source(const GgufFile& f);
// conv weight [N][C][3] (the reference's layout, loader.rs:254-268) ->
// launch_conv_gelu's [N][kk*C + c] (im2col order, layers.rs:118-121)
std::vector<float> conv_weight_im2col(const float* w, int N, int C);
wq4_status build_model(wa_model* m, Source& src);
wq4_status build_ln_fold(wa_model* m);

// ---- wa_forward.cpp
void kv_config(wa_model* m, int max_batch);
wq4_status alloc_activations(wa_model* m);
wq4_status ensure_ffn_ws(wa_model* m);
wq4_status prepare_call(wa_model* m, const DecodeCall& call);  // the device, and the buffers the call's mode needs
int decode_groups(int B);
wq4_status encoder_front(wa_model* m, const float* mel, int B, hipStream_t st);
wq4_status encoder_layers(wa_model* m, int B, int l0, int l1, hipStream_t st);
wq4_status encoder_post(wa_model* m, int B, hipStream_t st, float* enc_out_f32);
wq4_status encoder_forward(wa_model* m, const float* mel, int B, hipStream_t st, float* enc_out_f32);
wq4_status cross_kv_forward(wa_model* m, int B, hipStream_t st, bool caches, int lane = 0);
int ensure_lanes(wa_model* m, int want);
wq4_status decoder_forward(wa_model* m, DecGroup& g, const DecodeCall& call, const int* tokens, int Tq,
                           const DecodeState* state, int pos0, int kv0, hipStream_t st);
wq4_status prompt_group(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st);
wq4_status ensure_graph(wa_model* m, DecGroup& g, const DecodeCall& call);
// the SOT-position scores of prompt_group (wa_prompt.cpp takes them at ragged rows)
wq4_status score_sot(wa_model* m, DecGroup& g, const float* z0, const int* lang_idx, int lang_stride, int lang_fixed,
                     hipStream_t st);

// ---- wa_prompt.cpp
// The arguments of a prompted call (null pointers, n_tokens in [1, ld], ids in
// [0, n_vocab), max n_tokens + max_tokens <= n_text_ctx), on the host.
wq4_status check_prompt(const wa_model* m, const wa_prompt* p, int n_clips, int max_tokens);
wq4_status ensure_prefill(wa_model* m);
// The prompt pass of group g over the call's prompts: right-aligns them to the
// group's longest, P, runs the decoder over all P rows of every clip (self-K/V
// into the caches at slots pad .. P - 1), leaves the last position's logits in
// g.logits and, a scored call, the SOT-position scores; *P_out = P.
wq4_status prefill_group(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st, int* P_out);

// ---- wa_align.cpp
// The capture of an alignment call after layer li's cq GEMM (prefill_group):
// weights + filter of the layer's alignment heads over pf.q and the layer's
// head-major K, kAlignHeadsPerPass heads at a time.  *done: no later layer has
// alignment heads.
wq4_status align_layer(wa_model* m, DecGroup& g, int li, const float* xk, int P, hipStream_t st, bool* done);
// the rows [row0, row0 + N) x [0, F) of a clip's head mean msum [.][fld] -> dst [.][dst_ld], on st
hipError_t copy_matrix(const float* msum, int fld, int row0, int N, int F, float* dst, int dst_ld, hipStream_t st);

// ---- wa_transcribe.cpp
bool bad_temperatures(const float* t, int n);  // one is negative or not finite
// sizes, in order, of the units a call over NB batches decodes at up to `width` batches at once
std::vector<int> unit_sizes(int NB, int width);
// The ladder of wa_transcribe_fallback on checked arguments and a prepared
// sampled call (wa_long.cpp runs it per round).
wq4_status transcribe_ladder(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips,
                             const wa_fallback* fb, int32_t* tokens_out, int32_t* n_tokens_out,
                             const wa_scores* scores, int32_t* rung_out, void* stream);
// wa_transcribe's argument check (wa_prompt.cpp's entries share it)
wq4_status check_args(const wa_model* m, bool ptrs_ok, int n_batches, int max_tokens, int n_clips,
                      const float* temps = nullptr, const int* rungs = nullptr);
// one range tier up after a flagged run; WQ4_ERANGE at the last
wq4_status raise_tier(wa_model* m);
// a transcribe through the range tiers
wq4_status transcribe_tiers(wa_model* m, const DecodeCall& call, const float* mel_dev, int n_clips,
                            int32_t* tokens_out, int32_t* n_tokens_out, void* stream, const wa_scores* scores);

}  // namespace wa
