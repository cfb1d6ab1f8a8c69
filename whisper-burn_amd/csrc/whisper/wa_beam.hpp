// wa_beam.hpp -- launchers of the beam-search kernels (wa_beam.hip, and the
// ancestor-table self-attention beside the kernel it mirrors in
// wa_kernels.hip).  Semantics: include/whisper_amd.h, "Beam search".
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "wa_kernels.hpp"
#include "wa_pick.hpp"  // TsRule

namespace wa {

constexpr int kBeamMaxK = 8;      // beams per clip
constexpr int kBeamMaxCand = 16;  // finished sequences kept per clip
constexpr int kBeamMaxTop = kBeamMaxK + 1;

// Per-row log-softmax and top-kp (kp = K + 1 <= 9) of stored logit rows
// [rows][V] f32 (row stride ld): one workgroup per row, one pass -- every
// thread keeps an online (max, sum exp) and its own sorted top 9, then the
// workgroup merges both in a fixed order.  EOT is -inf when state ?
// state->step + 1 < min_tokens : suppress_fixed, and always when !eot_stop.
// Larger lp first, equal lp: larger id first.  out_tok / out_lp: [rows][kp].
// A non-finite raw logit sets *range_flag.  Needs V >= 16.
// sup (nullable, both launchers): the pick's suppress mask (wa_pick.hpp); its
// ids are -inf before the online (m, s) and the lists -- under the rules
// together with masks a-e, before rule f.
hipError_t launch_beam_topk(const float* logits, int rows, int64_t ld, int V, int kp, int suppress_fixed, int min_tokens,
                            int eot_stop, const DecodeState* state, int* out_tok, float* out_lp, int* range_flag,
                            hipStream_t st, const uint32_t* sup = nullptr);

// The same under the timestamp rules (wa_transcribe_beam_ex, timestamps): row
// r's masks a-e from rules[r] (EOT also by the rule above: mask a), rule f
// decided from the row's two sides after them (logsumexp of the timestamps
// against the text side's maximum, EOT on the text side), lp the log-softmax
// over the finally masked row.  An id the rules mask is no candidate: a row
// with fewer than kp allowed ids fills the rest with (0, -inf).  out_mass
// (nullable) [rows]: 1 where rule f fired.  ts0 in (EOT, V].
hipError_t launch_beam_topk_rules(const float* logits, int rows, int64_t ld, int V, int kp, int suppress_fixed,
                                  int min_tokens, int eot_stop, const DecodeState* state, const TsRule* rules, int ts0,
                                  int* out_tok, float* out_lp, int* out_mass, int* range_flag, hipStream_t st,
                                  const uint32_t* sup = nullptr);

// Everything beam_select reads and writes, device pointers.  rows = n_clips *
// K; row clip * K + j is beam j of its clip.
struct BeamSelect {
  const int* top_tok;   // [rows][K + 1]   beam_topk's pairs
  const float* top_lp;  // [rows][K + 1]
  float* S;             // [rows]          sums of the live beams, in place
  int* next_tok;        // [rows]          the token each new beam feeds to the next step
  int* parent;          // [rows]          the row each new beam continues
  int* anc;             // [2][rows][ctx]  ancestor tables; the live one is ((step + 1) & 1)
  int* fed;             // [ctx][rows]     fed[slot][row]: the token row fed at cache slot `slot`
  float* fin_sum;       // [n_clips][C]    finished sequences: sum of log-probabilities,
  int* fin_len;         // [n_clips][C]      tokens (EOT not counted),
  int* fin_anc;         // [n_clips][C][ctx] and the ancestor row of every slot
  int* fin_n;           // [n_clips]
  int* complete;        // [n_clips]       sticky
  int* ticket;          // [1]             arrival counter, zero between launches
  DecodeState* state;   // advanced by the last workgroup to arrive
  TsRule* rules;        // [rows]          nullable: the rows' timestamp rule records, in place
};
// One workgroup per clip: ranks the clip's K (K + 1) candidates (score =
// S[j] + lp in f32; score descending, then source beam, then rank, both
// ascending; -inf dropped), keeps the first K non-EOT ones as the next beams,
// files the EOT ones met on the way (while the clip holds fewer than C and is
// not complete), copies the ancestor rows into the other table and -- what
// launch_bookkeep does for a greedy step -- advances position / kv_len / step.
// state->n_done counts the complete clips.  With a.rules the record of new
// beam n becomes ts_rule_next(record of its parent, its token, ts0, V), every
// parent record of the clip read before any is written.
hipError_t launch_beam_select(const BeamSelect& a, int n_clips, int K, int C, int ctx, hipStream_t st, int ts0 = 0,
                              int V = 0);

// The decode step's self-attention (Tq = 1) over a reindexed cache: key j <
// kv_len of row r is read from cache row anc[r][j]; the row's new key / value
// are appended at (r, kv_len) as launch_decoder_self_attention does.  anc:
// [rows][ctx] int32; with state non-null the live table of a [2][rows][ctx]
// pair is picked by (state->step + 1) & 1.  An identity table gives the bits of
// launch_decoder_self_attention.  pad (device [rows], nullable; prompted beam
// calls): row r attends slots [pad[r], kv_len] only, the waves splitting the
// keys from pad[r] -- the bits of launch_decoder_self_attention with pad over
// physically gathered caches.
hipError_t launch_decoder_self_attention_beam(const float* qkv, float* cache_k, float* cache_v, int rows, int H,
                                              int ctx, const DecodeState* state, int kv_len_host, const int* anc,
                                              _Float16* tiled, int ns, hipStream_t st, float* out32 = nullptr,
                                              const int* pad = nullptr);

}  // namespace wa
