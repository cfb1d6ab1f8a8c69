// wa_pick.hpp -- launchers of the decoder's output end (wa_pick.hip): the
// logits, the token pick of every decoding mode, the greedy loop's bookkeeping.
// Reference semantics: src/model/{decoder,whisper}.rs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "wa_kernels.hpp"  // DecodeState

namespace wa {

// logits[b, v] = h[b * ldh] . E[v]  (decoder.rs:289-292, 342-343), f32
// products and accumulation (v_mfma_f32_32x32x2_f32).
hipError_t launch_logits(const float* h, int B, int D, long ldh, const float* emb, int V, float* logits,
                         hipStream_t st);

// Greedy pick per clip (whisper.rs:119-124, 131-138): argmax with the LAST
// maximum winning ties (Rust max_by), EOT (50257) masked when suppress != 0,
// or restricted to [lo, hi) for language detection (whisper.rs:76-83).
// Writes out_tok[b * out_stride].
// range_flag (nullable): set to 1 when a logit of [lo, hi) is not finite --
// an MFMA operand left the f16-pair range somewhere upstream (the
// overflow propagates to every logit of the clip); wa_transcribe checks it.
// sup (nullable, here and in every launcher below): the suppress mask of the
// pick (next section); its ids count as -inf before anything else.
hipError_t launch_argmax(const float* logits, int B, int V, int lo, int hi, int suppress_eot, int* out_tok,
                         int out_stride, int* range_flag, hipStream_t st, const uint32_t* sup = nullptr);
// Step-dependent EOT suppression (whisper.rs:120-122) folded into argmax:
// suppress iff state->step < min_tokens - 1 (state->step already advanced).
hipError_t launch_argmax_step(const float* logits, int B, int V, int min_tokens, const DecodeState* state,
                              int* out_tok, int* range_flag, hipStream_t st, const uint32_t* sup = nullptr);

// ---- suppress-token lists (wa_model_set_suppress) -------------------------
// OpenAI Whisper's SuppressTokens / SuppressBlank as a bit mask over the
// vocabulary: bit (id & 31) of word id >> 5 set = the id reads as -inf in the
// row a pick or a top-k sees, ahead of the EOT and timestamp masks.  A model
// holds two, `always` (picks >= 1) and `always | first` (pick 0), each
// sup_mask_words(V) words: the bits of emb_tiled_rows(V) ids, so the fused
// kernel's padded rows read in range.  The range flag is raised from the raw
// logits: a suppressed id that is not finite still counts.
int64_t sup_mask_words(int V);
// The mask of `ids` (n of them, each in [0, V)): sup_mask_words(V) words.
void sup_mask_build(const int32_t* ids, int n, int V, uint32_t* words);

// ---- timestamp decoding (wa_transcribe_timestamps) ----------------------
// OpenAI Whisper's ApplyTimestampRules, per row, as a record the bookkeeping
// kernel keeps on the device (ts0 = no_timestamps + 1, the id of <|0.00|>):
//   history (what the sampled tokens s so far decide)
//     last    s[-1] is a timestamp            penult  len(s) < 2 or s[-2] is one
//     t_last  the last timestamp in s, -1: none      first   len(s) == 0
//   masks derived from it, read by the pick kernels (ts_masked, wa_pick.hip)
//     ids >= ts0        allowed inside [ts_lo, ts_hi] only
//     ids in (EOT, ts0) never (the specials)
//     EOT               unless first, or the step suppresses it (whisper.rs:97-98, 120-122)
//     ids < EOT         when text_ok
// The allowed set is never empty: the first pick keeps [ts0, ts_hi] with
// ts_hi >= ts0; after two timestamps (or one as the only token) every text id
// stays; after text + timestamp [t_last, V) stays and t_last <= V - 1;
// otherwise every text id stays.
struct TsRule {
  int text_ok, ts_lo, ts_hi, first;
  int last, penult, t_last, pad;
};
// The record of an empty history: max_initial < 0 leaves the first timestamp unbounded.
TsRule ts_rule_first(int ts0, int V, int max_initial);
// The record after `tok` is appended to the history `r` describes.
TsRule ts_rule_next(const TsRule& r, int tok, int ts0, int V);

// ---- temperature sampling (wa_transcribe_sampled) -------------------------
// Gumbel-max over counter-based noise, all integer arithmetic uint64 and
// wrapping, mix = splitmix64's finaliser:
//   k(seed, pick)    = mix(seed + 0x9E3779B97F4A7C15 * (pick + 1))
//   h(seed, pick, v) = mix(k ^ v) >> 41                  (23 bits)
//   u = (h + 0.5) * 2^-23   g = -log(-log(u))   key_v = fmaf(T, g, z_v)
// pick = 0 for the prompt's pick, DecodeState::step + 1 for a decode step's.
// A row with T = 0 evaluates no noise: its key is z and its pick the greedy
// one.  The pick is the largest key, the largest index among equal keys; its
// score is the untempered log softmax(z)[tok] over the masked row.
// sample_noise: u and g of ids id0 .. id0 + n - 1 on the host (either nullable).
void sample_noise(uint64_t seed, int pick, int id0, int n, float* u_out, float* g_out);

// ---- the decode step's pick ---------------------------------------------
// What the fused kernel's pick reads and writes beside the logits.  The mode
// follows from the members that are set:
//   out_lp  the pick's log-probability log softmax(z_b)[out_tok[b]] over the
//           masked row the pick sees goes to out_lp[b] (scored transcribes)
//   rules   the rows' rule records: masks a-e applied while the logits are
//           written, then the mass rule (the timestamps' logsumexp against the
//           best text logit) and the pick over the surviving side or sides;
//           ids from ts0 on are timestamps.  Needs out_lp.
//   temp    (with seed: device [B], read when the kernel runs) the Gumbel-max
//           pick at the rows' temperatures; rule f from the raw sums.  Needs
//           out_lp.
//   sup     the suppress mask, applied where lg[] is written in every mode: a
//           wave's 32 vocabulary rows are one mask word.  Null: the
//           instantiations without the mask, the kernels of a list-free model.
// Rows >= B of the outputs are not written.
struct PickArgs {
  float* scratch;  // logits_pick_scratch_floats(V) f32 / u32: the workgroups' candidates
  int* counter;    // one int zeroed once (re-armed by the kernel)
  int* out_tok;
  float* out_lp;
  int* out_mass;  // nullable, read with rules: 1 where the mass rule masked the text side of row b
  const TsRule* rules;
  int ts0;
  const float* temp;
  const uint64_t* seed;
  const uint32_t* sup;  // nullable: the `always` suppress mask (the kernel runs picks >= 1 only)
};
int logits_argmax_groups(int V);
// Floats of PickArgs::scratch, sized for the widest mode: [side][array][32]
// [logits_argmax_groups(V)], 2 sides x 5 arrays; a mode uses the first 2
// (greedy), 3 (scored; timestamps) or 5 (sampled) arrays of its 1 or 2 sides.
int64_t logits_pick_scratch_floats(int V);
// Decode-step logits fused with the pick (launch_logits + the pick in one
// kernel, logits never stored): B <= 32 rows.
// htiled: the B hidden rows as the A-tiled operand (wq4 layout, m-tile 0,
// ns planes -- what wq4_layernorm writes with at_out); emb2: the f16-pair
// table, fragment-tiled (launch_emb_tiled); D % 128 == 0.
// trace_ids / trace_out (diagnostics; null in the product): [B][trace_s1]
// [trace_k] -- the logits of the listed ids at slot state->step + 1.
// range_flag (nullable): as launch_argmax, for every logit of the B rows.
hipError_t launch_logits_pick(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                              int min_tokens, const DecodeState* state, const PickArgs& pick, const int* trace_ids,
                              float* trace_out, int trace_s1, int trace_k, int* range_flag, hipStream_t st);
// The timestamp (temp null) or sampled pick over stored logit rows [rows][ld]
// (the prompt's pick, decode groups wider than 32 rows): rules nullable (the
// whole row one side, EOT suppression only); EOT suppressed when suppress_eot
// != 0 or, state non-null, when state->step + 1 < min_tokens; the noise's pick
// index is `pick`, or state->step + 1 when state is non-null.  out_lp /
// out_mass nullable.  (The plain and scored row picks stay launch_argmax +
// launch_row_logprob, which writes (z - m) - log s: this one's -log S differs
// in the sign of a zero.)
hipError_t launch_row_pick(const float* logits, int rows, int64_t ld, int V, int suppress_eot, int min_tokens,
                           const DecodeState* state, const TsRule* rules, int ts0, const float* temp,
                           const uint64_t* seed, int pick, int* out_tok, float* out_lp, int* out_mass,
                           int* range_flag, hipStream_t st, const uint32_t* sup = nullptr);

// Log-probability of one entry of stored logit rows (the scores outside the
// fused kernel: the prompt's pick, no-speech and language probabilities,
// decode groups wider than 32 rows): out[r * out_stride] = z[id] -
// logsumexp(z[lo:hi]), z = logits + r * ld, id = idx ? idx[r * idx_stride] :
// fixed_idx.  EOT counts as -inf when mask_eot != 0 -- or, mask_state
// non-null, when mask_state->step + 1 < min_tokens (whisper.rs:120-122).  An
// id outside [lo, hi) gives NaN.
hipError_t launch_row_logprob(const float* logits, int rows, int64_t ld, int lo, int hi, int mask_eot, int min_tokens,
                              const DecodeState* mask_state, const int* idx, int idx_stride, int fixed_idx, float* out,
                              int out_stride, hipStream_t st, const uint32_t* sup = nullptr);
// x[i] = exp(x[i]), i < n.
hipError_t launch_exp_inplace(float* x, int n, hipStream_t st);
// dst[i] = src[i * stride], i < n.
hipError_t launch_gather_int(const int* src, int stride, int* dst, int n, hipStream_t st);
// Whether the logits kernel reads a fragment-tiled table for this width.
bool emb_tiled_supported(int D);
// Rows of the fragment-tiled table (V padded to the kernel's 128-row groups).
int64_t emb_tiled_rows(int V);
// f32 [V][D] -> fragment-tiled f16 planes, chunk-major: per 128-column
// chunk c, 16-row group g (G = emb_tiled_rows(V) / 16 of them), 32-column
// step ks < 4 and plane p, the 16x16x32 MFMA operand of 64 lanes x 8 halves
// is 1 KiB contiguous at (((c * G + g) * 4 + ks) * ns + p) KiB (lane =
// 16 (k / 8 % 4) + row % 16), rows >= V zero -- every load instruction of
// the logits kernel reads 1 KiB contiguous and one chunk of the whole table
// is one contiguous stretch.  out: emb_tiled_rows(V) * ns * D halves.
hipError_t launch_emb_tiled(const float* emb, int V, int D, int ns, _Float16* out, hipStream_t st);

// Greedy-loop bookkeeping at the top of each step (whisper.rs:104-115):
// for every clip not yet done, EOT -> done (eot_stop != 0), else append the
// next token; then advance position / kv_len / step.
// next_lp / logprob (both or neither; scored transcribes): next_lp[b], the
// log-probability of next_tok[b], is stored beside the token in logprob [B]
// [max_tokens + 1]; the EOT pick that ends a clip leaves its own in the slot
// after the last token.
// rules (nullable; timestamp transcribes): every row's rule record advances
// by its next token (ts0, V: as ts_rule_next).
hipError_t launch_bookkeep(const int* next_tok, const float* next_lp, int* tokens, float* logprob, int* n_tokens,
                           int* done, int B, int max_tokens, int eot_stop, DecodeState* state, TsRule* rules, int ts0,
                           int V, hipStream_t st);

}  // namespace wa
