// wa_kernels.hpp -- launchers of the Whisper model kernels around the Q4 path
// (LayerNorm, attention, conv front-end, embedding, logits, greedy argmax).
// Reference semantics: src/model/{layers,attention,encoder,decoder,whisper}.rs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace wa {

// Device-resident decode state (read by kernels, advanced on the device so a
// captured step graph can be replayed without host involvement).
struct DecodeState {
  int position;  // positional-embedding index of the current token
  int kv_len;    // entries in the self-attention KV cache before this step
  int step;      // greedy-loop step index (whisper.rs:104)
  int n_done;    // clips that have emitted EOT
};

// Encoder self-attention (attention.rs:243-298, non-causal), flash-style,
// f32 MFMA.  qkv: [B*T, 3D] f32 (q | k | v).  Writes the A-tiled operand of
// the output projection (rows b*T + t, K = D) -- or, with out32 non-null
// (range tier 3, wa_model), f32 rows [B*T][D] there instead.  The same holds
// for every attention launcher below.
hipError_t launch_encoder_attention(const float* qkv, int B, int T, int H, _Float16* tiled, int ns,
                                    hipStream_t st, float* out32 = nullptr);

// Decoder self-attention with KV cache (attention.rs:62-125).  qkv [B*Tq, 3D];
// appends k, v of the Tq new tokens at cache index kv_len (+ kv_base_extra)
// and attends over kv_len + Tq entries, causal inside the new tokens when
// Tq > 1 (attention.rs:270-287).  cache_k/v: [B, ctx, D].
hipError_t launch_decoder_self_attention(const float* qkv, float* cache_k, float* cache_v, int B, int Tq, int H,
                                         int ctx, const DecodeState* state, int kv_len_host, _Float16* tiled,
                                         int ns, hipStream_t st, float* out32 = nullptr);

// Cross-attention over cached K / V (attention.rs:177-236, the reference's
// form; used for decode groups of a few clips): q [B*Tq, D] f32, k / v
// head-major [B][H][T][64] f32 (wq4_gemm_tiled_headmajor of the encoder
// output), Tq <= 4; part: cross_attention_kv_part_floats floats, counters:
// B * H ints zeroed once (re-armed by the kernel).  Writes the A-tiled
// operand of the output projection.
int cross_attention_kv_splits(int T);
size_t cross_attention_kv_part_floats(int B, int H, int T);
hipError_t launch_cross_attention_kv(const float* q, const float* k, const float* v, int B, int Tq, int T, int H,
                                     float* part, int* counters, _Float16* tiled, int ns, hipStream_t st,
                                     float* out32 = nullptr);

// Cross-attention over the encoder output (wa_xattn.hip; attention.rs:
// 204-298 restated without K/V caches): q [B*Tq, D] f32 (rows b*Tq + i),
// wk / wv: the layer's raw key / value weights [D, D] (wtype: Q4_0 blocks or
// f16), bv: value bias, enc: [B][T][ns][D] f16 planes (launch_enc_planes),
// qt: [B*Tq][ns][ceil16(H)][D] f16 scratch zeroed once, part:
// xattn_part_floats floats.  Writes the A-tiled operand of the output
// projection.  Needs D == 64 * H, D % 128 == 0, D <= 1280.
struct XattnPlan {
  int splits;  // frame ranges per query row (workgroups per row)
  int ch;      // 16-frame sub-chunks per range
};
// The frame split of a decode (wa_xattn.hip): rows = the rows of the largest
// concurrently decoding group, free_cus = the CUs the decode has while a
// CU-masked stream runs beside it (<= 0: nothing beside it, no bound).
// force_splits < 0: the product's rule (WA_XATTN_SPLITS_RT overrides it, A/B
// runs and tests only), 0: the rule alone, > 0: that many splits (normalised).
XattnPlan xattn_plan(int T, int rows = 1, int free_cus = 0, int force_splits = -1);
// sized for every plan of up to the maximum (8) splits
size_t xattn_part_floats(int R, int H, int D, int T);
// Q4_0 Wv repacked once at model load into the cross-attention
// projection's lane order (same bytes; wv_pack_words u32 words).
size_t wv_pack_words(int H, int D);
hipError_t launch_wv_pack(const uint8_t* wv, int H, int D, uint32_t* out, hipStream_t st);
// Infinity Cache residency of the encoder planes: of every kXattnResDen
// consecutive 16-frame sub-chunks of a clip, q load with the default cache
// policy (and stay on-die from one decoder layer to the next), the others
// nontemporal.  q = kXattnResDen: everything default.  Values never change.
constexpr int kXattnResDen = 64;
struct XattnResidency {
  int q = kXattnResDen;
};
// The one predicate of every kernel that reads the planes: a fixed function
// of the clip's sub-chunk index (never of step, layer, group or split), so a
// line always loads with the same policy.  Residents are evenly interleaved:
// any n consecutive sub-chunks hold floor or ceil(n q / 64) of them, so every
// (row, split) workgroup of a launch walks the same mix.
constexpr bool xattn_chunk_resident(int chunk, int q) { return ((chunk * q) & (kXattnResDen - 1)) + q >= kXattnResDen; }
// The share for a decode whose concurrently running groups stream the planes
// of live_clips clips in all ([T][ns][D] f16 each); budget_mb < 0: the
// product's rule, else a budget in MB (10^6 bytes) that replaces it.
XattnResidency xattn_residency(int live_clips, int T, int ns, int D, double budget_mb = -1.0);
// wvp: the launch_wv_pack words of wv (Q4 weights; ignored for f16 weights).
// plan: an xattn_plan of T (no empty split, at most the maximum splits).
hipError_t launch_xattn(const float* q, const uint8_t* wk, const uint8_t* wv, const uint32_t* wvp, const float* bv,
                        int wtype, const _Float16* enc, int B, int Tq, int T, int H, int D, _Float16* qt, float* part,
                        _Float16* tiled, int ns, XattnResidency res, XattnPlan plan, hipStream_t st,
                        float* out32 = nullptr);
// A-tiled operand [R][K] (hi + lo) -> f32 rows (diagnostics).
hipError_t launch_untile(const _Float16* tiled, int R, int K, int ns, float* out, hipStream_t st);
// f32 rows [rows][D] -> [rows][ns][D] f16 planes (hi | lo) for launch_xattn.
hipError_t launch_enc_planes(const float* x, int64_t rows, int D, int ns, _Float16* out, hipStream_t st);

// Conv1D (layers.rs:77-132) as an implicit-im2col f32 MFMA GEMM + bias +
// GELU (encoder.rs:89-94) (+ pos[t] if pos != nullptr).  Input element
// (b, c, t) at in[b*in_bs + c*in_cs + t*in_ts]; output [B, T_out, N].
// w_t: weights re-laid as [N][3*C] with k = kk*C + c.
hipError_t launch_conv_gelu(const float* in, long in_bs, long in_cs, long in_ts, int B, int C, int T_in,
                            int stride, const float* w_t, const float* bias, const float* pos, int N, float* out,
                            hipStream_t st);

// x[b*Tq + t] = tok_emb[tokens[b*Tq + t]] + pos_emb[pos0 + t]   (decoder.rs:326-343)
// pos0 = state ? state->position : pos0_host.
hipError_t launch_embed(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                        const DecodeState* state, int pos0_host, float* x, hipStream_t st);

// launch_embed + the LayerNorm-fold producer for gamma (wq4_gemm_tiled_lnfold):
// also writes at = A-tiled x * gamma and stats [rows][D/32][2]; D % 32 == 0.
hipError_t launch_embed_fold(const int* tokens, const float* tok_emb, const float* pos_emb, int B, int Tq, int D,
                             const DecodeState* state, int pos0_host, float* x, const float* gamma, _Float16* at,
                             float* stats, int ns, hipStream_t st);

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
hipError_t launch_argmax(const float* logits, int B, int V, int lo, int hi, int suppress_eot,
                         const DecodeState* state, int* out_tok, int out_stride, int* range_flag, hipStream_t st);

// Decode-step logits fused with the greedy pick (launch_logits +
// launch_argmax_step in one kernel, logits never stored): B <= 32 rows,
// D % 8 == 0; pval / pidx: 32 * logits_argmax_groups(V) scratch each,
// counter: one int zeroed once (re-armed by the kernel).
int logits_argmax_groups(int V);
// htiled: the B hidden rows as the A-tiled operand (wq4 layout, m-tile 0,
// ns planes -- what wq4_layernorm writes with at_out); emb2: the f16-pair
// table, fragment-tiled (launch_emb_tiled); D % 128 == 0.
// trace_ids / trace_out (diagnostics; null in the product): [B][trace_s1]
// [trace_k] -- the logits of the listed ids at slot state->step + 1.
// range_flag (nullable): as launch_argmax, for every logit of the B rows.
hipError_t launch_logits_argmax(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                                int min_tokens, const DecodeState* state, float* pval, int* pidx, int* counter,
                                int* out_tok, const int* trace_ids, float* trace_out, int trace_s1, int trace_k,
                                int* range_flag, hipStream_t st);
// The same launch for a scored transcribe (wa_transcribe_scored): the kernel's
// SCORE = 1 instantiation also writes out_lp[b] = log softmax(z_b)[out_tok[b]]
// = -log sum_v exp(z_b[v] - max z_b) over the masked row the pick sees, from
// per-workgroup partial sums in psum (a third 32 * logits_argmax_groups(V)
// scratch array beside pval / pidx).  Rows >= B of out_lp are not written.
hipError_t launch_logits_argmax_scored(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                                       int min_tokens, const DecodeState* state, float* pval, int* pidx, float* psum,
                                       int* counter, int* out_tok, float* out_lp, const int* trace_ids,
                                       float* trace_out, int trace_s1, int trace_k, int* range_flag, hipStream_t st);
// Log-probability of one entry of stored logit rows (the scores outside the
// fused kernel: the prompt's pick, no-speech and language probabilities,
// decode groups wider than 32 rows): out[r * out_stride] = z[id] -
// logsumexp(z[lo:hi]), z = logits + r * ld, id = idx ? idx[r * idx_stride] :
// fixed_idx.  EOT counts as -inf when mask_eot != 0 -- or, mask_state
// non-null, when mask_state->step + 1 < min_tokens (whisper.rs:120-122).  An
// id outside [lo, hi) gives NaN.
hipError_t launch_row_logprob(const float* logits, int rows, int64_t ld, int lo, int hi, int mask_eot, int min_tokens,
                              const DecodeState* mask_state, const int* idx, int idx_stride, int fixed_idx, float* out,
                              int out_stride, hipStream_t st);
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
hipError_t launch_bookkeep(const int* next_tok, int* tokens, int* n_tokens, int* done, int B, int max_tokens,
                           int eot_stop, DecodeState* state, hipStream_t st);

// The same for a scored transcribe: next_lp[b], the log-probability of
// next_tok[b], is stored beside the token in logprob [B][max_tokens + 1]; the
// EOT pick that ends a clip leaves its own in the slot after the last token.
hipError_t launch_bookkeep_scored(const int* next_tok, const float* next_lp, int* tokens, float* logprob,
                                  int* n_tokens, int* done, int B, int max_tokens, int eot_stop, DecodeState* state,
                                  hipStream_t st);

// Step-dependent EOT suppression (whisper.rs:120-122) folded into argmax:
// suppress iff state->step < min_tokens - 1 (state->step already advanced).
hipError_t launch_argmax_step(const float* logits, int B, int V, int min_tokens, const DecodeState* state,
                              int* out_tok, int* range_flag, hipStream_t st);

// ---- timestamp decoding (wa_transcribe_timestamps) ----------------------
// OpenAI Whisper's ApplyTimestampRules, per row, as a record the bookkeeping
// kernel keeps on the device (ts0 = no_timestamps + 1, the id of <|0.00|>):
//   history (what the sampled tokens s so far decide)
//     last    s[-1] is a timestamp            penult  len(s) < 2 or s[-2] is one
//     t_last  the last timestamp in s, -1: none      first   len(s) == 0
//   masks derived from it, read by the pick kernels (ts_masked, wa_kernels.hip)
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

// The timestamp form of launch_logits_argmax_scored: masks a-e of the rule
// applied while the logits are written, then the mass rule (the timestamps'
// logsumexp against the best text logit) and the pick in the last-arriving
// workgroup.  pval / pidx / psum carry the text side (ids < ts0), xval / xidx
// / xsum (three more 32 * logits_argmax_groups(V) arrays) the timestamp side.
// out_lp[b]: the pick's log-probability over the finally masked row.
// out_mass (nullable): 1 where the mass rule masked the text side of row b.
hipError_t launch_logits_argmax_ts(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                                   int min_tokens, const DecodeState* state, const TsRule* rules, int ts0,
                                   float* pval, int* pidx, float* psum, float* xval, int* xidx, float* xsum,
                                   int* counter, int* out_tok, float* out_lp, int* out_mass, const int* trace_ids,
                                   float* trace_out, int trace_s1, int trace_k, int* range_flag, hipStream_t st);
// The same rule over stored logit rows [rows][ld] (the prompt's pick, decode
// groups wider than 32 rows): EOT suppressed when suppress_eot != 0 or, state
// non-null, when state->step + 1 < min_tokens.
hipError_t launch_row_timestamp(const float* logits, int rows, int64_t ld, int V, int suppress_eot, int min_tokens,
                                const DecodeState* state, const TsRule* rules, int ts0, int* out_tok, float* out_lp,
                                int* out_mass, int* range_flag, hipStream_t st);
// launch_bookkeep_scored that also advances every row's rule record by its next token.
hipError_t launch_bookkeep_ts(const int* next_tok, const float* next_lp, int* tokens, float* logprob, int* n_tokens,
                              int* done, int B, int max_tokens, int eot_stop, DecodeState* state, TsRule* rules,
                              int ts0, int V, hipStream_t st);

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
// Floats of the sampled fused launch's scratch block `scr`.
int64_t logits_sample_scratch_floats(int V);
// The sampled form of launch_logits_argmax_scored (rules null) or of
// launch_logits_argmax_ts (rules non-null: masks a-e as there, rule f from the
// raw sums, the pick over the surviving side or sides): temp / seed device
// [B], read when the kernel runs; scr: logits_sample_scratch_floats(V) floats
// (per side and workgroup the key candidate with its raw logit, the raw
// maximum and the exp sum relative to it).
hipError_t launch_logits_argmax_sample(const _Float16* htiled, int B, int D, const _Float16* emb2, int ns, int V,
                                       int min_tokens, const DecodeState* state, const float* temp,
                                       const uint64_t* seed, const TsRule* rules, int ts0, float* scr, int* counter,
                                       int* out_tok, float* out_lp, int* out_mass, const int* trace_ids,
                                       float* trace_out, int trace_s1, int trace_k, int* range_flag, hipStream_t st);
// The same over stored logit rows [rows][ld] (the prompt's pick, decode groups
// wider than 32 rows): pick index `pick`, or state->step + 1 when state is
// non-null; EOT suppression as launch_row_timestamp.
hipError_t launch_row_sample(const float* logits, int rows, int64_t ld, int V, int suppress_eot, int min_tokens,
                             const DecodeState* state, const TsRule* rules, int ts0, const float* temp,
                             const uint64_t* seed, int pick, int* out_tok, float* out_lp, int* out_mass,
                             int* range_flag, hipStream_t st);

}  // namespace wa
