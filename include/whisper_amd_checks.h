/*
 * whisper_amd_checks.h -- the test side of libwhisper_amd's C ABI: one check
 * entry per kernel, each running that product kernel synchronously on
 * caller-supplied buffers in the mode its arguments select; the host-only
 * probes of the rules behind a decode's layout; and the model diagnostics the
 * parity tests compare with the oracle.  An integrator needs whisper_amd.h
 * only.  *_dev arguments are device pointers; arrays marked HOST are read on
 * the host.  Every argument an entry can see on the host is checked
 * (WQ4_EINVAL) before anything is launched.
 */
#ifndef WHISPER_AMD_CHECKS_H
#define WHISPER_AMD_CHECKS_H

#include "whisper_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- model diagnostics ---------------------------------------------------- */
/* Encoder (encoder.rs:87-115) -> encoder_out f32 [n_clips * 1500, D]. */
wq4_status wa_encode(wa_model* m, const float* mel_dev, int n_clips, float* enc_out_dev, void* stream);
/* After wa_encode: decoder forward_prompt (decoder.rs:251-296)
 * on prompt tokens [n_clips, plen] (device int32), plen <= 4, returning the
 * last-position logits [n_clips, n_vocab] (device f32). */
wq4_status wa_prompt_logits(wa_model* m, const int32_t* prompt_dev, int n_clips, int plen, float* logits_dev,
                            void* stream);
/* After wa_encode: the prefill of wa_transcribe_prompted over host prompts of
 * any lengths (checked as there, max n_tokens <= n_text_ctx), returning the
 * last-position logits [n_clips, n_vocab] (device f32).  Synchronous. */
wq4_status wa_prompt_logits_ragged(wa_model* m, const wa_prompt* prompt, int n_clips, float* logits_dev,
                                   void* stream);
/* wa_transcribe, additionally recording decode-step logits (the parity
 * tests' logit trace): trace_ids_dev / trace_out_dev are device int32 / f32
 * [n_clips][max_tokens + 1][trace_k]; the decode step that picks token s + 1
 * (s = 0 ..) writes, at slot s + 1, the logits its fused logits + greedy-pick
 * kernel computed for the listed ids (EOT already masked where
 * whisper.rs:120-122 masks it).  Slot 0 (the prompt's pick) is not written:
 * wa_prompt_logits covers it.  Synchronous; the next wa_transcribe
 * re-captures its step graphs. */
wq4_status wa_transcribe_trace(wa_model* m, const float* mel_dev, int n_clips, int lang_token, int max_tokens,
                               int eot_stop, int32_t* tokens_out, int32_t* n_tokens_out, const int32_t* trace_ids_dev,
                               int trace_k, float* trace_out_dev, void* stream);
/* The key of decode group `group`'s current step graph (-1: none): changes
 * whenever the next decode has to capture a new one. */
long long wa_decode_graph_key(const wa_model* m, int group);
/* The synthetic generator, for cross-checking with the numpy oracle. */
wq4_status wa_synth_uniform(uint64_t seed, const char* name, int64_t n, float lo, float hi, float* out);

/* ---- host-only probes of a decode's layout rules --------------------------- */
/* The rule behind wa_decode_graph_key: a mixed-radix number over the digits,
 * most significant first, mode / 8 (scored 1 + timestamps 2 + sampled 4),
 * lane / 3, b0 / 512, nb / 512, eot / 2, trace / 2, group_kv / 2,
 * range_tier / 4, splits / 16, residency / 65 -- so key % 65 is the plane
 * residency and key / 65 % 16 the frame split's splits.  -1 when a digit is
 * outside its radix (a decode then fails with WQ4_EINVAL rather than replay
 * another layout's graph). */
long long wa_decode_graph_key_check(int mode, int lane, int b0, int nb, int eot, int trace, int group_kv,
                                    int range_tier, int splits, int residency);
/* Infinity Cache residency of the encoder planes the cross-attention streams.
 * A decode whose concurrently running groups stream the planes of live_clips
 * clips ([T][planes][D] f16 each, planes 1 or 2) keeps share / 64 of every
 * clip's 16-frame sub-chunks cached (default load policy) and loads the rest
 * nontemporal: wa_xattn_resident_share returns share (64 = everything; -1 on
 * bad sizes) for a budget of budget_mb MB (10^6 bytes), or for the product's
 * rule when budget_mb < 0 (the environment variable WA_XATTN_RESIDENT_MB, for
 * A/B runs and tests, then replaces its budget: 0 = everything nontemporal,
 * large = everything default; wa_xattn_check follows it too, with its n_clips
 * live).  wa_xattn_chunk_resident: 1 when sub-chunk `chunk` (frames 16 chunk
 * ..) of a clip is resident at `share`.
 * wa_xattn_plan: the frame split of a row's T frames, `splits` workgroups of
 * chunks_per_split consecutive sub-chunks, of a decode with nothing beside it.
 * wa_xattn_plan_splits: the host rule behind it -- the split of a decode whose
 * largest concurrently decoding group has `rows` rows and whose
 * cross-attention launches may take free_cus CUs (the device's less the masked
 * encoder stream's and what is left to the decode's other groups; <= 0: no
 * bound): the most splits, up to 8, with splits * rows <= free_cus, no split
 * empty.
 * WA_XATTN_SPLITS_RT=<1..8> (A/B runs and tests) replaces the rule's count
 * where a decode's plan is decided and in wa_xattn_check, never here. */
int wa_xattn_resident_share(int live_clips, int T, int planes, int D, double budget_mb);
int wa_xattn_chunk_resident(int chunk, int share);
wq4_status wa_xattn_plan(int T, int* splits, int* chunks_per_split);
wq4_status wa_xattn_plan_splits(int T, int rows, int free_cus, int* splits, int* chunks_per_split);
/* The sizes, in order, of the units a wa_transcribe_batches over n_batches
 * batches forms when up to `width` (1 .. 3) batches decode at once.  sizes:
 * room for n_batches ints; *n_units of them are written. */
wq4_status wa_pipeline_unit_sizes(int n_batches, int width, int* sizes, int* n_units);

/* ---- attention ------------------------------------------------------------- */
/* Cross-attention of one decoder layer (attention.rs:204-298) through the
 * product kernels (wa_xattn.hip): q_dev [n_clips*Tq, 64H] f32, wk_dev /
 * wv_dev raw [64H, 64H] weights (weight_type 0: Q4_0 blocks, 1: f16), bv_dev
 * [64H], enc_dev [n_clips, T, 64H] f32 -> out_dev [n_clips*Tq, 64H] f32 (the
 * attention output before the output projection). */
wq4_status wa_xattn_check(int device, const float* q_dev, const uint8_t* wk_dev, const uint8_t* wv_dev,
                          const float* bv_dev, int weight_type, const float* enc_dev, int n_clips, int Tq, int T,
                          int H, wq4_precision prec, float* out_dev);
/* The few-clip form of the same (attention.rs:177-236 with the caches): the
 * cross-attention GEMV over cached K / V (cross_attn_kv_kernel): q_dev
 * [n_clips*Tq, 64H] f32 (Tq <= 4), k_dev / v_dev head-major [n_clips][H][T]
 * [64] f32 -> out_dev [n_clips*Tq, 64H] f32 (softmax(q K^T / 8) V per head). */
wq4_status wa_xattn_kv_check(int device, const float* q_dev, const float* k_dev, const float* v_dev, int n_clips,
                             int Tq, int T, int H, wq4_precision prec, float* out_dev);
/* Encoder self-attention (attention.rs:243-298, non-causal): qkv_dev
 * [n_clips * T, 3D] f32 (q | k | v), D = 64 H -> out_dev [n_clips * T, D] f32. */
wq4_status wa_encoder_attention_check(int device, const float* qkv_dev, int n_clips, int T, int H, wq4_precision prec,
                                      float* out_dev);
/* The decode step's self-attention with a KV cache (attention.rs:62-125):
 * qkv_dev [n_rows * Tq, 3D] (the Tq new tokens of every row), caches
 * head-major [n_rows][H][ctx][64] f32 holding kv_len entries (the new keys /
 * values are appended at kv_len), causal inside the new tokens -> out_dev
 * [n_rows * Tq, D] f32.  Tq <= 4, kv_len + Tq <= ctx <= 448.  The modes:
 *   pad (HOST [n_rows], nullable): the pad form of a prompted step; row r
 *     attends cache slots [pad[r], kv_len], 0 <= pad[r] <= kv_len.
 *   anc_dev ([n_rows][ctx] int32, nullable): the beam step's kernel, Tq = 1;
 *     key j < kv_len of row r is read from cache row anc_dev[r][j], and every
 *     entry read (j >= pad[r]) must lie in [0, n_rows).
 *   f32_out != 0: the f32-row form of range tier 3 instead of the A-tiled
 *     operand (out_dev holds f32 rows either way). */
wq4_status wa_self_attention_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                   const int32_t* anc_dev /* nullable */, const int32_t* pad /* nullable */,
                                   int n_rows, int Tq, int H, int ctx, int kv_len, wq4_precision prec, int f32_out,
                                   float* out_dev);
/* The prefill's self-attention: qkv_dev [n_clips * P, 3D] f32, pad (HOST)
 * [n_clips], each in [0, P): clip c's rows are [pad[c], P), row t attends keys
 * [pad[c], t]; K / V of those rows are copied into the head-major caches
 * [n_clips][H][ctx][64] at slots pad[c] .. P - 1 (nothing else of them is
 * written) -> out_dev [n_clips * P, D] f32 (pad rows: zeros).  P <= ctx <= 448. */
wq4_status wa_self_attention_prefill_check(int device, const float* qkv_dev, float* cache_k_dev, float* cache_v_dev,
                                           int n_clips, int P, const int32_t* pad, int H, int ctx,
                                           wq4_precision prec, float* out_dev);
/* The prefill's cross-attention: q_dev [n_clips * P, D] f32, k_dev / v_dev
 * head-major [n_clips][H][T][64] f32 -> out_dev [n_clips * P, D] f32. */
wq4_status wa_cross_attention_prefill_check(int device, const float* q_dev, const float* k_dev, const float* v_dev,
                                            int n_clips, int P, int T, int H, wq4_precision prec, float* out_dev);

/* ---- conv stem and embedding ----------------------------------------------- */
/* The conv stem's kernel (layers.rs:77-132 padding 1, kernel 3; + bias, GELU
 * of encoder.rs:89-94, + pos_dev[t] when non-null): input element (b, c, t) at
 * in_dev[b * in_bs + c * in_cs + t * in_ts] (f32, strides in elements), w_dev
 * [N][C][3] f32 (the reference's layout; re-laid for the kernel by the model
 * loader's code), bias_dev [N], pos_dev [T_out][N] or null -> out_dev [B]
 * [T_out][N] f32, T_out = (T_in - 1) / stride + 1.  stride 1 or 2, C % 4 == 0;
 * a channel-contiguous input (in_cs == 1) needs in_ts % 4 == 0 and
 * in_bs % 4 == 0. */
wq4_status wa_conv_gelu_check(int device, const float* in_dev, int64_t in_bs, int64_t in_cs, int64_t in_ts, int B,
                              int C, int T_in, int stride, const float* w_dev, const float* bias_dev,
                              const float* pos_dev, int N, float* out_dev);
/* The decoder's embedding kernels (decoder.rs:326-343): tokens (HOST)
 * [B * Tq], each in [0, V), tok_emb_dev [V][D], pos_emb_dev [ctx][D] -> x_dev
 * [B * Tq][D] = tok_emb[token] + pos_emb[pos0 + t], 0 <= pos0, pos0 + Tq <=
 * ctx.  The modes:
 *   use_state != 0: pos0 reaches the kernel through a device-resident decode
 *     state only (the host position passed beside it is -1).
 *   pad (HOST [B], nullable): the pad form of a prompted step; clip b's rows
 *     get positions pos0 + t - pad[b], 0 <= pad[b] <= pos0.
 *   gamma_dev non-null (D % 32 == 0): the LayerNorm-fold producer, which also
 *     writes tiled_dev = the A-tiled operand of x * gamma
 *     (wq4_atiled_bytes(B * Tq, D, prec) bytes; only rows < B * Tq are written)
 *     and stats_dev [B * Tq][D / 16][2] = (mean, sum of squared deviations) of
 *     each 16-column tile of x. */
wq4_status wa_embed_check(int device, const int32_t* tokens, const float* tok_emb_dev, int V,
                          const float* pos_emb_dev, int ctx, int B, int Tq, int D, int pos0, int use_state,
                          const int32_t* pad /* nullable */, const float* gamma_dev, wq4_precision prec,
                          float* x_dev, void* tiled_dev, float* stats_dev);

/* ---- the picks --------------------------------------------------------------
 * What the two pick entries share.  ts0 in [0, V].  ids (HOST [n_ids], n_ids
 * >= 0): a suppress list for this pick, each id in [0, ts0) -- in [0, V) with
 * ts0 = 0; an empty list launches what the entry launches without one.
 * records (HOST [rows][8], nullable; needs ts0 >= 1): one rule record per row
 * (wa_timestamp_rule) selects the timestamp form; mass_dev (nullable, int32
 * [rows]) then receives 1 where rule f masked [0, ts0) as well.  temperature /
 * seed (HOST [rows], both or neither; every temperature finite and >= 0)
 * select the sampled pick.  tok_dev int32 [rows]; logprob_dev f32 [rows]
 * (nullable in the greedy form only) = log softmax(z)[tok] over the finally
 * masked row z the pick saw, untempered.  At most 32 rows. */
/* The decode step's fused tied-embedding logits + pick: hid_dev [n_clips, D]
 * f32 (final LayerNorm output), emb_dev [V, D] f32, D % 128 == 0.  Greedy: the
 * last maximum on ties (whisper.rs:131-138), EOT masked when step + 1 < 3
 * (:120-122); with logprob_dev the scored launch (entries n_clips .. 31 of a
 * longer logprob_dev are not written).  Sampled: pick index step + 1, 0 <=
 * step <= 16.  logits_dev (nullable) [n_clips, V]: the rows as the workgroups
 * saw them -- masks a-e and the list applied, without rule f and without
 * noise. */
wq4_status wa_logits_pick_check(int device, const float* hid_dev, const float* emb_dev, int n_clips, int D, int V,
                                int step, wq4_precision prec, const int32_t* ids, int n_ids,
                                const float* temperature, const uint64_t* seed, int ts0, const int32_t* records,
                                int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev, float* logits_dev);
/* The picks from stored logits (the prompt's pick, decode groups wider than 32
 * rows): logits_dev [n_rows, V] f32.  Without temperature and records: the
 * argmax kernel (EOT masked when suppress_eot) and, logprob_dev non-null,
 * wa_row_logprob_check's kernel over the masked row.  Otherwise the row-pick
 * kernel, `pick` >= 0 the noise's index; without records EOT is masked when
 * suppress_eot and mass_dev, when given, is written 0. */
wq4_status wa_row_pick_check(int device, const float* logits_dev, int n_rows, int V, int suppress_eot, int pick,
                             const int32_t* ids, int n_ids, const float* temperature, const uint64_t* seed, int ts0,
                             const int32_t* records, int32_t* tok_dev, float* logprob_dev, int32_t* mass_dev);
/* The row kernel behind the scores taken from stored logits (the prompt's
 * pick, no-speech and language probabilities, decode groups wider than 32
 * rows): logits_dev [n_rows, V] f32 -> logprob_dev [n_rows] f32 = z[id] -
 * logsumexp(z[lo:hi]), id = idx_dev[row] (idx_dev nullable: then fixed_idx),
 * EOT (50257) counted as -inf when mask_eot != 0.  An id outside [lo, hi)
 * gives NaN.  n_rows <= 32, 0 <= lo < hi <= V. */
wq4_status wa_row_logprob_check(int device, const float* logits_dev, int n_rows, int V, int lo, int hi, int mask_eot,
                                const int32_t* idx_dev, int fixed_idx, float* logprob_dev);
/* The timestamp bookkeeping kernel, one token per row and launch: tokens HOST
 * [n_rows][n_steps] -> records_out HOST [n_steps][n_rows][8], the records
 * after each launch (from the first pick's record). */
wq4_status wa_timestamp_bookkeep_check(int device, const int32_t* tokens, int n_rows, int n_steps, int ts0, int V,
                                       int max_initial, int32_t* records_out);

/* ---- beam search ------------------------------------------------------------ */
/* The per-row log-softmax + top-kp kernel: logits_dev [n_rows][V] f32, V >=
 * 16, kp = K + 1 in [2, 9]; EOT is masked when !eot_stop, else step < 0 ?
 * suppress_eot : step + 1 < 3 (through a device state) -> tok_dev / lp_dev
 * [n_rows][kp], *flag_out = the range flag.  records (HOST [n_rows][8],
 * nullable) selects the kernel under the timestamp rules; mass_dev (nullable)
 * int32 [n_rows] is then 1 where rule f fired, and a row with fewer than kp
 * allowed ids ends in (0, -inf) entries.  ids (HOST [n_ids]) as for the picks.
 * ts0 in (EOT, V] with records or ids; read by neither otherwise (pass 0). */
wq4_status wa_beam_topk_check(int device, const float* logits_dev, int n_rows, int V, int kp, int suppress_eot,
                              int step, int eot_stop, int ts0, const int32_t* ids, int n_ids,
                              const int32_t* records, int32_t* tok_dev, float* lp_dev,
                              int32_t* mass_dev /* nullable */, int32_t* flag_out);
/* One merge step over n_clips clips of K beams (rows = n_clips * K), in place
 * on the caller's state so that consecutive calls are consecutive steps:
 * top_tok_dev / top_lp_dev [rows][K + 1]; S_dev [rows]; next_tok_dev,
 * parent_dev [rows] (the cache row each new beam continues); anc_dev [2][rows]
 * [ctx] ancestor tables, the live one (state step + 1) & 1; fed_dev [ctx][rows];
 * fin_sum_dev, fin_len_dev [n_clips][C]; fin_anc_dev [n_clips][C][ctx];
 * fin_n_dev, complete_dev [n_clips]; state_dev int32 [4] = position, kv_len,
 * step, complete clips -- with 0 <= kv_len < ctx and fin_n in [0, C].
 * records_dev (nullable): the rows' rule records, device int32 [rows][8],
 * advanced in place -- new beam n gets the record of its parent advanced by its
 * token (wa_timestamp_rule's update with ts0, V; 1 <= ts0 <= V).  Without
 * records ts0 and V are not read. */
wq4_status wa_beam_select_check(int device, const int32_t* top_tok_dev, const float* top_lp_dev, float* S_dev,
                                int32_t* next_tok_dev, int32_t* parent_dev, int32_t* anc_dev, int32_t* fed_dev,
                                float* fin_sum_dev, int32_t* fin_len_dev, int32_t* fin_anc_dev, int32_t* fin_n_dev,
                                int32_t* complete_dev, int32_t* state_dev, int32_t* records_dev /* nullable */,
                                int ts0, int V, int n_clips, int K, int C, int ctx);

/* ---- token alignment -------------------------------------------------------- */
/* The weights and filter kernels of wa_align: q_dev [n_clips * P, 64 H] f32
 * (clip c's rows are [pad[c], P), pad HOST), k_dev head-major [n_clips][H][T]
 * [64] f32, heads (HOST) n_heads distinct heads of that layer, F (HOST)
 * [n_clips] each in [4, T] -> matrix_out_dev [n_clips][P][T] f32: row i < N_c =
 * P - pad[c] - 1 - first_row of clip c is M of its position first_row + i over
 * frames < F[c]; everything else 0.  P <= 448. */
wq4_status wa_align_matrix_check(int device, const float* q_dev, const float* k_dev, int n_clips, int P,
                                 const int32_t* pad, int T, int H, const int32_t* heads, int n_heads,
                                 const int32_t* F, int first_row, wq4_precision prec, float* matrix_out_dev);
/* The DTW kernel on caller costs: x_dev [n_clips][N_ld][F_ld] f32, N / F
 * (HOST) [n_clips], 1 <= N <= N_ld <= 447, 1 <= F <= F_ld -> jump_out_dev
 * [n_clips][N_ld] int32 (entries < N written), trace_out_dev (nullable) bytes
 * [n_clips][N_ld + 1][F_ld + 1]: cells [0 .. N][0 .. F] written, row 0 = 2,
 * column 0 = 1. */
wq4_status wa_dtw_check(int device, const float* x_dev, int n_clips, int N_ld, int F_ld, const int32_t* N,
                        const int32_t* F, int32_t* jump_out_dev, uint8_t* trace_out_dev /* nullable */);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_AMD_CHECKS_H */
