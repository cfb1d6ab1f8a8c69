// wa_forward.cpp -- Whisper model runtime around the Q4 path (host side):
// the activations and the encoder / decoder passes.
//
// Re-builds, MI355X-first, the module graph that calls the Q4 operator in the
// reference (zerr0o/whisper-burn):
//   WhisperEncoder::forward        src/model/encoder.rs:87-115
//   EncoderBlock::forward          src/model/encoder.rs:37-49
//   DecoderBlock::forward_*        src/model/decoder.rs:77-283
//   WhisperDecoder::forward_prompt src/model/decoder.rs:251-296
//   WhisperDecoder::decode_step    src/model/decoder.rs:306-348
//   WhisperModel::transcribe       src/model/whisper.rs:51-128 (wa_transcribe.cpp)
// Design points: clips are batched through every kernel; q/k/v
// (and cross k/v) projections run as ONE Q4 GEMM over row-concatenated Q4
// weights (bitwise identical per output to separate GEMMs); bias, GELU and
// the residual add are fused into the Q4 GEMM epilogues; LayerNorm and the
// attention kernels write the Q4 GEMM operand (A-tiled f16 hi/lo) directly;
// the KV caches are preallocated (no Tensor::cat); the greedy loop keeps
// tokens, positions and the done flags on the device and each decode step is
// one replayed hipGraph.
#include "wa_model.hpp"

using namespace wa;

namespace {

constexpr int kSOT = 50258;

// HIP-event bracket of one launch (only when m->profile).
struct Prof {
  wa_model* m;
  hipStream_t st;
  int cat;
  double gflop, gb;
  hipEvent_t a = nullptr, b = nullptr;
  Prof(wa_model* m_, hipStream_t st_, int cat_, double gflop_, double gb_)
      : m(m_), st(st_), cat(cat_), gflop(gflop_), gb(gb_) {
    // the CU-masked stream of a pipelined transcribe is not timed: the
    // events measure the kernels at full width
    if (m->profile && st != m->enc_stream && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
      (void)hipEventRecord(a, st);
  }
  ~Prof() {
    if (a && b) {
      (void)hipEventRecord(b, st);
      m->pending.push_back({a, b, cat, gflop, gb});
    }
  }
};

// Algorithmic cost of one Q4 GEMM: 2*rows*N*K flops;
// N*K*18/32 weight bytes + rows*K*4 (x, f32 at the ABI) + rows*N*4 (y).
Prof q4prof(wa_model* m, hipStream_t st, const wq4_tensor* w, int64_t rows) {
  int64_t n = 0, k = 0;
  (void)wq4_tensor_shape(w, &n, &k);
  return Prof(m, st, 0, 2.0 * rows * n * k * 1e-9, ((double)n * k * 18 / 32 + 4.0 * rows * k + 4.0 * rows * n) * 1e-9);
}

// LayerNorm fold for this decoder pass: decode steps (Tq = 1) whose GEMMs
// all run the 8-wave decode plans (WA_LN_FOLD=0 disables, for A/B runs).
bool lnfold_on(const wa_model* m, int Tq, const DecodeState* state, int64_t rows) {
  static const bool enabled = [] {
    const char* e = getenv("WA_LN_FOLD");
    return e ? atoi(e) != 0 : true;
  }();
  if (!enabled || !m->fold_allowed() || state == nullptr || Tq != 1 || m->dec.empty()) return false;
  const DecLayer& L = m->dec[0];
  for (const wq4_tensor* w : {L.qkv, L.out, L.cq, L.cout, L.fc1, L.fc2})
    if (!wq4_lnfold_supported(w, rows)) return false;
  return true;
}

// A decode step of <= 32 clips picks its tokens inside the logits kernel
// (wa::launch_logits_pick); prompts and larger groups keep the stored logits +
// a separate pick.  A beam call keeps the stored logits: its top-(K + 1) reads them.
bool fused_pick(const DecGroup& g, const DecodeCall& call, int Tq, const DecodeState* state) {
  return state != nullptr && Tq == 1 && g.nb <= 32 && call.beam_k == 0;
}

// The fused pick of group g in the call's mode: a scored call (call.score)
// leaves the pick's log-probability in next_lp, a timestamp one (call.ts)
// picks under the clips' rule records, a sampled one (call.sample) at their
// temperatures and seeds; under the model's `always` suppress mask, if it
// has lists (every pick but a clip's first).
PickArgs pick_args(const wa_model* m, const DecGroup& g, const DecodeCall& call) {
  PickArgs p{};
  p.scratch = g.lg_scr;
  p.counter = g.lg_ctr;
  p.out_tok = g.next_tok;
  p.out_lp = call.score ? g.next_lp : nullptr;
  p.rules = call.ts ? g.ts_rules : nullptr;
  p.ts0 = m->ts0();
  p.temp = call.sample ? g.smp_temp : nullptr;
  p.seed = call.sample ? g.smp_seed : nullptr;
  p.sup = m->sup_mask;
  return p;
}

// One greedy step (whisper.rs:104-125): bookkeeping, decode_step, the pick.
// The bookkeeping stores a scored call's log-probabilities where the tokens
// go and advances a timestamp call's rule records; a stored-logits group
// picks with the row kernels, in the mode of pick_args.
wq4_status decode_step(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st) {
  const PickArgs p = pick_args(m, g, call);
  const int V = m->cfg.n_vocab;
  WA_HIP(launch_bookkeep(g.next_tok, p.out_lp, g.tokens, call.score ? g.logprob : nullptr, g.ntok, g.done, g.nb,
                         kMaxTokens, call.eot_stop, g.state, call.ts ? g.ts_rules : nullptr, p.ts0, V, st));
  WA_TRY(decoder_forward(m, g, call, g.next_tok, 1, g.state, 0, 0, st));
  if (fused_pick(g, call, 1, g.state)) return WQ4_OK;
  if (p.temp || p.rules) {  // the sampled (pick step + 1) or timestamp pick over the stored rows
    WA_HIP(launch_row_pick(g.logits, g.nb, V, V, 0, kMinTokens, g.state, p.rules, p.ts0, p.temp, p.seed, 0, g.next_tok,
                           g.next_lp, nullptr, m->range_flag, st, p.sup));
  } else {
    WA_HIP(launch_argmax_step(g.logits, g.nb, V, kMinTokens, g.state, g.next_tok, m->range_flag, st, p.sup));
    if (call.score)
      WA_HIP(launch_row_logprob(g.logits, g.nb, V, 0, V, 0, kMinTokens, g.state, g.next_tok, 1, 0, g.next_lp, 1, st,
                                p.sup));
  }
  return WQ4_OK;
}

}  // namespace

namespace wa {

wq4_status alloc_activations(wa_model* m) {
  const Config& c = m->cfg;
  const int D = c.n_audio_state, F = 4 * D, Dt = c.n_text_state, Ft = 4 * Dt;
  const int B = m->bmax, T = c.n_audio_ctx;
  const int64_t renc = (int64_t)B * T, rdec = (int64_t)B * 4;
  Dev& d = m->dev;
  auto tiled = [&](int64_t rows, int k) {
    const size_t n = wq4_atiled_bytes(rows, k, m->prec);
    m->bytes += n;
    return d.alloc<_Float16>(n / 2);
  };
  auto f32 = [&](int64_t n) {
    m->bytes += (size_t)n * 4;
    return d.alloc<float>((size_t)n);
  };
  m->h1 = f32((int64_t)B * 2 * T * D);
  m->x = f32(renc * D);
  m->qkv = f32(renc * 3 * D);
  m->at_d = tiled(renc, D);
  m->at_f = tiled(renc, F);
  Lane& lane0 = m->lanes[0];  // the further lanes: ensure_lanes
  lane0.planes = d.alloc<_Float16>((size_t)renc * m->ns * D);
  m->bytes += (size_t)renc * m->ns * D * 2;
  for (size_t li = 0; li < m->dec.size(); ++li) {
    lane0.cache_k.push_back(f32((int64_t)B * c.n_text_ctx * Dt));
    lane0.cache_v.push_back(f32((int64_t)B * c.n_text_ctx * Dt));
  }  // the cross K / V caches: on the first transcribe that reads them (cross_kv_forward)
  // f16-pair tied embedding for the decode step's fused logits + pick,
  // fragment-tiled (1 KiB contiguous per load instruction)
  if (!emb_tiled_supported(Dt)) return fail(WQ4_EINVAL, "n_text_state must be a multiple of 128");
  const size_t erows = (size_t)emb_tiled_rows(c.n_vocab);
  m->tok_emb2 = d.alloc<_Float16>(erows * m->ns * Dt);
  if (!m->tok_emb2) return fail(WQ4_ENOMEM, "embedding plane allocation failed");
  m->bytes += erows * m->ns * Dt * 2;
  WA_HIP(launch_emb_tiled(m->tok_emb, c.n_vocab, Dt, m->ns, m->tok_emb2, nullptr));
  // cross-attention scratch, sized for the largest plan over 1..4B rows
  const int HP = (c.n_text_head + 15) / 16 * 16;
  size_t xpart = 0;
  for (int r = 1; r <= rdec; ++r) xpart = std::max(xpart, xattn_part_floats(r, c.n_text_head, Dt, T));
  m->groups.resize(kMaxGroups);
  for (DecGroup& g : m->groups) {  // each group sized for the whole batch (small)
    g.xd = f32(rdec * Dt);
    g.qkvd = f32(rdec * 3 * Dt);
    g.qd = f32(rdec * Dt);
    g.hid = f32(rdec * Dt);
    g.logits = f32((int64_t)B * c.n_vocab);
    g.atd_dec = tiled(rdec, Dt);
    g.atf_dec = tiled(rdec, Ft);
    g.prompt_tok = d.alloc<int>(rdec);
    g.next_tok = d.alloc<int>(B);
    g.tokens = d.alloc<int>((size_t)B * kMaxTokens);
    g.ntok = d.alloc<int>(B);
    g.done = d.alloc<int>(B);
    g.state = d.alloc<DecodeState>(1);
    g.xattn_part = f32((int64_t)xpart);
    const int kvc = std::max(1, m->kv_clips);
    g.xkv_part = f32((int64_t)cross_attention_kv_part_floats(kvc, c.n_text_head, T));
    g.xkv_ctr = d.alloc<int>((size_t)kvc * c.n_text_head);
    g.xqt = d.alloc<_Float16>((size_t)rdec * m->ns * HP * Dt);
    g.atd_ln = tiled(rdec, Dt);
    g.ln_stats = f32(rdec * (Dt / 16) * 2);  // per 16-column tile (the decode-step GEMM)
    g.hid_t = tiled(rdec, Dt);
    g.lg_scr = f32(logits_pick_scratch_floats(c.n_vocab));
    g.lg_ctr = d.alloc<int>(1);
    m->bytes += (size_t)rdec * m->ns * HP * Dt * 2;
    for (void* p : {(void*)g.xd, (void*)g.qkvd, (void*)g.qd, (void*)g.hid, (void*)g.logits, (void*)g.atd_dec,
                    (void*)g.atf_dec, (void*)g.prompt_tok, (void*)g.next_tok, (void*)g.tokens, (void*)g.ntok,
                    (void*)g.done, (void*)g.state, (void*)g.xattn_part, (void*)g.xqt, (void*)g.lg_scr,
                    (void*)g.lg_ctr, (void*)g.atd_ln, (void*)g.ln_stats, (void*)g.hid_t,
                    (void*)g.xkv_part, (void*)g.xkv_ctr})
      if (!p) return fail(WQ4_ENOMEM, "decode-group allocation failed");
    WA_HIP(hipMemset(g.xkv_ctr, 0, (size_t)kvc * c.n_text_head * sizeof(int)));
    WA_HIP(hipMemset(g.atd_ln, 0, wq4_atiled_bytes(rdec, Dt, m->prec)));
    WA_HIP(hipMemset(g.hid_t, 0, wq4_atiled_bytes(rdec, Dt, m->prec)));  // padded clips stay 0
    WA_HIP(hipMemset(g.lg_ctr, 0, sizeof(int)));
    WA_HIP(hipMemset(g.xqt, 0, (size_t)rdec * m->ns * HP * Dt * 2));  // padded heads stay 0
    WA_HIP(hipMemset(g.atd_dec, 0, wq4_atiled_bytes(rdec, Dt, m->prec)));
    WA_HIP(hipMemset(g.atf_dec, 0, wq4_atiled_bytes(rdec, Ft, m->prec)));
    WA_HIP(hipHostMalloc(reinterpret_cast<void**>(&g.host_ndone), 8 * sizeof(int), 0));
    WA_HIP(hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking));
  }
  m->range_flag = d.alloc<int>(1);
  for (void* p : {(void*)m->h1, (void*)m->x, (void*)m->qkv, (void*)m->at_d, (void*)m->at_f, (void*)lane0.planes,
                  (void*)m->range_flag})
    if (!p) return fail(WQ4_ENOMEM, "activation allocation failed");
  WA_HIP(hipMemset(m->range_flag, 0, sizeof(int)));
  for (size_t li = 0; li < m->dec.size(); ++li)
    if (!lane0.cache_k[li] || !lane0.cache_v[li]) return fail(WQ4_ENOMEM, "KV cache allocation failed");
  // zero the A-tiled buffers once: padded rows stay finite forever
  WA_HIP(hipMemset(m->at_d, 0, wq4_atiled_bytes(renc, D, m->prec)));
  WA_HIP(hipMemset(m->at_f, 0, wq4_atiled_bytes(renc, F, m->prec)));
  return WQ4_OK;
}

// ------------------------------------------------------------ forward --
// WhisperEncoder::forward (encoder.rs:87-115) in three parts, so that a
// pipelined transcribe (wa_transcribe_batches) can run the front and the
// first layers of the next batch's encoder on a CU-masked stream beside the
// current batch's decode: encoder_front (the conv stem), encoder_layers
// [l0, l1) and encoder_post (ln_post, f32, into enc_out_f32 or the conv
// scratch; m->enc_f32 points at it).
wq4_status encoder_front(wa_model* m, const float* mel, int B, hipStream_t st) {
  const Config& c = m->cfg;
  const int D = c.n_audio_state, T = c.n_audio_ctx;
  const int T_mel = 2 * T;
  const int64_t rows = (int64_t)B * T;
  {  // conv1 + GELU: mel [B, n_mels, 3000] -> h1 [B, 3000, D]   (encoder.rs:89-90)
    Prof p(m, st, 2, 2.0 * B * T_mel * D * 3.0 * c.n_mels * 1e-9, 4.0 * B * T_mel * (c.n_mels + D) * 1e-9);
    WA_HIP(launch_conv_gelu(mel, (long)c.n_mels * T_mel, T_mel, 1, B, c.n_mels, T_mel, 1, m->conv1_wt, m->conv1_b,
                            nullptr, D, m->h1, st));
  }
  {  // conv2 (stride 2) + GELU + positional embedding -> x [B, 1500, D]   (:93-106)
    Prof p(m, st, 2, 2.0 * rows * D * 3.0 * D * 1e-9, 4.0 * B * (T_mel + T) * D * 1e-9);
    WA_HIP(launch_conv_gelu(m->h1, (long)T_mel * D, 1, D, B, D, T_mel, 2, m->conv2_wt, m->conv2_b, m->enc_pos, D,
                            m->x, st));
  }
  return WQ4_OK;
}

wq4_status encoder_layers(wa_model* m, int B, int l0, int l1, hipStream_t st) {
  const Config& c = m->cfg;
  const int D = c.n_audio_state, T = c.n_audio_ctx, H = c.n_audio_head;
  const int64_t rows = (int64_t)B * T;
  const double ln_gb = 8.0 * rows * D * 1e-9;
  for (int li = l0; li < l1; ++li) {  // EncoderBlock::forward (encoder.rs:37-49)
    const EncLayer& L = m->enc[li];
    {
      Prof p(m, st, 3, 0.0, ln_gb);
      WA_WQ4(wq4_layernorm(m->x, L.ln1_w, L.ln1_b, rows, D, m->prec, m->at_d, nullptr, st));
    }
    {
      Prof p = q4prof(m, st, L.qkv, rows);
      WA_WQ4(wq4_gemm_tiled(L.qkv, L.qkv_b, m->at_d, nullptr, m->qkv, nullptr, rows, 0u, m->prec, 1, st));
    }
    {
      Prof p(m, st, 1, 4.0 * B * H * (double)T * T * 64 * 1e-9, 16.0 * rows * D * 1e-9);
      WA_HIP(launch_encoder_attention(m->qkv, B, T, H, m->at_d, m->ns, st, m->f32_attn() ? m->h1 : nullptr));
    }
    if (m->f32_attn()) {  // range tier 3: the f32 attention output through Q4Linear::forward (m->at_d: workspace)
      WA_WQ4(wq4_linear_forward_ws(L.out, L.out_b, m->h1, m->x, m->x, rows, D, WQ4_EPI_RESIDUAL, m->prec, m->at_d,
                                   wq4_atiled_bytes(rows, D, m->prec), st));
    } else {
      Prof p = q4prof(m, st, L.out, rows);
      WA_WQ4(wq4_gemm_tiled(L.out, L.out_b, m->at_d, m->x, m->x, nullptr, rows, WQ4_EPI_RESIDUAL, m->prec, 1, st));
    }
    if (m->abi_ffn()) {  // range tier 2: Q4FFN::forward with per-call operand scales (m->qkv: f32 scratch)
      WA_WQ4(wq4_layernorm(m->x, L.ln2_w, L.ln2_b, rows, D, WQ4_PREC_F16X2, nullptr, m->qkv, st));
      WA_WQ4(wq4_ffn_forward_ws(L.fc1, L.fc1_b, L.fc2, L.fc2_b, m->qkv, m->x, m->x, rows, WQ4_EPI_RESIDUAL, m->prec,
                                m->ffn_ws, m->ffn_ws_bytes, st));
      continue;
    }
    {
      Prof p(m, st, 3, 0.0, ln_gb);
      WA_WQ4(wq4_layernorm(m->x, L.ln2_w, L.ln2_b, rows, D, m->prec, m->at_d, nullptr, st));
    }
    {
      Prof p = q4prof(m, st, L.fc1, rows);
      WA_WQ4(wq4_gemm_tiled(L.fc1, L.fc1_b, m->at_d, nullptr, nullptr, m->at_f, rows,
                            WQ4_EPI_GELU | WQ4_EPI_TILED_OUT, m->prec, 1, st));
    }
    {
      Prof p = q4prof(m, st, L.fc2, rows);
      WA_WQ4(wq4_gemm_tiled(L.fc2, L.fc2_b, m->at_f, m->x, m->x, nullptr, rows, WQ4_EPI_RESIDUAL, m->prec, 1, st));
    }
  }
  return WQ4_OK;
}

wq4_status encoder_post(wa_model* m, int B, hipStream_t st, float* enc_out_f32) {
  const Config& c = m->cfg;
  const int D = c.n_audio_state;
  const int64_t rows = (int64_t)B * c.n_audio_ctx;
  Prof p(m, st, 3, 0.0, 8.0 * rows * D * 1e-9);
  float* out = enc_out_f32 ? enc_out_f32 : m->h1;
  WA_WQ4(wq4_layernorm(m->x, m->lnp_w, m->lnp_b, rows, D, WQ4_PREC_F16X2, nullptr, out, st));
  m->enc_f32 = out;
  return WQ4_OK;
}

wq4_status encoder_forward(wa_model* m, const float* mel, int B, hipStream_t st, float* enc_out_f32) {
  WA_TRY(encoder_front(m, mel, B, st));
  WA_TRY(encoder_layers(m, B, 0, (int)m->enc.size(), st));
  return encoder_post(m, B, st, enc_out_f32);
}

// The cross-attention state of every decoder layer: the reference caches
// K = enc Wk^T and V = enc Wv^T per layer (attention.rs:177-206
// forward_init_cache); here one copy of encoder_out as f16 planes serves all
// layers (wa_xattn.hip).
// Transcribes of at most kv_clips clips also get the reference's own
// per-layer caches, K = enc Wk^T and V = enc Wv^T + bv, head-major (the
// few-clip decode reads them: launch_cross_attention_kv).
// `caches` false (wa_encode: no decode follows it) fills the planes only.
// The caches (f32, kv_clips x n_audio_ctx x n_text_state per layer and
// tensor: 3.9 GB for Large-V3 at 8 clips) are allocated on the first
// transcribe of at most kv_small clips, so batches past that never hold them.
wq4_status cross_kv_forward(wa_model* m, int B, hipStream_t st, bool caches, int lane) {
  const Config& c = m->cfg;
  const int64_t rows = (int64_t)B * c.n_audio_ctx;
  WA_HIP(launch_enc_planes(m->enc_f32, rows, c.n_audio_state, m->ns, m->lanes[lane].planes, st));
  // a further lane's batch is one of a unit (more clips than the caches serve: no caches)
  if (lane > 0) return WQ4_OK;
  m->kv_batch = B;
  m->kv_n = caches && B <= m->kv_small ? B : 0;
  if (m->kv_n > 0 && !m->kv_alloc_ok) {
    // all layers or none: a partial failure frees what it got, so the next
    // transcribe retries the allocation (or fails the same way) instead of
    // running the cache GEMMs on a null layer
    const size_t n = (size_t)m->kv_clips * c.n_audio_ctx * c.n_text_state;
    bool ok = true;
    for (DecLayer& L : m->dec) {
      if (!L.xk) L.xk = m->dev.alloc<float>(n);
      if (!L.xv) L.xv = m->dev.alloc<float>(n);
      if (!L.xk || !L.xv) {
        ok = false;
        break;
      }
    }
    if (!ok) {
      for (DecLayer& L : m->dec) {
        m->dev.release(L.xk);
        m->dev.release(L.xv);
        L.xk = L.xv = nullptr;
      }
      m->kv_n = 0;
      return fail(WQ4_ENOMEM, "cross K/V cache allocation failed");
    }
    m->bytes += n * 8 * m->dec.size();
    m->kv_alloc_ok = true;
  }
  if (m->kv_n > 0) {
    // ln_post again, as the GEMMs' A-tiled operand (m->x still holds its
    // input); the caches of clips [0, kv_n): a prefix of the rows
    const int64_t kv_rows = (int64_t)m->kv_n * c.n_audio_ctx;
    WA_WQ4(wq4_layernorm(m->x, m->lnp_w, m->lnp_b, kv_rows, c.n_audio_state, m->prec, m->at_d, nullptr, st));
    for (DecLayer& L : m->dec) {
      WA_WQ4(wq4_gemm_tiled_headmajor(L.ck, nullptr, m->at_d, L.xk, kv_rows, c.n_audio_ctx, c.n_text_state, m->prec,
                                      0, st));
      WA_WQ4(wq4_gemm_tiled_headmajor(L.cv, L.cv_b, m->at_d, L.xv, kv_rows, c.n_audio_ctx, c.n_text_state, m->prec,
                                      0, st));
    }
  }
  return WQ4_OK;
}

// Decoder pass over Tq new tokens for the clips of group g (forward_prompt
// when state == nullptr, decode_step otherwise), ending in last-position
// logits.  Self-KV and the encoder planes are addressed at the group's clip
// offset.  The call decides the fused pick's mode and the trace, nothing else.
wq4_status decoder_forward(wa_model* m, DecGroup& g, const DecodeCall& call, const int* tokens, int Tq,
                           const DecodeState* state, int pos0, int kv0, hipStream_t st) {
  const Config& c = m->cfg;
  const int D = c.n_text_state, H = c.n_text_head, T = c.n_audio_ctx;
  const int B = g.nb;
  const int64_t rows = (int64_t)B * Tq;
  const size_t self_ofs = (size_t)g.b0 * H * c.n_text_ctx * 64;
  const Lane& lane = m->lanes[g.lane];
  const _Float16* enc = lane.planes + (size_t)g.b0 * T * m->ns * c.n_audio_state;
  // Decode steps fold every decoder LayerNorm into the GEMMs around it
  // (wq4_gemm_tiled_lnfold): the residual GEMM producing x also writes
  // tiled(x * gamma) and tile statistics, the GEMM reading LN(x) corrects
  // its epilogue -- no LayerNorm launches inside the layer loop.
  const bool fold = lnfold_on(m, Tq, state, rows);
  // range tier 3: attention outputs as f32 rows in g.hid, projected through
  // Q4Linear::forward at the ABI (g.atd_dec: its workspace); tier >= 1 has
  // the fold off
  float* const a32 = m->f32_attn() ? g.hid : nullptr;
  // a prompted call's steps: the clips' first cache slots (the pad forms)
  const int* const pad = call.prompt && state ? g.pad : nullptr;
  // y / yt = W LN(x) + bias, LN the LayerNorm (lw, lb) of the residual stream
  // g.xd: folded (wg, b2: W gamma and W beta + bias), or LayerNorm then GEMM
  auto ln_gemm = [&](const wq4_tensor* w, const float* bias, const float* wg, const float* b2, const float* lw,
                     const float* lb, float* y, void* yt, unsigned flags) -> wq4_status {
    if (fold) {
      const wq4_ln_fold cons{nullptr, nullptr, nullptr, g.ln_stats, wg};
      WA_WQ4(wq4_gemm_tiled_lnfold(w, b2, g.atd_ln, nullptr, y, yt, rows, flags, m->prec, &cons, st));
    } else {
      WA_WQ4(wq4_layernorm(g.xd, lw, lb, rows, D, m->prec, g.atd_dec, nullptr, st));
      WA_WQ4(wq4_gemm_tiled(w, bias, g.atd_dec, nullptr, y, yt, rows, flags, m->prec, 2, st));
    }
    return WQ4_OK;
  };
  // g.xd += W a + bias, a the A-tiled operand `at` or (tier 3) the f32 rows
  // `x32`.  Folded, it also produces the operand of the LayerNorm that reads
  // g.xd next (its gamma `next_lw`; null: none follows in the layer loop).
  auto resid_gemm = [&](const wq4_tensor* w, const float* bias, const void* at, const float* x32,
                        const float* next_lw) -> wq4_status {
    if (x32) {
      WA_WQ4(wq4_linear_forward_ws(w, bias, x32, g.xd, g.xd, rows, D, WQ4_EPI_RESIDUAL, m->prec, g.atd_dec,
                                   wq4_atiled_bytes(rows, D, m->prec), st));
    } else if (fold) {
      const wq4_ln_fold prod{next_lw, next_lw ? g.atd_ln : nullptr, next_lw ? g.ln_stats : nullptr, nullptr, nullptr};
      WA_WQ4(wq4_gemm_tiled_lnfold(w, bias, at, g.xd, g.xd, nullptr, rows, WQ4_EPI_RESIDUAL, m->prec, &prod, st));
    } else {
      WA_WQ4(wq4_gemm_tiled(w, bias, at, g.xd, g.xd, nullptr, rows, WQ4_EPI_RESIDUAL, m->prec, 2, st));
    }
    return WQ4_OK;
  };
  if (fold)
    WA_HIP(launch_embed_fold(tokens, m->tok_emb, m->dec_pos, B, Tq, D, state, pos0, g.xd, m->dec[0].ln1_w, g.atd_ln,
                             g.ln_stats, m->ns, st, pad));
  else
    WA_HIP(launch_embed(tokens, m->tok_emb, m->dec_pos, B, Tq, D, state, pos0, g.xd, st, pad));
  const int nl = (int)m->dec.size();
  for (int li = 0; li < nl; ++li) {  // DecoderBlock (decoder.rs:77-112 / 140-183)
    DecLayer& L = m->dec[li];
    // self-attention
    WA_TRY(ln_gemm(L.qkv, L.qkv_b, L.qkv_wg, L.qkv_b2, L.ln1_w, L.ln1_b, g.qkvd, nullptr, 0u));
    if (call.beam_k > 0 && state)  // a beam call's step: the caches through the rows' ancestor table
      WA_HIP(launch_decoder_self_attention_beam(g.qkvd, lane.cache_k[li] + self_ofs, lane.cache_v[li] + self_ofs, B, H,
                                                c.n_text_ctx, state, kv0, m->bm.anc, g.atd_dec, m->ns, st, a32, pad));
    else
      WA_HIP(launch_decoder_self_attention(g.qkvd, lane.cache_k[li] + self_ofs, lane.cache_v[li] + self_ofs, B, Tq, H,
                                           c.n_text_ctx, state, kv0, g.atd_dec, m->ns, st, a32, pad));
    WA_TRY(resid_gemm(L.out, L.out_b, g.atd_dec, a32, L.ln2_w));
    // cross-attention
    WA_TRY(ln_gemm(L.cq, L.cq_b, L.cq_wg, L.cq_b2, L.ln2_w, L.ln2_b, g.qd, nullptr, 0u));
    if (m->group_kv(g)) {  // few clips: one GEMV launch over the cached K / V
      const size_t kofs = (size_t)g.b0 * T * D;
      WA_HIP(launch_cross_attention_kv(g.qd, L.xk + kofs, L.xv + kofs, B, Tq, T, H, g.xkv_part, g.xkv_ctr, g.atd_dec,
                                       m->ns, st, a32));
    } else {
      WA_HIP(launch_xattn(g.qd, L.ck_raw, L.cv_raw, L.cv_p, L.cv_b, m->wtype, enc, B, Tq, T, H, D, g.xqt,
                          g.xattn_part, g.atd_dec, m->ns, g.xres, g.xplan, st, a32));
    }
    WA_TRY(resid_gemm(L.cout, L.cout_b, g.atd_dec, a32, L.ln3_w));
    // FFN
    if (m->abi_ffn()) {  // range tier 2: Q4FFN::forward with per-call operand scales (g.hid: f32 scratch)
      WA_WQ4(wq4_layernorm(g.xd, L.ln3_w, L.ln3_b, rows, D, WQ4_PREC_F16X2, nullptr, g.hid, st));
      WA_WQ4(wq4_ffn_forward_ws(L.fc1, L.fc1_b, L.fc2, L.fc2_b, g.hid, g.xd, g.xd, rows, WQ4_EPI_RESIDUAL, m->prec,
                                g.ffn_ws, g.ffn_ws_bytes, st));
      continue;
    }
    WA_TRY(ln_gemm(L.fc1, L.fc1_b, L.fc1_wg, L.fc1_b2, L.ln3_w, L.ln3_b, nullptr, g.atf_dec,
                   WQ4_EPI_GELU | WQ4_EPI_TILED_OUT));
    // fc2 feeds the next layer's attn_ln (none after the last layer: decoder.ln below)
    WA_TRY(resid_gemm(L.fc2, L.fc2_b, g.atf_dec, nullptr, li + 1 < nl ? m->dec[li + 1].ln1_w : nullptr));
  }
  // final LN (decoder.rs:286 / 340) and tied-embedding logits of the last
  // position of every clip (decoder.rs:289-292, 342-343)
  if (fused_pick(g, call, Tq, state)) {  // decode step: logits + the mode's pick in one kernel, into next_tok
    // the final LN writes the pick's operand directly (A-tiled, the
    // embedding planes' precision)
    WA_WQ4(wq4_layernorm(g.xd, m->dln_w, m->dln_b, rows, D, m->prec, g.hid_t, nullptr, st));
    const size_t tofs = (size_t)g.b0 * call.trace_s1 * call.trace_k;
    WA_HIP(launch_logits_pick(g.hid_t, B, D, m->tok_emb2, m->ns, c.n_vocab, kMinTokens, state, pick_args(m, g, call),
                              call.trace_out ? call.trace_ids + tofs : nullptr,
                              call.trace_out ? call.trace_out + tofs : nullptr, call.trace_s1, call.trace_k,
                              m->range_flag, st));
    return WQ4_OK;
  }
  WA_WQ4(wq4_layernorm(g.xd, m->dln_w, m->dln_b, rows, D, WQ4_PREC_F16X2, nullptr, g.hid, st));
  WA_HIP(launch_logits(g.hid + (size_t)(Tq - 1) * D, B, D, (int64_t)Tq * D, m->tok_emb, c.n_vocab, g.logits, st));
  return WQ4_OK;
}

// The scores taken at the SOT position of group g's prompt, from its unmasked
// logit rows z0 [nb][n_vocab]: the no-speech probability softmax(z0)
// [no_speech] and the language token's probability among the language tokens
// -- the token from lang_idx (stride lang_stride; the detected one) or the
// caller's lang_fixed.
wq4_status score_sot(wa_model* m, DecGroup& g, const float* z0, const int* lang_idx, int lang_stride, int lang_fixed,
                     hipStream_t st) {
  const Config& c = m->cfg;
  const int B = g.nb, V = c.n_vocab;
  WA_HIP(launch_row_logprob(z0, B, V, 0, V, 0, 0, nullptr, nullptr, 0, c.no_speech_token(), g.no_speech, 1, st));
  WA_HIP(launch_exp_inplace(g.no_speech, B, st));
  WA_HIP(launch_row_logprob(z0, B, V, 50259, 50259 + c.n_lang, 0, 0, nullptr, lang_idx, lang_stride, lang_fixed,
                            g.lang_prob, 1, st));
  WA_HIP(launch_exp_inplace(g.lang_prob, B, st));
  if (lang_idx) {
    WA_HIP(launch_gather_int(lang_idx, lang_stride, g.lang_tok, B, st));
  } else {
    const std::vector<int> lt(B, lang_fixed);  // pageable: the copy is staged before the call returns
    WA_HIP(hipMemcpyAsync(g.lang_tok, lt.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  }
  return WQ4_OK;
}

// Prompt of group g (whisper.rs:60-99), leaving the first greedy token in
// next_tok and the DecodeState ready for the step graph.
wq4_status prompt_group(wa_model* m, DecGroup& g, const DecodeCall& call, hipStream_t st) {
  const Config& c = m->cfg;
  const int B = g.nb, lang_token = call.lang_token;
  // a timestamp transcribe's prompt ends at TRANSCRIBE: no NO_TIMESTAMPS
  const int tail = call.ts ? 1 : 2;  // prompt tokens after the language token
  std::vector<int> ptok((size_t)B * 4);
  int pos0, kv0;
  if (call.prompt) {  // the caller's prompts: one prefill pass, the scores with it
    int P = 0;
    WA_TRY(prefill_group(m, g, call, st, &P));
    pos0 = P;
    kv0 = P;
  } else if (lang_token >= 0) {
    const int plen = 2 + tail;
    for (int b = 0; b < B; ++b) {
      ptok[b * plen + 0] = kSOT;
      ptok[b * plen + 1] = lang_token;
      ptok[b * plen + 2] = c.transcribe_token();
      if (!call.ts) ptok[b * plen + 3] = c.no_timestamps_token();
    }
    WA_HIP(hipMemcpyAsync(g.prompt_tok, ptok.data(), (size_t)B * plen * 4, hipMemcpyHostToDevice, st));
    WA_TRY(decoder_forward(m, g, call, g.prompt_tok, plen, nullptr, 0, 0, st));
    if (call.score) {
      // z0, the SOT position's logits: row 0 of each clip's final-LN rows in
      // g.hid (by causality the single-SOT pass of the auto-detect prompt)
      WA_HIP(launch_logits(g.hid, B, c.n_text_state, (int64_t)plen * c.n_text_state, m->tok_emb, c.n_vocab, g.z0, st));
      WA_TRY(score_sot(m, g, g.z0, nullptr, 0, lang_token, st));
    }
    pos0 = plen;
    kv0 = plen;
  } else {
    // decode_step(SOT, 0) fills a 1-entry cache; the language is the last max
    // over the language-token range (whisper.rs:73-83) ...
    const int plen = 1 + tail;
    for (int b = 0; b < B; ++b) {
      ptok[b * plen + 0] = kSOT;
      ptok[b * plen + 1] = c.transcribe_token();
      if (!call.ts) ptok[b * plen + 2] = c.no_timestamps_token();
    }
    WA_HIP(hipMemcpyAsync(g.prompt_tok, ptok.data(), (size_t)B * plen * 4, hipMemcpyHostToDevice, st));
    // SOT rows: embed reads tokens[b * Tq + t] with Tq = 1 -> a contiguous [B]
    // array: next_tok as scratch
    std::vector<int> sot(B, kSOT);
    WA_HIP(hipMemcpyAsync(g.next_tok, sot.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    WA_TRY(decoder_forward(m, g, call, g.next_tok, 1, nullptr, 0, 0, st));
    WA_HIP(launch_argmax(g.logits, B, c.n_vocab, 50259, 50259 + c.n_lang, 0, g.prompt_tok, plen, m->range_flag, st));
    if (call.score) WA_TRY(score_sot(m, g, g.logits, g.prompt_tok, plen, 0, st));  // before the next pass rewrites g.logits
    // ... then forward_prompt([lang, TRANSCRIBE, NO_TIMESTAMPS]) OVERWRITES the
    // cache from index 0 with positions 0..2 (decoder.rs:272-283) while the
    // position counter continues at 1 + 3 = 4 (whisper.rs:74,93) -- without
    // NO_TIMESTAMPS: positions 0..1, the counter at 1 + 2.
    WA_TRY(decoder_forward(m, g, call, g.prompt_tok, plen, nullptr, 0, 0, st));
    pos0 = 1 + plen;
    kv0 = plen;
  }
  if (call.sample) {
    // the clips' temperatures and seeds (pageable: the copies are staged before the calls return)
    WA_HIP(hipMemcpyAsync(g.smp_temp, call.temp + g.clip0, (size_t)B * 4, hipMemcpyHostToDevice, st));
    WA_HIP(hipMemcpyAsync(g.smp_seed, call.seed + g.clip0, (size_t)B * 8, hipMemcpyHostToDevice, st));
  }
  if (call.ts) {  // every clip's rule record back to the empty history
    const std::vector<TsRule> first(B, ts_rule_first(m->ts0(), c.n_vocab, call.ts_max_initial));  // pageable: staged
    WA_HIP(hipMemcpyAsync(g.ts_rules, first.data(), (size_t)B * sizeof(TsRule), hipMemcpyHostToDevice, st));
  }
  if (call.sample || call.ts) {
    // pick 0 and its log-probability through the row kernel: under the first
    // pick's rule record (rule e; EOT is masked with the text) or with EOT
    // suppressed (whisper.rs:97-99); the suppress mask of pick 0 is the union
    const PickArgs p = pick_args(m, g, call);
    WA_HIP(launch_row_pick(g.logits, B, c.n_vocab, c.n_vocab, 1, 0, nullptr, p.rules, p.ts0, p.temp, p.seed, 0,
                           g.next_tok, g.next_lp, nullptr, m->range_flag, st, m->sup_mask0));
  } else {
    // first token: EOT suppressed (whisper.rs:97-99)
    WA_HIP(launch_argmax(g.logits, B, c.n_vocab, 0, c.n_vocab, 1, g.next_tok, 1, m->range_flag, st, m->sup_mask0));
    if (call.score)  // its log-probability over the masked row; step 0's bookkeeping stores it in slot 0
      WA_HIP(launch_row_logprob(g.logits, B, c.n_vocab, 0, c.n_vocab, 1, 0, nullptr, g.next_tok, 1, 0, g.next_lp, 1, st,
                                m->sup_mask0));
  }
  if (call.score) WA_HIP(hipMemsetAsync(g.logprob, 0xFF, (size_t)B * (kMaxTokens + 1) * 4, st));  // all bits set: NaN
  // frozen clips start done, and counted: the loop stops once the live ones emitted EOT
  std::vector<int> done0(B, 0);
  int n_frozen = 0;
  if (call.frozen)
    for (int b = 0; b < B; ++b) n_frozen += done0[b] = call.frozen[g.clip0 + b] ? 1 : 0;
  const DecodeState init{pos0 - 1, kv0 - 1, -1, n_frozen};
  WA_HIP(hipMemcpyAsync(g.state, &init, sizeof(init), hipMemcpyHostToDevice, st));
  WA_HIP(hipMemsetAsync(g.ntok, 0, (size_t)B * 4, st));
  if (n_frozen)
    WA_HIP(hipMemcpyAsync(g.done, done0.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));  // pageable: staged
  else
    WA_HIP(hipMemsetAsync(g.done, 0, (size_t)B * 4, st));
  WA_HIP(hipMemsetAsync(g.tokens, 0, (size_t)B * kMaxTokens * 4, st));
  return WQ4_OK;
}

// Capture (once per group size / eot mode) the step graph of group g.
wq4_status ensure_graph(wa_model* m, DecGroup& g, const DecodeCall& call) {
  // a group that decoded alone and then decodes in a pair, or in another mode, recaptures
  const char* bad = nullptr;
  const int64_t key = graph_key((call.score ? 1 : 0) + (call.ts ? 2 : 0) + (call.sample ? 4 : 0), g.lane, g.b0, g.nb,
                                call.eot_stop ? 1 : 0, call.trace_out ? 1 : 0, m->group_kv(g) ? 1 : 0, m->range_tier,
                                g.xplan.splits, g.xres.q, &bad);
  if (key < 0) return fail(WQ4_EINVAL, std::string("step-graph key: digit '") + bad + "' is outside its radix");
  // a prompted call's graph runs the pad forms: kept apart beside the key
  const bool prompted = call.prompt != nullptr;
  if (g.graph && g.graph_key == key && g.graph_prompted == prompted) return WQ4_OK;
  // the other layouts' graphs are kept: a call goes from units of three to
  // pairs or a lone last batch, beside the masked stream and without it, and
  // the next call back again
  for (DecGroup::KeptGraph& k : g.kept)
    if (k.exec && k.key == key && k.prompted == prompted) {
      std::swap(g.graph, k.exec);
      std::swap(g.graph_key, k.key);
      std::swap(g.graph_prompted, k.prompted);
      return WQ4_OK;
    }
  if (g.graph) {  // park it: in a free slot, else in place of the one parked longest ago
    DecGroup::KeptGraph* slot = nullptr;
    for (DecGroup::KeptGraph& k : g.kept)
      if (!k.exec && !slot) slot = &k;
    if (!slot) {
      slot = &g.kept[g.kept_next];
      g.kept_next = (g.kept_next + 1) % kKeptGraphs;
      (void)hipGraphExecDestroy(slot->exec);
    }
    slot->exec = g.graph;
    slot->key = g.graph_key;
    slot->prompted = g.graph_prompted;
    g.graph = nullptr;
    g.graph_key = -1;
  }
  WA_WQ4(wq4_prepare_stream(m->device, g.st));  // split-K workspace exists before capture
  hipGraph_t gr;
  WA_HIP(hipStreamBeginCapture(g.st, hipStreamCaptureModeThreadLocal));
  wq4_status s = decode_step(m, g, call, g.st);
  hipError_t ce = hipStreamEndCapture(g.st, &gr);
  if (s != WQ4_OK) return s;
  if (ce != hipSuccess) return fail(WQ4_EHIP, std::string("graph capture: ") + hipGetErrorString(ce));
  ce = hipGraphInstantiate(&g.graph, gr, nullptr, nullptr, 0);
  (void)hipGraphDestroy(gr);
  if (ce != hipSuccess) return fail(WQ4_EHIP, std::string("graph instantiate: ") + hipGetErrorString(ce));
  g.graph_key = key;
  g.graph_prompted = prompted;
  return WQ4_OK;
}

// Clips up to which a transcribe decodes over cross K / V caches
// (WA_XATTN_KV_CLIPS overrides; 0 = never; measured in DESIGN.md §4).
void kv_config(wa_model* m, int max_batch) {
  static const int small = [] {
    const char* e = getenv("WA_XATTN_KV_CLIPS");
    return e ? std::max(0, atoi(e)) : 8;
  }();
  m->kv_small = std::min(small, max_batch);
  m->kv_clips = m->kv_small;
}

// Range tier 2's workspaces (wq4_ffn_forward_ws): the encoder's B * T rows
// and 4 * B rows per decode group (prompts), allocated once.
wq4_status ensure_ffn_ws(wa_model* m) {
  if (m->ffn_ws) return WQ4_OK;
  const DecLayer& Ld = m->dec.front();
  const EncLayer& Le = m->enc.front();
  const size_t ne = wq4_ffn_workspace_bytes(Le.fc1, Le.fc2, (int64_t)m->bmax * m->cfg.n_audio_ctx);
  const size_t nd = wq4_ffn_workspace_bytes(Ld.fc1, Ld.fc2, (int64_t)m->bmax * 4);
  if (ne == 0 || nd == 0) return fail(WQ4_EINVAL, "FFN workspace size");
  // all or nothing: a partial failure releases what it got, so a later
  // tier-2 entry allocates (or fails) afresh instead of leaking the first set
  void* e = m->dev.alloc<uint8_t>(ne);
  bool ok = e != nullptr;
  for (DecGroup& g : m->groups) {
    g.ffn_ws = ok ? m->dev.alloc<uint8_t>(nd) : nullptr;
    ok = ok && g.ffn_ws != nullptr;
  }
  if (!ok) {
    m->dev.release(e);
    for (DecGroup& g : m->groups) {
      m->dev.release(g.ffn_ws);
      g.ffn_ws = nullptr;
      g.ffn_ws_bytes = 0;
    }
    return fail(WQ4_ENOMEM, "range tier 2: FFN workspace allocation failed");
  }
  for (DecGroup& g : m->groups) {
    g.ffn_ws_bytes = nd;
    m->bytes += nd;
  }
  m->ffn_ws = e;
  m->ffn_ws_bytes = ne;
  m->bytes += ne;
  return WQ4_OK;
}

// The score buffers of every decode group (DecGroup::next_lp ..), each sized
// for the whole batch like the group's other buffers: allocated by the first
// scored transcribe, all or nothing, never released.
static wq4_status ensure_score_buffers(wa_model* m) {
  if (m->score_alloc_ok) return WQ4_OK;
  const size_t B = (size_t)m->bmax, V = (size_t)m->cfg.n_vocab;
  bool ok = true;
  for (DecGroup& g : m->groups) {
    g.next_lp = m->dev.alloc<float>(B);
    g.logprob = m->dev.alloc<float>(B * (kMaxTokens + 1));
    g.no_speech = m->dev.alloc<float>(B);
    g.lang_prob = m->dev.alloc<float>(B);
    g.lang_tok = m->dev.alloc<int>(B);
    g.z0 = m->dev.alloc<float>(B * V);
    ok = ok && g.next_lp && g.logprob && g.no_speech && g.lang_prob && g.lang_tok && g.z0;
  }
  if (!ok) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (DecGroup& g : m->groups) {
      for (void* p : {(void*)g.next_lp, (void*)g.logprob, (void*)g.no_speech, (void*)g.lang_prob, (void*)g.lang_tok,
                      (void*)g.z0})
        m->dev.release(p);
      g.next_lp = g.logprob = g.no_speech = g.lang_prob = g.z0 = nullptr;
      g.lang_tok = nullptr;
    }
    return fail(WQ4_ENOMEM, "score buffer allocation failed");
  }
  m->bytes += m->groups.size() * 4 * (B * (kMaxTokens + 1 + 4) + B * V);
  m->score_alloc_ok = true;
  return WQ4_OK;
}

// The timestamp buffers of every decode group (DecGroup::ts_rules ..):
// allocated by the first timestamp transcribe, all or nothing, never released.
static wq4_status ensure_ts_buffers(wa_model* m) {
  if (m->ts_alloc_ok) return WQ4_OK;
  const size_t B = (size_t)m->bmax;
  bool ok = true;
  for (DecGroup& g : m->groups) {
    g.ts_rules = m->dev.alloc<TsRule>(B);
    ok = ok && g.ts_rules;
  }
  if (!ok) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (DecGroup& g : m->groups) {
      m->dev.release(g.ts_rules);
      g.ts_rules = nullptr;
    }
    return fail(WQ4_ENOMEM, "timestamp buffer allocation failed");
  }
  m->bytes += m->groups.size() * B * sizeof(TsRule);
  m->ts_alloc_ok = true;
  return WQ4_OK;
}

// The sampling buffers of every decode group (DecGroup::smp_temp ..):
// allocated by the first sampled transcribe, all or nothing, never released.
static wq4_status ensure_sample_buffers(wa_model* m) {
  if (m->sample_alloc_ok) return WQ4_OK;
  const size_t B = (size_t)m->bmax;
  bool ok = true;
  for (DecGroup& g : m->groups) {
    g.smp_temp = m->dev.alloc<float>(B);
    g.smp_seed = m->dev.alloc<uint64_t>(B);
    ok = ok && g.smp_temp && g.smp_seed;
  }
  if (!ok) {
    (void)hipGetLastError();  // the failed hipMalloc is handled here
    for (DecGroup& g : m->groups) {
      for (void* p : {(void*)g.smp_temp, (void*)g.smp_seed}) m->dev.release(p);
      g.smp_temp = nullptr;
      g.smp_seed = nullptr;
    }
    return fail(WQ4_ENOMEM, "sampling buffer allocation failed");
  }
  m->bytes += m->groups.size() * B * 12;
  m->sample_alloc_ok = true;
  return WQ4_OK;
}

wq4_status prepare_call(wa_model* m, const DecodeCall& call) {
  WA_HIP(hipSetDevice(m->device));
  if (call.score) WA_TRY(ensure_score_buffers(m));
  if (call.ts) WA_TRY(ensure_ts_buffers(m));
  if (call.sample) WA_TRY(ensure_sample_buffers(m));
  return WQ4_OK;
}

// Lanes [0, want) of the per-clip decode state (wa_model::lanes), each sized
// like lane 0.  Returns the lanes the model has afterwards, at most `want`:
// a lane the device has no room for is not held in part, and the caller
// decodes narrower units (two lanes: pairs; one: every batch on its own).
int ensure_lanes(wa_model* m, int want) {
  want = std::min(want, kMaxLanes);
  const Config& c = m->cfg;
  const size_t np = (size_t)m->bmax * c.n_audio_ctx * m->ns * c.n_audio_state;
  const size_t nc = (size_t)m->bmax * c.n_text_ctx * c.n_text_state;
  while (m->n_lanes < want) {
    Lane lane;
    lane.planes = m->dev.alloc<_Float16>(np);
    bool ok = lane.planes != nullptr;
    for (size_t li = 0; ok && li < m->dec.size(); ++li) {
      lane.cache_k.push_back(m->dev.alloc<float>(nc));
      lane.cache_v.push_back(m->dev.alloc<float>(nc));
      ok = lane.cache_k.back() && lane.cache_v.back();
    }
    if (!ok) {
      (void)hipGetLastError();  // the failed hipMalloc is handled here
      m->dev.release(lane.planes);
      for (float* p : lane.cache_k) m->dev.release(p);
      for (float* p : lane.cache_v) m->dev.release(p);
      break;
    }
    m->lanes[m->n_lanes++] = std::move(lane);
    m->bytes += np * 2 + nc * 8 * m->dec.size();
  }
  return std::min(m->n_lanes, want);
}

// Number of decode groups for a batch (WA_DECODE_GROUPS overrides).
int decode_groups(int B) {
  static const int forced = [] {
    const char* env = getenv("WA_DECODE_GROUPS");
    return env ? atoi(env) : 0;
  }();
  int G = forced > 0 ? forced : (B >= 16 ? 2 : 1);
  if (G > kMaxGroups) G = kMaxGroups;
  if (G > B) G = B;
  return G;
}

}  // namespace wa
