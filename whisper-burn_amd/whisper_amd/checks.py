"""The kernel check wrappers (include/whisper_amd_checks.h): one function per
C check entry, running that product kernel on the caller's tensors in the mode
its arguments select, and the host-only probes of a decode's layout rules.
The older per-mode names (logits_argmax_check, row_sample_check,
self_attention_beam_pad_check, ...) are adapters of a few lines over them.
"""
from __future__ import annotations

import ctypes

import numpy as np

import wq4

from ._ffi import _as, _dev, _i32, _ptr, _torch, check, lib

XATTN_SHARE_DEN = 64  # wa_xattn_resident_share counts 64ths of a clip's sub-chunks
BEAM_SELECT_ARRAYS = ("top_tok", "top_lp", "S", "next_tok", "parent", "anc", "fed", "fin_sum", "fin_len", "fin_anc",
                      "fin_n", "complete", "state")


# ---- host-only probes --------------------------------------------------------
def xattn_resident_share(live_clips: int, T: int, planes: int, D: int, budget_mb: float = -1.0) -> int:
    """64ths of every clip's encoder-plane sub-chunks a decode with live_clips
    clips live keeps in the Infinity Cache (wa_xattn_resident_share; host
    logic): budget_mb < 0 = the product's rule."""
    q = int(lib().wa_xattn_resident_share(live_clips, T, planes, D, budget_mb))
    if q < 0:
        raise ValueError("bad sizes")
    return q


def xattn_chunk_resident(chunk: int, share: int) -> bool:
    """Whether 16-frame sub-chunk `chunk` of a clip is resident at `share` 64ths."""
    r = int(lib().wa_xattn_chunk_resident(chunk, share))
    if r < 0:
        raise ValueError("bad chunk / share")
    return bool(r)


def xattn_plan(T: int) -> tuple[int, int]:
    """(splits, sub-chunks per split) of the cross-attention's frame split for T frames."""
    s, c = ctypes.c_int(), ctypes.c_int()
    check(lib().wa_xattn_plan(T, ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def xattn_plan_splits(T: int, rows: int, free_cus: int) -> tuple[int, int]:
    """(splits, sub-chunks per split) of a decode whose largest group has `rows`
    rows and whose cross-attention launches may take free_cus CUs (<= 0: no
    bound): the host rule (wa_xattn_plan_splits), without the
    WA_XATTN_SPLITS_RT override."""
    s, c = ctypes.c_int(), ctypes.c_int()
    check(lib().wa_xattn_plan_splits(T, rows, free_cus, ctypes.byref(s), ctypes.byref(c)))
    return s.value, c.value


def decode_graph_key_check(mode: int, lane: int, b0: int, nb: int, eot: int, trace: int, group_kv: int,
                           range_tier: int, splits: int, residency: int) -> int:
    """The step-graph key of these digits, most significant first (mode: scored 1
    + timestamps 2 + sampled 4); -1 when one is outside its radix
    (wa_decode_graph_key_check)."""
    return int(lib().wa_decode_graph_key_check(mode, lane, b0, nb, eot, trace, group_kv, range_tier, splits, residency))


def pipeline_unit_sizes(n_batches: int, width: int) -> list[int]:
    """Sizes, in order, of the units a transcribe_batches over n_batches
    batches forms when up to `width` batches decode at once: the host rule
    (wa_pipeline_unit_sizes), without the device's room for lanes."""
    sizes, n = (ctypes.c_int * max(1, n_batches))(), ctypes.c_int()
    check(lib().wa_pipeline_unit_sizes(n_batches, width, sizes, ctypes.byref(n)))
    return [int(sizes[i]) for i in range(n.value)]


# ---- attention ---------------------------------------------------------------
def xattn_check(q, wk_raw, wv_raw, bv, enc, Tq: int, H: int, weight_type: int = 0,
                precision: int = wq4.PREC_F16X2):
    """One decoder layer's cross-attention through the product kernels
    (wa_xattn_check): q cuda f32 [B*Tq, 64H], wk_raw / wv_raw cuda uint8 raw
    weights, bv cuda f32 [64H], enc cuda f32 [B, T, 64H] -> [B*Tq, 64H]."""
    torch = _torch()
    B, T, D = enc.shape
    out = torch.empty((B * Tq, D), device=enc.device, dtype=torch.float32)
    ptr = lambda t: ctypes.c_void_p(t.contiguous().data_ptr())
    check(lib().wa_xattn_check(_dev(enc), ptr(q), ptr(wk_raw), ptr(wv_raw), ptr(bv), weight_type, ptr(enc), B, Tq, T,
                               H, precision, ptr(out)))
    return out


def xattn_kv_check(q, k, v, Tq: int, precision: int = wq4.PREC_F16X2):
    """The few-clip cross-attention over cached K / V (wa_xattn_kv_check):
    q cuda f32 [B*Tq, 64H], k / v cuda f32 head-major [B, H, T, 64] ->
    [B*Tq, 64H] (softmax(q K^T / 8) V per head)."""
    torch = _torch()
    B, H, T, _ = k.shape
    out = torch.empty((B * Tq, 64 * H), device=k.device, dtype=torch.float32)
    ptr = lambda t: ctypes.c_void_p(t.contiguous().data_ptr())
    check(lib().wa_xattn_kv_check(_dev(k), ptr(q), ptr(k), ptr(v), B, Tq, T, H, precision, ptr(out)))
    return out


def encoder_attention_check(qkv, T: int, H: int, precision: int = wq4.PREC_F16X2):
    """Encoder self-attention through the product kernel (wa_encoder_attention_check):
    qkv cuda f32 [B*T, 3*64H] -> [B*T, 64H]."""
    torch = _torch()
    qkv = qkv.contiguous()
    B = qkv.shape[0] // T
    out = torch.empty((B * T, 64 * H), device=qkv.device, dtype=torch.float32)
    check(lib().wa_encoder_attention_check(_dev(qkv), _ptr(qkv), B, T, H, precision, _ptr(out)))
    return out


def self_attention_check(qkv, cache_k, cache_v, Tq: int, H: int, kv_len: int, precision: int = wq4.PREC_F16X2,
                         anc=None, pad=None, f32_out: bool = False):
    """The decode step's self-attention through the product kernel
    (wa_self_attention_check): qkv cuda f32 [R*Tq, 3*64H]; caches [R, H, ctx,
    64] (updated in place: the new keys / values appended at kv_len) ->
    [R*Tq, 64H].  pad (host int32 [R]): the pad form of a prompted step, row r
    attends slots [pad[r], kv_len].  anc (cuda int32 [R, ctx]; Tq = 1): the beam
    step's kernel, key j of row r read from cache row anc[r, j].  f32_out: the
    f32-row form of range tier 3."""
    torch = _torch()
    R, _, ctx, _ = cache_k.shape
    if anc is not None:
        assert anc.dtype == torch.int32 and anc.is_contiguous() and tuple(anc.shape) == (R, ctx)
    if pad is not None:
        pad = _i32(pad)
        assert pad.size == R
    out = torch.empty((R * Tq, 64 * H), device=qkv.device, dtype=torch.float32)
    check(lib().wa_self_attention_check(_dev(qkv), _ptr(qkv.contiguous()), _ptr(cache_k), _ptr(cache_v),
                                        None if anc is None else _ptr(anc),
                                        None if pad is None else _as(pad, ctypes.c_int32), R, Tq, H, ctx, kv_len,
                                        precision, 1 if f32_out else 0, _ptr(out)))
    return out


def self_attention_pad_check(qkv, cache_k, cache_v, H: int, kv_len: int, pad, precision: int = wq4.PREC_F16X2):
    """self_attention_check with Tq = 1 in the pad form of a prompted decode step."""
    return self_attention_check(qkv, cache_k, cache_v, 1, H, kv_len, precision, pad=_i32(pad))


def self_attention_beam_check(qkv, cache_k, cache_v, anc, H: int, kv_len: int, precision: int = wq4.PREC_F16X2,
                              f32_out: bool = False):
    """The beam step's self-attention; anc None: the kernel of self_attention_check itself."""
    return self_attention_check(qkv, cache_k, cache_v, 1, H, kv_len, precision, anc=anc, f32_out=f32_out)


def self_attention_beam_pad_check(qkv, cache_k, cache_v, anc, pad, H: int, kv_len: int,
                                  precision: int = wq4.PREC_F16X2, f32_out: bool = False):
    """self_attention_beam_check in the pad form of a prompted beam step."""
    assert anc is not None
    return self_attention_check(qkv, cache_k, cache_v, 1, H, kv_len, precision, anc=anc, pad=_i32(pad),
                                f32_out=f32_out)


def self_attention_prefill_check(qkv, cache_k, cache_v, P: int, pad, H: int, precision: int = wq4.PREC_F16X2):
    """The prefill's self-attention (wa_self_attention_prefill_check): qkv cuda
    f32 [B*P, 3*64H], pad host int32 [B] (clip b's rows are [pad[b], P)); caches
    [B, H, ctx, 64], slots pad[b] .. P-1 written in place -> [B*P, 64H]."""
    torch = _torch()
    B, _, ctx, _ = cache_k.shape
    pad = _i32(pad)
    assert pad.size == B and qkv.shape[0] == B * P
    out = torch.empty((B * P, 64 * H), device=qkv.device, dtype=torch.float32)
    check(lib().wa_self_attention_prefill_check(_dev(qkv), _ptr(qkv.contiguous()), _ptr(cache_k), _ptr(cache_v), B, P,
                                                _as(pad, ctypes.c_int32), H, ctx, precision, _ptr(out)))
    return out


def cross_attention_prefill_check(q, k, v, P: int, precision: int = wq4.PREC_F16X2):
    """The prefill's cross-attention (wa_cross_attention_prefill_check): q cuda
    f32 [B*P, 64H], k / v head-major [B, H, T, 64] -> [B*P, 64H]."""
    torch = _torch()
    B, H, T, _ = k.shape
    assert q.shape == (B * P, 64 * H) and k.is_contiguous() and v.is_contiguous()
    out = torch.empty((B * P, 64 * H), device=q.device, dtype=torch.float32)
    check(lib().wa_cross_attention_prefill_check(_dev(q), _ptr(q.contiguous()), _ptr(k), _ptr(v), B, P, T, H,
                                                 precision, _ptr(out)))
    return out


# ---- conv stem and embedding -------------------------------------------------
def conv_gelu_check(x, w, bias, stride: int, pos=None, out=None):
    """The conv stem's kernel (wa_conv_gelu_check): x cuda f32 of logical shape
    [B, C, T_in] in any element strides (x.stride(): channel-major as the mel,
    or a permuted [B, T_in, C] as conv1's output), w cuda f32 [N, C, 3], bias
    [N], pos [T_out, N] or None -> [B, T_out, N] = gelu(conv1d(x) + bias)
    (+ pos), padding 1."""
    torch = _torch()
    B, C, T_in = x.shape
    N = w.shape[0]
    assert tuple(w.shape) == (N, C, 3)
    T_out = (T_in - 1) // stride + 1
    if out is None:
        out = torch.empty((B, T_out, N), device=x.device, dtype=torch.float32)
    bs, cs, ts = x.stride()
    w, bias = w.contiguous(), bias.contiguous()
    pos = None if pos is None else pos.contiguous()
    check(lib().wa_conv_gelu_check(_dev(x), _ptr(x), bs, cs, ts, B, C, T_in, stride, _ptr(w), _ptr(bias),
                                   None if pos is None else _ptr(pos), N, _ptr(out)))
    return out


def embed_check(tokens, tok_emb, pos_emb, B: int, Tq: int, pos0: int, use_state: bool = False, gamma=None,
                precision: int = wq4.PREC_F16X2, x=None, tiled=None, stats=None, pad=None):
    """The decoder's embedding kernels (wa_embed_check): tokens host int32
    [B * Tq], tok_emb cuda f32 [V, D], pos_emb cuda f32 [ctx, D] -> x
    [B * Tq, D]; the position reaches the kernel from the host or, with
    use_state, from a device-resident decode state.  pad (host int32 [B]): the
    pad form, clip b's rows get positions pos0 + t - pad[b].  With gamma (cuda
    f32 [D]) the LayerNorm-fold producer form: also (tiled, stats) = the A-tiled
    operand bytes of x * gamma and the 16-column tile statistics [B * Tq, D /
    16, 2].  x / tiled / stats: caller-allocated outputs (guarded buffers)."""
    torch = _torch()
    V, D = tok_emb.shape
    ctx = pos_emb.shape[0]
    tokens = np.ascontiguousarray(tokens, np.int32)
    assert tokens.size == B * Tq and tok_emb.is_contiguous() and pos_emb.is_contiguous()
    if pad is not None:
        pad = _i32(pad)
        assert pad.size == B
    R = B * Tq
    if x is None:
        x = torch.empty((R, D), device=tok_emb.device, dtype=torch.float32)
    if gamma is not None:
        if tiled is None:
            tiled = torch.zeros(wq4.lib().wq4_atiled_bytes(R, D, precision), device=tok_emb.device, dtype=torch.uint8)
        if stats is None:
            stats = torch.empty((R, D // 16, 2), device=tok_emb.device, dtype=torch.float32)
    check(lib().wa_embed_check(_dev(tok_emb), _as(tokens, ctypes.c_int32), _ptr(tok_emb), V, _ptr(pos_emb), ctx, B, Tq,
                               D, pos0, 1 if use_state else 0, None if pad is None else _as(pad, ctypes.c_int32),
                               None if gamma is None else _ptr(gamma), precision, _ptr(x),
                               None if gamma is None else _ptr(tiled), None if gamma is None else _ptr(stats)))
    return x, tiled, stats


def embed_pad_check(tokens, tok_emb, pos_emb, B: int, Tq: int, pos0: int, pad, use_state: bool = False, gamma=None,
                    precision: int = wq4.PREC_F16X2):
    """embed_check in the pad form: pad host int32 [B]."""
    return embed_check(tokens, tok_emb, pos_emb, B, Tq, pos0, use_state, gamma, precision, pad=_i32(pad))


# ---- the picks ---------------------------------------------------------------
def timestamp_rule(tokens, ts0: int, V: int, max_initial: int = 50) -> np.ndarray:
    """The rule record (8 int32, RULE_FIELDS) after one clip's sampled tokens
    (wa_timestamp_rule; host only)."""
    toks = _i32(tokens)
    rec = np.zeros(8, np.int32)
    check(lib().wa_timestamp_rule(_as(toks, ctypes.c_int32), int(toks.size), int(ts0), int(V), int(max_initial),
                                  _as(rec, ctypes.c_int32)))
    return rec


def _records(histories, ts0: int, V: int, max_initial: int):
    """Each row's sampled tokens so far -> its rule records int32 [R, 8]; None stays None."""
    if histories is None:
        return None
    return np.ascontiguousarray(np.stack([timestamp_rule(h, ts0, V, max_initial) for h in histories]), np.int32)


def _sampling_arrays(temperature, seed, n: int):
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(temperature, np.float32), (n,)))
    s = np.ascontiguousarray(np.broadcast_to(np.asarray(seed, np.uint64), (n,)))
    return t, s


def _id_list(ids):
    a = np.ascontiguousarray(ids, np.int32).reshape(-1)
    return a, (a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a.size else None), int(a.size)


def _pick_args(n: int, ids, temperature, seed, records):
    """The host arrays both pick entries take (kept alive by the caller) and their pointers."""
    keep = [_id_list(ids)]
    t = s = None
    if temperature is not None:
        t, s = _sampling_arrays(temperature, seed, n)
    rec = None if records is None else np.ascontiguousarray(records, np.int32)
    assert rec is None or rec.shape == (n, 8)
    keep += [t, s, rec]
    opt = lambda a, ct: None if a is None else _as(a, ct)
    return keep, keep[0][1], keep[0][2], opt(t, ctypes.c_float), opt(s, ctypes.c_uint64), opt(rec, ctypes.c_int32)


def _opt_ptr(t):
    return None if t is None else _ptr(t)


def logits_pick_check(hid, emb, step: int, ids=(), temperature=None, seed=None, ts0: int = 0, records=None,
                      precision: int = wq4.PREC_F16X2, scored: bool = True, want_logits: bool = True, logprob=None):
    """The decode step's fused logits + pick (wa_logits_pick_check): hid cuda f32
    [B, D], emb cuda f32 [V, D] -> (tokens int32 [B], logprob f32 [B] or None,
    logits [B, V] as the workgroups saw them or None, mass int32 [B] or None).
    Greedy (scored False: no log-probability), scored, under the timestamp
    rules (records int32 [B, 8]), sampled at pick index step + 1 (temperature /
    seed per row), each under the suppress list `ids`.  logprob: an optional
    cuda f32 buffer of >= B entries to write into."""
    torch = _torch()
    B, D = hid.shape
    V = emb.shape[0]
    keep, idp, n_ids, tp, sdp, recp = _pick_args(B, ids, temperature, seed, records)
    tok = torch.empty(B, device=hid.device, dtype=torch.int32)
    lp = logprob
    if lp is None and (scored or tp is not None or recp is not None):
        lp = torch.empty(B, device=hid.device, dtype=torch.float32)
    mass = torch.zeros(B, device=hid.device, dtype=torch.int32) if recp is not None else None
    lg = torch.empty((B, V), device=hid.device, dtype=torch.float32) if want_logits else None
    check(lib().wa_logits_pick_check(_dev(hid), _ptr(hid.contiguous()), _ptr(emb.contiguous()), B, D, V, step,
                                     precision, idp, n_ids, tp, sdp, int(ts0), recp, _ptr(tok), _opt_ptr(lp),
                                     _opt_ptr(mass), _opt_ptr(lg)))
    return tok, lp, lg, mass


def _rule_f(lg, mass, ts0: int):
    """Rule f's mask of [0, ts0), applied to the traced rows where the kernel reports it."""
    if mass is not None:
        lg[mass.bool(), :ts0] = float("-inf")


def logits_argmax_check(hid, emb, step: int, precision: int = wq4.PREC_F16X2, want_logits: bool = True):
    """The greedy form -> (tokens int32 [B], logits [B, V] as the pick saw them, or None)."""
    tok, _, lg, _ = logits_pick_check(hid, emb, step, precision=precision, scored=False, want_logits=want_logits)
    return tok, lg


def logits_logprob_check(hid, emb, step: int, precision: int = wq4.PREC_F16X2, want_logits: bool = True,
                         logprob=None):
    """The scored form -> (tokens, logprob = log softmax(z)[token] over the masked row, logits or None)."""
    return logits_pick_check(hid, emb, step, precision=precision, want_logits=want_logits, logprob=logprob)[:3]


def logits_timestamp_check(hid, emb, histories, step: int, ts0: int, max_initial: int = 50,
                           precision: int = wq4.PREC_F16X2, logprob=None):
    """The timestamp form; histories = each row's sampled tokens so far -> (tokens, logprob, logits as the
    pick saw them: rule f's mask applied here, mass)."""
    rec = _records(histories, ts0, emb.shape[0], max_initial)
    tok, lp, lg, mass = logits_pick_check(hid, emb, step, ts0=ts0, records=rec, precision=precision, logprob=logprob)
    _rule_f(lg, mass, ts0)
    return tok, lp, lg, mass


def logits_sample_check(hid, emb, temperature, seed, step: int, histories=None, ts0: int = 0,
                        max_initial: int = 50, precision: int = wq4.PREC_F16X2):
    """The sampled form at pick index step + 1; histories selects the timestamp form -> (tokens, logprob,
    logits without noise, rule f's mask applied here, mass or None)."""
    rec = _records(histories, ts0, emb.shape[0], max_initial)
    tok, lp, lg, mass = logits_pick_check(hid, emb, step, temperature=temperature, seed=seed, ts0=ts0, records=rec,
                                          precision=precision)
    _rule_f(lg, mass, ts0)
    return tok, lp, lg, mass


def logits_suppress_check(hid, emb, ids, step: int, ts0: int = 50365, temperature=None, seed=None, histories=None,
                          max_initial: int = 50, precision: int = wq4.PREC_F16X2, scored: bool = True):
    """Any form under the suppress list `ids` -> (tokens, logprob or None, logits as the kernel's masks a-e
    and the list left them, mass or None)."""
    rec = _records(histories, ts0, emb.shape[0], max_initial)
    return logits_pick_check(hid, emb, step, ids, temperature, seed, ts0, rec, precision, scored)


def row_pick_check(logits, ids=(), ts0: int = 0, suppress_eot: bool = False, pick: int = 0, temperature=None,
                   seed=None, records=None, scored: bool = True, logprob=None):
    """The picks from stored logits (wa_row_pick_check): logits cuda f32 [R, V]
    -> (tokens int32 [R], logprob f32 [R] or None, mass int32 [R] or None).
    Without temperature and records the argmax kernel and, scored, the
    row-logprob kernel over the masked row; else the row-pick kernel under the
    timestamp rules (records) and / or sampled at pick index `pick`; each under
    the suppress list `ids`.  logprob: an optional cuda f32 buffer to write into."""
    torch = _torch()
    logits = logits.contiguous()
    R, V = logits.shape
    keep, idp, n_ids, tp, sdp, recp = _pick_args(R, ids, temperature, seed, records)
    picked = tp is not None or recp is not None
    tok = torch.empty(R, device=logits.device, dtype=torch.int32)
    lp = logprob
    if lp is None and (scored or picked):
        lp = torch.empty(R, device=logits.device, dtype=torch.float32)
    mass = torch.zeros(R, device=logits.device, dtype=torch.int32) if picked else None
    check(lib().wa_row_pick_check(_dev(logits), _ptr(logits), R, V, 1 if suppress_eot else 0, int(pick), idp, n_ids,
                                  tp, sdp, int(ts0), recp, _ptr(tok), _opt_ptr(lp), _opt_ptr(mass)))
    return tok, lp, mass


def row_timestamp_check(logits, histories, ts0: int, suppress_eot: bool = False, max_initial: int = 50):
    """The stored-logits pick under the timestamp rules -> (tokens, logprob, mass)."""
    rec = _records(histories, ts0, logits.shape[1], max_initial)
    return row_pick_check(logits, ts0=ts0, suppress_eot=suppress_eot, records=rec)


def row_sample_check(logits, temperature, seed, pick: int, suppress_eot: bool = False, histories=None, ts0: int = 0,
                     max_initial: int = 50):
    """The stored-logits sampled pick at pick index `pick`; histories selects the timestamp form."""
    rec = _records(histories, ts0, logits.shape[1], max_initial)
    return row_pick_check(logits, (), ts0, suppress_eot, pick, temperature, seed, rec)


def row_suppress_check(logits, ids, ts0: int = 50365, suppress_eot: bool = False, pick: int = 0, temperature=None,
                       seed=None, histories=None, max_initial: int = 50):
    """The stored-logits picks under the suppress list `ids` -> (tokens, logprob, mass or None)."""
    rec = _records(histories, ts0, logits.shape[1], max_initial)
    return row_pick_check(logits, ids, ts0, suppress_eot, pick, temperature, seed, rec)


def row_logprob_check(logits, lo: int, hi: int, mask_eot: bool = False, idx=None, fixed_idx: int = 0):
    """The row kernel of the stored-logits scores (wa_row_logprob_check):
    logits cuda f32 [R, V] -> f32 [R], z[id] - logsumexp(z[lo:hi]) per row,
    id = idx[row] (cuda int32 [R]) or fixed_idx; EOT counts as -inf with mask_eot."""
    torch = _torch()
    logits = logits.contiguous()
    R, V = logits.shape
    out = torch.empty(R, device=logits.device, dtype=torch.float32)
    check(lib().wa_row_logprob_check(_dev(logits), _ptr(logits), R, V, lo, hi, 1 if mask_eot else 0,
                                     _ptr(idx.contiguous()) if idx is not None else None, int(fixed_idx), _ptr(out)))
    return out


def timestamp_bookkeep_check(tokens, ts0: int, V: int, max_initial: int = 50, device: int = 0) -> np.ndarray:
    """Token sequences int32 [R, S] through the timestamp bookkeeping kernel,
    one token per row and launch (wa_timestamp_bookkeep_check) -> the rule
    records after each launch, int32 [S, R, 8]."""
    toks = np.ascontiguousarray(tokens, np.int32)
    R, S = toks.shape
    out = np.zeros((S, R, 8), np.int32)
    check(lib().wa_timestamp_bookkeep_check(device, _as(toks, ctypes.c_int32), R, S, int(ts0), int(V),
                                            int(max_initial), _as(out, ctypes.c_int32)))
    return out


# ---- beam search -------------------------------------------------------------
def beam_topk_check(logits, kp: int, step: int = -1, suppress_eot: bool = False, eot_stop: bool = True, tok=None,
                    lp=None, ids=(), ts0: int = 0, records=None, mass=None):
    """The per-row log-softmax + top-kp kernel (wa_beam_topk_check): logits cuda
    f32 [R, V] -> (tokens int32 [R, kp], log-probabilities f32 [R, kp], range
    flag).  EOT is masked when not eot_stop, else suppress_eot (step < 0) or
    step + 1 < 3 through a device state.  records (int32 [R, 8], with ts0): the
    kernel under the timestamp rules, mass (cuda int32 [R], optional) then 1
    where rule f fired; ids (with ts0): a suppress list.  tok / lp / mass:
    output tensors to write into (flat)."""
    torch = _torch()
    logits = logits.contiguous()
    R, V = logits.shape
    _keep, idp, n_ids = _id_list(ids)
    rec = None if records is None else np.ascontiguousarray(records, np.int32)
    assert rec is None or rec.shape == (R, 8)
    if tok is None:
        tok = torch.empty((R, kp), device=logits.device, dtype=torch.int32)
    if lp is None:
        lp = torch.empty((R, kp), device=logits.device, dtype=torch.float32)
    flag = ctypes.c_int32(0)
    check(lib().wa_beam_topk_check(_dev(logits), _ptr(logits), R, V, kp, 1 if suppress_eot else 0, step,
                                   1 if eot_stop else 0, int(ts0), idp, n_ids,
                                   None if rec is None else _as(rec, ctypes.c_int32), _ptr(tok), _ptr(lp),
                                   _opt_ptr(mass), ctypes.byref(flag)))
    return tok, lp, int(flag.value)


def beam_topk_rules_check(logits, kp: int, records, ts0: int, step: int = -1, suppress_eot: bool = False,
                          eot_stop: bool = True, tok=None, lp=None, mass=None):
    """beam_topk_check under the timestamp rules -> (tokens, log-probabilities, mass, range flag)."""
    assert records is not None
    if mass is None:
        mass = _torch().empty(logits.shape[0], device=logits.device, dtype=_torch().int32)
    tok, lp, flag = beam_topk_check(logits, kp, step, suppress_eot, eot_stop, tok, lp, (), ts0, records, mass)
    return tok, lp, mass, flag


def beam_topk_suppress_check(logits, kp: int, ids, ts0: int = 50365, records=None, step: int = -1,
                             suppress_eot: bool = False, eot_stop: bool = True):
    """beam_topk_check (records None) / beam_topk_rules_check under the suppress list `ids`
    -> (tokens, log-probabilities, mass or None, range flag)."""
    torch = _torch()
    mass = torch.empty(logits.shape[0], device=logits.device, dtype=torch.int32) if records is not None else None
    tok, lp, flag = beam_topk_check(logits, kp, step, suppress_eot, eot_stop, None, None, ids, ts0, records, mass)
    return tok, lp, mass, flag


def beam_select_check(arrays: dict, n_clips: int, K: int, C: int, ctx: int, records=None, ts0: int = 0,
                      V: int = 0) -> None:
    """One merge step of the beam search in place on the caller's cuda tensors
    (wa_beam_select_check; BEAM_SELECT_ARRAYS names them, shapes in
    include/whisper_amd_checks.h): consecutive calls are consecutive steps.
    records (cuda int32 [rows, 8], with ts0 and V): the rows' rule records,
    advanced in place."""
    t = [arrays[k] for k in BEAM_SELECT_ARRAYS]
    assert all(x.is_cuda and x.is_contiguous() for x in t)
    assert records is None or (records.is_cuda and records.is_contiguous())
    check(lib().wa_beam_select_check(_dev(t[0]), *[_ptr(x) for x in t], _opt_ptr(records), int(ts0), int(V), n_clips,
                                     K, C, ctx))


def beam_select_rules_check(arrays: dict, n_clips: int, K: int, C: int, ctx: int, ts0: int, V: int) -> None:
    """beam_select_check with the rows' rule records, arrays["records"] (None: the plain launch)."""
    beam_select_check(arrays, n_clips, K, C, ctx, arrays.get("records"), ts0, V)


# ---- token alignment ---------------------------------------------------------
def align_matrix_check(q, k, P: int, pad, heads, F, first_row: int = 0, precision: int = wq4.PREC_F16X2):
    """The alignment's weights and filter kernels (wa_align_matrix_check): q cuda
    f32 [B*P, 64H], k head-major [B, H, T, 64], pad / F host [B], heads the
    layer's alignment heads -> cuda f32 [B, P, T]: row i of clip b is M of its
    position first_row + i, zero past its N rows and F frames."""
    torch = _torch()
    B, H, T, _ = k.shape
    pad, heads, F = _i32(pad), _i32(heads), _i32(F)
    assert q.shape == (B * P, 64 * H) and k.is_contiguous() and pad.size == B and F.size == B
    out = torch.empty((B, P, T), device=q.device, dtype=torch.float32)
    check(lib().wa_align_matrix_check(_dev(q), _ptr(q.contiguous()), _ptr(k), B, P, _as(pad, ctypes.c_int32), T, H,
                                      _as(heads, ctypes.c_int32), heads.size, _as(F, ctypes.c_int32), first_row,
                                      precision, _ptr(out)))
    return out


def dtw_check(x, N, F, jump=None, want_trace: bool = True):
    """The alignment's DTW kernel (wa_dtw_check): x cuda f32 [B, N_ld, F_ld]
    costs, N / F host [B] -> (jump cuda int32 [B, N_ld], entries < N[b] written,
    trace cuda uint8 [B, N_ld + 1, F_ld + 1] or None).  jump: a cuda int32
    buffer of at least B * N_ld entries to write into."""
    torch = _torch()
    B, N_ld, F_ld = x.shape
    N, F = _i32(N), _i32(F)
    assert x.is_contiguous() and x.dtype == torch.float32 and N.size == B and F.size == B
    if jump is None:
        jump = torch.full((B, N_ld), -1, device=x.device, dtype=torch.int32)
    assert jump.dtype == torch.int32 and jump.is_contiguous() and jump.numel() >= B * N_ld
    trace = torch.full((B, N_ld + 1, F_ld + 1), 255, device=x.device, dtype=torch.uint8) if want_trace else None
    check(lib().wa_dtw_check(_dev(x), _ptr(x), B, N_ld, F_ld, _as(N, ctypes.c_int32), _as(F, ctypes.c_int32),
                             _ptr(jump), _opt_ptr(trace)))
    return jump, trace
