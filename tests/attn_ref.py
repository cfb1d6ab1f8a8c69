"""Float64 references, planted softmax patterns, per-element error bounds and
numpy emulations of the four attention kernels: encoder self-attention
(encoder_attention_f16_kernel), decoder self-attention (dec_self_attn_kernel),
the cache-free cross-attention (wa_xattn.hip) and the cross-attention over
cached K / V (cross_attn_kv_kernel).  numpy only, no GPU: test_attn_ref.py
shows on the CPU that the bounds accept the kernels' arithmetic and reject
the mistakes they are meant to catch; test_attn_gpu.py holds the kernels to
them.  Derivations: DESIGN.md "Numerics", "Attention against float64 on
planted scores".
"""
from __future__ import annotations

import numpy as np

from front_ref import _flushed_lo, split_f16_pair, violations  # noqa: F401  (violations: re-exported)

LOG2E = 1.4426950408889634
Q_SCALE = float(np.float32(0.125 * LOG2E))  # kEaQScale / kXqScale: 1 / sqrt(64) * log2(e), f32
OP_SCALE = 32.0     # kQKScale, kQtScale, kEncScale, kZnScale: operands enter as x * 2^5
W_SCALE = 4096.0    # kWkScale, kWvScale
ACT_SCALE = 16.0    # kActScale: q rows of xattn_q and every output row (split_act)
P_SCALE = 16384.0   # kPScale
LAZY = 1024.0       # kLazyMax: 1.0 in base-2 units at the scores' 2^10 operand scale
U2 = 2.0**-22       # an f16 pair
U1 = 2.0**-11       # hi alone
XKV_KEYS = 188      # kXkvKeys
XATTN_TC = 16       # kTc
ENC_SUB = 32        # the 32-key sub-tile of the encoder's 64-key tile

# The relative term's constant: the smallest of {1, 2, 5} x 10^-k for which
# every emulated case of test_attn_ref.py stays at or under half its bound
# (test_attn_ref.py test_c_is_the_smallest_admissible shows 2e-7 is not).
C_REL = 5e-7
# Standard deviations of the statistical operand term (pair_ms): roundings of
# different operand elements are independent, so their first-order sum over
# the 64 .. 1280 terms of a product is bounded by K_SIGMA root mean squares
# where the sum of the worst cases would be 10 .. 40 times the error seen.
# Eight: a test compares 10^4 .. 10^5 elements, whose largest error is then
# expected at 4 .. 4.5, and the faithful arithmetic is to stay at half.
K_SIGMA = 8.0
# The flushed-lo terms of the f16x2 cross-attention bound stand for an effect
# the MI355X does not show (MFMA_FLUSHES below) and the emulation does not
# model, so the half criterion does not bear on them: six standard
# deviations, which 10^6 elements all keep with probability 0.998.
K_FLUSH = 6.0
FLUSH = 2.0**-14    # below this an f16 is subnormal: the MFMA reads 0

PRECS = ("f16x2", "f16")

FAMILIES = ("ramp_up", "ramp_down", "creep", "just_over", "brink", "spike_first", "spike_cm1", "spike_c",
            "spike_last", "spike_split_last", "spike_split_first", "tied_spikes", "flat", "wide", "gauss")
# families whose point is which side of the lazy-maximum threshold a score is on
THRESHOLD_FAMILIES = ("creep", "just_over", "brink")
VALUE_FAMILIES = ("gauss", "ones", "marker", "tiny", "large")
SPIKE = 30.0


def family_scores(name, T, c, sb, rng):
    """Target scores (natural units) of T keys.  c: the kernel's chunk length,
    sb: the first key of the second split (c where there is one split).
      ramp_up / ramp_down  +-0.1 t: a rescale in every chunk, the maximum the
                           last valid key / none after the first, the tail
                           underflowing to 0
      creep                0 in the first chunk, 0.68 after (0.98 in base 2):
                           the lazy reference never moves, p = 1.97 throughout
      just_over            0.70 (1.01 in base 2): exactly one move
      brink                0.6930 (0.9998 in base 2): p * 2^15 = 65526 rounds
                           to the f16 infinity, p * 2^14 is half of that
      spike_*              flat 0 with +30 at key 0, c - 1, c, T - 1, sb - 1, sb
      tied_spikes          +30 at one key of the first and of the second split
      flat                 0 (the caller also makes q = 0: the exact mean)
      wide                 12 N(0, 1): near one-hot, a long tail of small p
      gauss                2 N(0, 1): the distribution of the older tests"""
    t = np.arange(T, dtype=np.float64)
    s = np.zeros(T)
    at = lambda k: min(max(k, 0), T - 1)
    if name == "ramp_up":
        s = 0.1 * t
    elif name == "ramp_down":
        s = -0.1 * t
    elif name in THRESHOLD_FAMILIES:
        s[c:] = {"creep": 0.68, "just_over": 0.70, "brink": 0.6930}[name]
    elif name.startswith("spike_"):
        s[at({"first": 0, "cm1": c - 1, "c": c, "last": T - 1, "split_last": sb - 1, "split_first": sb}[name[6:]])] = SPIKE
    elif name == "tied_spikes":
        s[at(c // 2)] = s[at(sb + c // 2)] = SPIKE
    elif name == "wide":
        s = 12.0 * rng.standard_normal(T)
    elif name == "gauss":
        s = 2.0 * rng.standard_normal(T)
    elif name != "flat":
        raise ValueError(name)
    return s


def plant(G, S, e0):
    """Keys with prescribed scores: rows x_t = e0_t + corrections in the span
    of G's rows such that G x_t = 8 S[:, t] (scores are q . k / 8).  G [n, D]
    (n <= D, the zero rows -- flat queries -- left out), S [n, T], e0 [T, D]."""
    G, S, e0 = (np.asarray(a, np.float64) for a in (G, S, e0))
    live = np.abs(G).sum(axis=1) > 0
    if not live.any():
        return e0
    G, S = G[live], S[live]
    return e0 + (8.0 * S.T - e0 @ G.T) @ np.linalg.pinv(G).T


def values(name, T, rng):
    """[T, 64] value rows.  ones: dimensions 32 .. 63 are the constant 1, where
    the output must be 1 (the others stay Gaussian: they see the scores); marker: v[t, 0] = t names the key a spike picked;
    tiny: |v| about 2^-10, below the lo-flush threshold 2^-8 of the x 2^5
    operands; large: |v| up to 2000, inside the documented |x| < 2047."""
    v = rng.standard_normal((T, 64))
    if name == "ones":
        v[:, 32:] = 1.0
    elif name == "marker":
        v[:, 0] = np.arange(T)
    elif name == "tiny":
        v *= 2.0**-10
    elif name == "large":
        v = rng.uniform(-2000.0, 2000.0, (T, 64))
    elif name != "gauss":
        raise ValueError(name)
    return v


def softmax64(s, vis=None):
    s = np.asarray(s, np.float64)
    if vis is not None:
        s = np.where(vis, s, -np.inf)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True), e


def _tail_loss(e):
    """Relative loss of a softmax weight in the P operand (p' * 2^14 as an f16
    pair, p' >= e = exp(s - max)): the lo half is a flushed subnormal below
    p' = 2^-17, the hi half below 2^-28."""
    return np.where(e < 2.0**-28, 1.0, np.where(e < 2.0**-17, U1, 0.0))


def _half_ulp(ax):
    """Half an f16 ulp at |scaled value| ax >= 2^-14."""
    return 2.0 ** (np.floor(np.log2(np.maximum(ax, FLUSH))) - 11.0)


def hi_worst(x, scale):
    """The most x is off as hi alone (WQ4_PREC_F16): half an ulp of the f16
    of x * scale, at most 2^-11 |x|; all of x where that is subnormal."""
    ax = np.abs(np.asarray(x, np.float64)) * scale
    return np.where(ax < FLUSH, ax, _half_ulp(ax)) / scale


def pair_ms(x, scale, prec="f16x2"):
    """Mean square error of an operand element x as the bound lets the MFMA
    read its f16 pair of x * scale (include/wq4.h "Result precision"): the
    remainder x - hi is uniform within half an ulp h of hi and lost where the
    lo half is an f16 subnormal (|x scale| < 2^-3: _flushed_lo's regime) or
    not kept at all (WQ4_PREC_F16): h^2 / 3; otherwise 0 (the pair's own
    2^-22 is in E_t and the product term); all of x where hi itself is
    subnormal."""
    ax = np.abs(np.asarray(x, np.float64)) * scale
    h = _half_ulp(ax)
    ms = np.where((ax < 2.0**-3) | (prec == "f16"), h * h / 3.0, 0.0)
    return np.where(ax < FLUSH, ax * ax, ms) / (scale * scale)


def _out_repr(out, prec):
    """The output's own tiled f16-pair representation (x 2^4)."""
    a = np.abs(out)
    if prec == "f16":  # hi alone: one more independent rounding, K_SIGMA root mean squares (3.5 times its worst case)
        return K_SIGMA * np.sqrt(pair_ms(out, ACT_SCALE, prec)) + 2.0**-28
    return U2 * a + _flushed_lo(out, ACT_SCALE) + 2.0**-28


def sdpa_ref(q, k, v, prec="f16x2", pair=True, vis=None):
    """softmax(q k^T / 8) v in float64 and its per-element bound.  q [n, 64],
    k, v [T, 64] f32; vis [n, T]: which keys a query sees (None = all).
    pair: the kernel forms its products from f16 pairs of x * 2^5 (the
    encoder); False: f32 products (decoder self-attention, the K / V form),
    no operand terms.  Returns (out, bound) [n, 64]:
        bound = c sum_t p_t |v_t|  +  2 sum_t p_t E_t |v_t - out|  +  sum_t p_t d(v_t)
                + sum_t p_t lambda_t |v_t|  +  repr(out)
        E_t   = 2^-22 sum_d |q_d k_td| / 8 + sum_d (d(q_d) |k_td| + |q_d| d(k_td)) / 8
    d(.) = _flushed_lo of the operand, lambda the tail loss of P.  f32
    products: E_t = 2^-23 sum_d |q_d k_td| / 8, i.e. 2 E_t is four f32
    roundings of the whole absolute sum, where the nine of the scaled query,
    the product and the eight adds of a 64-term dot each act on a part of it.
    WQ4_PREC_F16, the hi-only analogue: d(.) becomes hi_worst(.) of every
    element of q, k and v (half an ulp of hi), and P as one f16 adds 2^-11
    sum_t p_t |v_t|."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    out, bound = np.zeros((q.shape[0], v.shape[1])), np.zeros((q.shape[0], v.shape[1]))
    for i in range(0, q.shape[0], 64):  # blocks of queries: the [n, T, 64] deviations stay small
        sl = slice(i, i + 64)
        out[sl], bound[sl] = _sdpa_block(q[sl], k, v, prec, pair, None if vis is None else vis[sl])
    return out, bound


def _sdpa_block(q, k, v, prec, pair, vis):
    p, e = softmax64(q @ k.T / 8.0, vis)
    out = p @ v
    av = np.abs(v)
    sd = v[None, :, :] - out[:, None, :]  # [n, T, 64]
    Es = (U2 if pair else 0.5 * U2) * (np.abs(q) @ np.abs(k).T) / 8.0
    bound = C_REL * (p @ av) + _out_repr(out, prec)
    if pair:
        Es = Es + (_flushed_lo(q, Q_SCALE * OP_SCALE) @ np.abs(k).T + np.abs(q) @ _flushed_lo(k, OP_SCALE).T) / 8.0
        bound = bound + p @ _flushed_lo(v, OP_SCALE) + (p * _tail_loss(e)) @ av
    if pair and prec == "f16":
        Es = Es + (hi_worst(q, Q_SCALE * OP_SCALE) @ np.abs(k).T + np.abs(q) @ hi_worst(k, OP_SCALE).T) / 8.0
        bound = bound + p @ hi_worst(v, OP_SCALE) + U1 * (p @ av)
    bound = bound + 2.0 * np.einsum("nt,ntj->nj", p * Es, np.abs(sd))
    return out, bound


# ------------------------------------------------------------ emulation --
def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _exp2f(x):
    with np.errstate(over="ignore", under="ignore"):
        return _f32(np.exp2(np.asarray(x, np.float64)))


# Whether the emulated MFMA reads f16 subnormal operands as 0, as
# wq4_device.hpp split_act and include/wq4.h say.  On the MI355X it does not:
# encoder attention over one key returns v to 2^-22 |v| also where the lo half
# of v * 2^5 is subnormal, and the cross-attention at the older tests' inputs
# is within 5e-7 max|ref| where this emulation gives 1.2e-5 with the flush and
# 4e-7 without (DESIGN.md "Attention against float64 on planted scores").
# The bound keeps the documented flushed-lo terms; with the flush on, the
# emulation leaves it (test_attn_ref.py test_mfma_flush_would_leave_the_bound):
# a lo half under 2^-14 is lost at any magnitude of x, not only below 2^-3.
MFMA_FLUSHES = False


def pair_op(x, scale, ns=2):
    """(hi, lo) of x * scale as the MFMA reads them; ns = 1 keeps hi alone."""
    with np.errstate(over="ignore", invalid="ignore"):
        if MFMA_FLUSHES:
            hi, lo = split_f16_pair(x, scale)
        else:
            s = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)
            h16 = s.astype(np.float16)
            hi, lo = h16.astype(np.float64), (s - h16.astype(np.float32)).astype(np.float16).astype(np.float64)
    return (hi, lo if ns == 2 else np.zeros_like(lo))


def _prod3(a, b, drop_lo_hi=False):
    """hi hi + lo hi + hi lo of a [.., K] against b [n, K] -> [.., n], one f32 result."""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = a[0] @ b[0].T + a[0] @ b[1].T
        if not drop_lo_hi:
            acc = acc + a[1] @ b[0].T
        return _f32(acc)


def store_pair(out, ns=2):
    """The output as the tiled operand holds it and the check entry reads it back."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (np.asarray(out, np.float64) * ACT_SCALE).astype(np.float32)
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
        r = hi.astype(np.float64) + (lo.astype(np.float64) if ns == 2 else 0.0)
    return r / ACT_SCALE


def merge_partials(M, L, Z, weights="ref", drop=None):
    """Flash merge of partials by their base-2 references (xattn_out, the last
    arriver of the K / V form): Z [n, ...].  weights = "equal": the mistake of
    adding the partials unweighted; drop: one partial left out."""
    keep = [i for i in range(len(M)) if i != drop]
    M, L, Z = np.asarray(M, np.float64)[keep], np.asarray(L, np.float64)[keep], np.asarray(Z, np.float64)[keep]
    if weights == "equal":
        w = np.where(np.isneginf(M), 0.0, 1.0)
    else:
        w = np.where(np.isneginf(M), 0.0, _exp2f(M - M.max()))
    lsum = _f32((w * L).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return _f32(_f32(np.tensordot(w, Z, 1)) / lsum)


def online_pair(a, K, V, splits, c, *, t_valid=None, drop_lo_hi=False, no_rescale=False, extra_frame=False,
                p_single=False, p_scale=P_SCALE, merge="ref", drop_split=None):
    """The lazy-maximum online softmax of xattn_main / the encoder attention
    for one query operand.  a: (hi, lo) [Dk] of the base-2 query x 2^5; K, V:
    (hi, lo) [T, Dk] / [T, Dv] x 2^5; splits: [(t0, t1)] key ranges, each
    walked in chunks of c keys with its own reference; partials merged by
    their references.  Returns sum_t softmax_t V_t [Dv] (f32 values).
    Switches, the mistakes the bound must reject: t_valid (keys >= t_valid
    masked: T - 1 drops the last key), extra_frame (one frame past T counted
    valid in a ragged last chunk, with its zero row), drop_lo_hi (the score
    product without lo hi), no_rescale (Z never rescaled: WA_XATTN_DIAG 5),
    p_single (P as one f16), p_scale, merge / drop_split (merge_partials)."""
    T = K[0].shape[0]
    tv = T if t_valid is None else t_valid
    Ms, Ls, Zs = [], [], []
    for t0, t1 in splits:
        M, L, Z = -np.inf, 0.0, np.zeros(V[0].shape[1])
        for u0 in range(t0, t1, c):
            idx = np.arange(u0, min(u0 + c, t1))
            sv = _prod3((K[0][idx], K[1][idx]), (a[0][None], a[1][None]), drop_lo_hi)[:, 0]
            sv = np.where(idx < tv, sv, -np.inf)
            Vh, Vl = V[0][idx], V[1][idx]
            if extra_frame and u0 + c > T and t1 == T:
                sv = np.append(sv, 0.0)
                Vh, Vl = np.vstack([Vh, 0 * Vh[:1]]), np.vstack([Vl, 0 * Vl[:1]])
            mn = max(M, sv.max())
            if M != -np.inf and mn - M <= LAZY:
                mn = M
            if mn == -np.inf:
                continue
            alpha = _exp2f((M - mn) / 1024.0)
            p = _exp2f((sv - mn) / 1024.0)
            L = _f32(L * alpha + _f32(p.sum()))
            ph, pl = pair_op(p, p_scale)
            if p_single:
                pl = 0 * pl
            if not no_rescale:
                Z = _f32(Z * alpha)
            with np.errstate(invalid="ignore", over="ignore"):
                Z = _f32(Z + ph @ Vh + pl @ Vh + ph @ Vl)
            M = mn
        Ms.append(M / 1024.0)
        Ls.append(L)
        Zs.append(_f32(Z / (p_scale * OP_SCALE)))
    return merge_partials(Ms, Ls, Zs, merge, drop_split)


def encoder_emulate(q, k, v, ns=2, **mistakes):
    """encoder_attention_f16_kernel for the queries q [n, 64] over k, v [T, 64]:
    one range, 32-key sub-tiles, the output through its tiled pair."""
    T = k.shape[0]
    K, V = pair_op(k, OP_SCALE, ns), pair_op(v, OP_SCALE, ns)
    A = pair_op(_f32(np.asarray(q, np.float32).astype(np.float64) * Q_SCALE), OP_SCALE, ns)
    out = [online_pair((A[0][i], A[1][i]), K, V, [(0, T)], ENC_SUB, **mistakes) for i in range(q.shape[0])]
    return store_pair(np.array(out), ns)


def xkv_ranges(T):
    """The K / V form's splits: ceil(T / 188) of them, equal lengths."""
    S = min(32, max(1, -(-T // XKV_KEYS)))
    per = -(-T // S)
    return [(min(T, i * per), min(T, (i + 1) * per)) for i in range(S)]


def _lane_groups(t0, t1):
    """The 16 (wave, 16-lane group) key sets of one workgroup's range."""
    per = -(-(t1 - t0) // 4)
    out = []
    for w in range(4):
        k0 = min(t1, t0 + w * per)
        k1 = min(t1, k0 + per)
        out += [np.arange(k0 + g, k1, 4) for g in range(4)]
    return out


def f32_emulate(q, k, v, splits, vis=None, ns=2, *, no_rescale=False, t_valid=None, merge="ref", drop_split=None):
    """dec_self_attn_kernel / cross_attn_kv_kernel: f32 products, a per-key
    online softmax per 16-lane group, the groups and waves of a workgroup
    merged by their references, then the splits.  q [n, 64], k, v [T, 64];
    vis [n, T] or None."""
    q2 = _f32(np.asarray(q, np.float32).astype(np.float64) * Q_SCALE)
    k, v = _f32(k), _f32(v)
    n, T = q2.shape[0], k.shape[0]
    tv = T if t_valid is None else t_valid
    dots = _f32(q2 @ k.T)
    out = np.zeros((n, 64))
    for i in range(n):
        SM, SL, SZ = [], [], []
        for t0, t1 in splits:
            GM, GL, GZ = [], [], []
            for keys in _lane_groups(t0, t1):
                m, l, o = -np.inf, 0.0, np.zeros(64)
                for j in keys:
                    if j >= tv or (vis is not None and not vis[i, j]):
                        continue
                    mn = max(m, dots[i, j])
                    alpha, p = _exp2f(m - mn), _exp2f(dots[i, j] - mn)
                    l = _f32(l * alpha + p)
                    o = _f32((o if no_rescale else o * alpha) + v[j] * p)
                    m = mn
                GM.append(m), GL.append(l), GZ.append(o)
            GM, GL = np.array(GM), np.array(GL)
            mx = GM.max()
            w = np.where(np.isneginf(GM), 0.0, _exp2f(GM - mx)) if mx > -np.inf else 0 * GL
            SM.append(mx), SL.append(_f32((w * GL).sum())), SZ.append(_f32(np.tensordot(w, np.array(GZ), 1)))
        out[i] = merge_partials(SM, SL, SZ, merge, drop_split)
    return store_pair(out, ns)


def causal_vis(Tq, kv, off=0):
    """Query t of the prompt sees keys <= kv + t (off = 1: the mistake of one more)."""
    return np.arange(kv + Tq)[None, :] <= kv + np.arange(Tq)[:, None] + off


# ------------------------------------------- cache-free cross-attention --
def xattn_splits(T, S, plan=None):
    """Frame ranges of a plan of S splits: wa_xattn_plan_splits' geometry
    (plan = that entry, (T, rows, free_cus) -> (splits, chunks per split);
    None restates it: ch = ceil(nchunk / S), no split empty)."""
    nchunk = -(-T // XATTN_TC)
    S = max(1, min(S, 8, nchunk))
    if plan is not None:
        splits, ch = plan(T, 1, S)
    else:
        ch = -(-nchunk // S)
        splits = -(-nchunk // ch)
    return [(s * ch * XATTN_TC, min(T, (s + 1) * ch * XATTN_TC)) for s in range(splits)]


def xattn_ref(q, wk, wv, bv, enc, Tq, H, prec="f16x2"):
    """K = enc Wk^T, V = enc Wv^T + bv, out_h = softmax(q_h K_h^T / 8) V_h in
    float64 (wk, wv: the dequantised weights) and the per-element bound.
    The kernel's products run over the D encoder columns (qt = Wk_h^T q_h / 8,
    s_t = qt . enc_t, Z = sum_t p_t enc_t, out = Wv_h Z + bv), so
        bound = c sum_t p_t |V_t| + 2 sum_t p_t E_t |V_t - out| + sum_t p_t lambda_t |V_t - bv|
                + 4 x 2^-22 sqrt(sum_t p_t ||Wv_h[j] o enc_t||^2) + repr(out) + K sqrt(T1 + T2 + T3)
        E_t = 2^-22 (||qt o enc_t|| + ||aq o enc_t||),  aq_c = ||q o Wk_h[:, c]|| / 8
        T1  = sum_c W_jc^2 (ms(qt_c) + sum_d ms(q_d) Wk_dc^2 / 64),  W_jc = sum_t p_t (V_tj - out_j) enc_tc
        T2  = sum_t p_t^2 (V_tj - out_j)^2 sum_c qt_c^2 ms(enc_tc)
        T3  = sum_t p_t^2 sum_c Wv_jc^2 ms(enc_tc) + sum_c Wv_jc^2 ms(Zn_c)
    No 64-term product q . K exists in this form: a score is a D-term product
    whose terms each carry up to three roundings of 2^-22 (the two pairs, the
    dropped lo lo), so 2^-22 ||qt o enc_t|| is one standard deviation of
    their sum and 2^-22 ||aq o enc_t|| that of qt's own product; 2 E_t is two
    of each per frame, added over the frames as absolute values.  The value
    side is a D-term product too (V_t never exists): its pair roundings
    per term (enc, P, Zn, the dropped lo lo) give the 4 x 2^-22 term, which
    c |V_t| cannot stand for where V_tj is small by cancellation.  T1 .. T3
    are the flushed lo halves (pair_ms) of qt and q (shared by all frames:
    W), of enc in the scores, and of enc and Zn in the value product.
    K = K_FLUSH.  WQ4_PREC_F16, K = K_SIGMA (xattn_q and xattn_out keep their three-term products; qt's
    store, the encoder planes, P and the output drop the lo half): ms(qt_c)
    and ms(enc_tc) of hi alone, P as one f16 in T3, (2^-22 / 3) sum_t p_t^2
    (V_tj - bv_j)^2, and the output as one f16, ms(out_j).
    Returns (out, bound) [B Tq, 64 H]."""
    B, T, D = enc.shape
    q64 = np.asarray(q, np.float64).reshape(B, Tq, H, 64)
    wk, wv, bv = (np.asarray(a, np.float64) for a in (wk, wv, bv))
    out = np.zeros((B, Tq, H, 64))
    bound = np.zeros_like(out)
    for b in range(B):
        E = np.asarray(enc[b], np.float64)
        E2, msE = E * E, pair_ms(E, OP_SCALE, prec)
        EW2 = (E2 @ (wv * wv).T).reshape(T, H, 64).transpose(1, 0, 2)  # ||Wv_h[j] o enc_t||^2
        msEW = (msE @ (wv * wv).T).reshape(T, H, 64).transpose(1, 0, 2)
        for h in range(H):
            sl = slice(h * 64, (h + 1) * 64)
            Wk, Wv = wk[sl], wv[sl]                      # [64, D]
            K, Vp = E @ Wk.T, E @ Wv.T                   # [T, 64]
            V = Vp + bv[sl]
            for r in range(Tq):
                qh = q64[b, r, h]
                p, e = softmax64(K @ qh / 8.0)
                o = p @ V
                qt = Wk.T @ qh / 8.0
                aq2 = (qh * qh) @ (Wk * Wk) / 64.0
                Es = U2 * (np.sqrt(E2 @ (qt * qt)) + np.sqrt(E2 @ aq2))
                sd = V - o                               # [T, 64]
                Zn = p @ E
                bd = (C_REL * (p @ np.abs(V)) + 2.0 * (p * Es) @ np.abs(sd) + (p * _tail_loss(e)) @ np.abs(Vp)
                      + 4.0 * U2 * np.sqrt(p @ EW2[h]) + _out_repr(o, "f16x2"))
                W = (p[:, None] * sd).T @ E              # [64, D]: d out_j / d qt_c
                ms_qt = pair_ms(qt, LOG2E * OP_SCALE, prec) + pair_ms(qh, ACT_SCALE) @ (Wk * Wk) / 64.0
                t1 = (W * W) @ ms_qt
                t2 = ((p * p) * (msE @ (qt * qt))) @ (sd * sd)
                t3 = (p * p) @ msEW[h] + (Wv * Wv) @ pair_ms(Zn, OP_SCALE)
                if prec == "f16":                        # P and the output as single f16 values
                    t3 = t3 + U1 * U1 / 3.0 * ((p * p) @ (Vp * Vp)) + pair_ms(o, ACT_SCALE, prec)
                bd = bd + (K_SIGMA if prec == "f16" else K_FLUSH) * np.sqrt(t1 + t2 + t3)
                out[b, r, h], bound[b, r, h] = o, bd
    return out.reshape(B * Tq, H * 64), bound.reshape(B * Tq, H * 64)


def xattn_emulate(q, wk, wv, bv, enc, Tq, H, splits, ns=2, *, head_tile_mixup=False, bias_per_key=False, **mistakes):
    """xattn_q, xattn_main, xattn_out on the CPU.  splits: xattn_splits(T, S).
    head_tile_mixup: the second head tile (heads 16 ..) reads the qt of heads
    0 .. 3; bias_per_key: the value bias added once per key instead of once."""
    B, T, D = enc.shape
    qf = np.asarray(q, np.float32).reshape(B, Tq, H, 64)
    out = np.zeros((B, Tq, H, 64))
    WK = pair_op(wk, W_SCALE)  # xattn_q and xattn_out run their three products at either precision
    WV = pair_op(wv, W_SCALE)
    for b in range(B):
        E = pair_op(enc[b], OP_SCALE, ns)
        for r in range(Tq):
            A = []
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                qa = pair_op(qf[b, r, h], ACT_SCALE)
                acc = _prod3((WK[0][sl].T, WK[1][sl].T), (qa[0][None], qa[1][None]))[:, 0]  # [D]
                A.append(pair_op(_f32(acc / (ACT_SCALE * W_SCALE) * Q_SCALE), OP_SCALE, ns))
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                a = A[h - 16] if head_tile_mixup and h >= 16 else A[h]
                Zn = online_pair(a, E, E, splits, XATTN_TC, **mistakes)
                zp = pair_op(Zn, OP_SCALE)
                o = _prod3((WV[0][sl], WV[1][sl]), (zp[0][None], zp[1][None]))[:, 0] / (OP_SCALE * W_SCALE)
                out[b, r, h] = _f32(np.asarray(bv[sl], np.float64) * (T if bias_per_key else 1) + o)
    return store_pair(out.reshape(B * Tq, H * 64), ns)


# ------------------------------------------------------------ the cases --
def rotate(i, names=FAMILIES):
    return names[i % len(names)]


def _row_scores(fam, T, c, sb, rng, t_vis=None):
    """A family over the first t_vis keys (the ones a causal query sees)."""
    tv = T if t_vis is None else t_vis
    s = np.zeros(T)
    s[:tv] = family_scores(fam, tv, c, sb, rng)
    return s


def kv_case(B, Tq, T, H, seed, shift=0):
    """Inputs of xattn_kv_check: a score family per (clip, head, query) and a
    value family per (clip, head), rotated from `shift`.  Returns q [B Tq,
    64 H], k, v [B, H, T, 64] f32 and the names, [B][H] lists of (value
    family, [score family per query])."""
    rng = np.random.default_rng(seed)
    rg = xkv_ranges(T)
    c, sb = rg[0][1], (rg[1][1] if len(rg) > 2 else rg[0][1])
    q = np.zeros((B, Tq, H, 64))
    k, v = np.zeros((B, H, T, 64)), np.zeros((B, H, T, 64))
    names = [[None] * H for _ in range(B)]
    for b in range(B):
        for h in range(H):
            i = shift + (b * H + h) * Tq
            fams = [rotate(i + t) for t in range(Tq)]
            vf = rotate(shift + b * H + h, VALUE_FAMILIES)
            Q = 2.0 * rng.standard_normal((Tq, 64))
            Q[[f == "flat" for f in fams]] = 0.0
            S = np.array([_row_scores(f, T, c, sb, rng) for f in fams])
            k0 = rng.standard_normal((T, 64)) * (2.0**-10 if vf == "tiny" else 1.0)
            q[b, :, h], k[b, h], v[b, h] = Q, plant(Q, S, k0), values(vf, T, rng)
            names[b][h] = (vf, fams)
    f = np.float32
    return q.reshape(B * Tq, H * 64).astype(f), k.astype(f), v.astype(f), names


def self_case(B, Tq, kv, H, seed, shift=0, ctx=448):
    """Inputs of self_attention_check: qkv [B Tq, 3 * 64 H] (the Tq new rows),
    caches [B, H, ctx, 64] holding kv planted keys; query t sees kv + t + 1
    keys and its family is planted over those (spike_last: the key it appends).
    Also returns k, v [B, H, kv + Tq, 64] (cache + new) and the names."""
    rng = np.random.default_rng(seed)
    T, D = kv + Tq, 64 * H
    c = -(-T // 4)  # keys per wave
    sb = min(T - 1, c) if T > 1 else 1
    qkv = np.zeros((B, Tq, 3, H, 64))
    ck, cv = (rng.standard_normal((B, H, ctx, 64)) for _ in range(2))  # what lies past kv must not be read
    k, v = np.zeros((B, H, T, 64)), np.zeros((B, H, T, 64))
    names = [[None] * H for _ in range(B)]
    for b in range(B):
        for h in range(H):
            i = shift + (b * H + h) * Tq
            fams = [rotate(i + t) for t in range(Tq)]
            vf = rotate(shift + b * H + h, VALUE_FAMILIES)
            Q = 2.0 * rng.standard_normal((Tq, 64))
            Q[[f == "flat" for f in fams]] = 0.0
            S = np.array([_row_scores(f, T, c, sb, rng, kv + t + 1) for t, f in enumerate(fams)])
            k0 = rng.standard_normal((T, 64)) * (2.0**-10 if vf == "tiny" else 1.0)
            k[b, h], v[b, h] = plant(Q, S, k0), values(vf, T, rng)
            qkv[b, :, 0, h] = Q
            names[b][h] = (vf, fams)
    f = np.float32
    k, v = k.astype(f), v.astype(f)
    qkv[:, :, 1], qkv[:, :, 2] = k[:, :, kv:].transpose(0, 2, 1, 3), v[:, :, kv:].transpose(0, 2, 1, 3)
    ck, cv = ck.astype(f), cv.astype(f)
    ck[:, :, :kv], cv[:, :, :kv] = k[:, :, :kv], v[:, :, :kv]
    return qkv.reshape(B * Tq, 3 * D).astype(f), ck, cv, k, v, names


ENC_BLOCK = 16  # queries per planted family: two families in every wave's 32 queries


def encoder_case(B, T, H, seed, shift=0):
    """Inputs of encoder_attention_check, qkv [B T, 3 * 64 H]: every block of
    16 queries of a (clip, head) shares a direction g with its own family
    planted in that head's keys (different queries of one wave, and of one
    workgroup, then need different rescales); query i is a_i g, a_i = 1 for
    the threshold families and 1 - (i % 16) / 160 otherwise.  Returns qkv and
    the names, [B][H] lists of (value family, [family per block])."""
    rng = np.random.default_rng(seed)
    D, nb = 64 * H, -(-T // ENC_BLOCK)
    qkv = np.zeros((B, T, 3, H, 64))
    names = [[None] * H for _ in range(B)]
    blk = np.arange(T) // ENC_BLOCK
    for b in range(B):
        for h in range(H):
            i = shift + (b * H + h) * nb
            fams = [rotate(i + j) for j in range(nb)]
            vf = rotate(shift + b * H + h, VALUE_FAMILIES)
            G = 2.0 * rng.standard_normal((nb, 64))
            G[[f == "flat" for f in fams]] = 0.0
            S = np.array([family_scores(f, T, ENC_SUB, 2 * ENC_SUB, rng) for f in fams])
            a = np.array([1.0 if fams[j] in THRESHOLD_FAMILIES else 1.0 - (t % ENC_BLOCK) / 160.0 for t, j in enumerate(blk)])
            k0 = rng.standard_normal((T, 64)) * (2.0**-10 if vf == "tiny" else 1.0)
            qkv[b, :, 0, h] = a[:, None] * G[blk]
            qkv[b, :, 1, h] = plant(G, S, k0)
            qkv[b, :, 2, h] = values(vf, T, rng)
            names[b][h] = (vf, fams)
    return qkv.reshape(B * T, 3 * D).astype(np.float32), names


def encoder_ref(qkv, B, T, H, prec="f16x2"):
    D = 64 * H
    x = qkv.reshape(B, T, 3, H, 64)
    out, bound = np.zeros((B, T, H, 64)), np.zeros((B, T, H, 64))
    for b in range(B):
        for h in range(H):
            out[b, :, h], bound[b, :, h] = sdpa_ref(x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h], prec, True)
    return out.reshape(B * T, D), bound.reshape(B * T, D)


def f32_ref(q, k, v, Tq, prec="f16x2", kv=None):
    """Reference and bound of the two f32 kernels: q [B Tq, 64 H], k, v [B, H,
    T, 64]; kv: the prompt's causal form over kv cached keys (None: every
    query sees every key)."""
    B, H, T, _ = k.shape
    qh = q.reshape(B, Tq, H, 64)
    vis = None if kv is None else causal_vis(Tq, kv)
    out, bound = np.zeros((B, Tq, H, 64)), np.zeros((B, Tq, H, 64))
    for b in range(B):
        for h in range(H):
            out[b, :, h], bound[b, :, h] = sdpa_ref(qh[b, :, h], k[b, h], v[b, h], prec, False, vis)
    return out.reshape(B * Tq, 64 * H), bound.reshape(B * Tq, 64 * H)


XATTN_SCALES = ("unit", "tiny", "large")


def xattn_weights(H, wtype, seed, quantize=None, dequantize=None):
    """Dense random Wk, Wv (the older tests' range) as the raw bytes the entry
    takes and the values they hold; bv.  wtype 0: Q4_0 through `quantize` /
    `dequantize` (wq4.quantize_q4_0, oracle.dequantize_np), 1: f16."""
    D = 64 * H
    rng = np.random.default_rng(seed)
    wk = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
    wv = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
    bv = rng.uniform(-0.02, 0.02, D).astype(np.float32)
    if wtype == 0:
        rk, rv = quantize(wk), quantize(wv)
        wk_d, wv_d = dequantize(rk, D * D).reshape(D, D), dequantize(rv, D * D).reshape(D, D)
    else:
        hk, hv = wk.astype(np.float16), wv.astype(np.float16)
        rk, rv = hk.view(np.uint8).ravel(), hv.view(np.uint8).ravel()
        wk_d, wv_d = hk.astype(np.float32), hv.astype(np.float32)
    return dict(rk=rk, rv=rv, wk=wk_d, wv=wv_d, bv=bv)


def xattn_case(B, Tq, T, H, w, seed, sb, shift=0, scale="unit"):
    """q [B Tq, 64 H] and enc [B, T, 64 H] with a family of its own planted in
    every (query row, head): G's rows are Wk_h^T q_h, enc = e0 + (8 S - e0
    G^T)(G^+)^T.  sb: the first frame of the second split of the plan under
    test.  scale: "tiny" makes |enc| about 2^-10 and "large" max |enc| = 2000
    (q scaled the other way, so the planted scores stay).  Returns q, enc and
    the names [B Tq][H]."""
    rng = np.random.default_rng(seed)
    D = 64 * H
    wk = np.asarray(w["wk"], np.float64)
    q = np.zeros((B, Tq, H, 64))
    enc = np.zeros((B, T, D))
    names = []
    qsd = {"unit": 2.0, "tiny": 0.5, "large": 8.0}[scale]
    for b in range(B):
        G, S = [], []
        for r in range(Tq):
            row = []
            for h in range(H):
                fam = rotate(shift + (b * Tq + r) * 7 + h)
                qh = np.zeros(64) if fam == "flat" else qsd * rng.standard_normal(64)
                q[b, r, h] = qh
                G.append(wk[h * 64:(h + 1) * 64].T @ qh)
                S.append(family_scores(fam, T, XATTN_TC, sb, rng))
                row.append(fam)
            names.append(row)
        enc[b] = plant(np.array(G), np.array(S), rng.standard_normal((T, D)))
    if scale == "tiny":
        sig = 2.0**-10
    elif scale == "large":
        sig = 2000.0 / np.abs(enc).max()
    else:
        sig = 1.0
    return (q / sig).reshape(B * Tq, D).astype(np.float32), (enc * sig).astype(np.float32), names
