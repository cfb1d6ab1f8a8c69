"""Float64 restatement of the token alignment (include/whisper_amd.h "Token
alignment", OpenAI timing.py find_alignment), an f32 DTW bit-faithful to the
stated rule, a first-order per-element error bound for M, planted inputs, and
the oracle subclass that records the decoder's cross-attention operands.
numpy only, no GPU: test_align_ref.py checks the restatement against a
transliteration of OpenAI's lines; test_align_gpu.py holds the kernels to it.

The bound (DESIGN.md section 5 "Token alignment"), per head, n positions x F frames:
  scores   d s_tf <= 2 E_tf, E the operand bound of attn_ref._sdpa_block (the
           f16 pairs of q / 8 log2(e) x 2^5 and k x 2^5: 2^-22 sum|q k| / 8, the
           flushed lo halves, and hi_worst of every element at WQ4_PREC_F16)
  softmax  d w_tf <= w_tf (d s_tf + sum_u w_tu d s_tu) + w_tf (r_tf + sum_u w_tu r_tu) + 2^-125
           r = C_REL + ln 2 x 2^-24 (|log2 e_tf| + 2): exp2, the compensated sum
           and the division (C_REL), and the one f32 rounding of the exponent's
           argument, which is absolute in the exponent; 2^-125: f32 underflow
  z        z = (w - mu) / sd per frame column over the n positions:
           d z_t <= (d w_t + mean_u d w_u) / sd + |z_t| mean_u(|z_u| d w_u) / sd + 2^-23 |z_t|
           (d mu = mean d w; d sd = mean(z d w)); a column with sd == 0 is
           exact when every position carries the same query, else unbounded
  median   of 7 is 1-Lipschitz in the maximum norm: the largest d z of the window
  mean     over heads, plus (heads + 1) 2^-24 mean_h |median|: the f32 sums
"""
from __future__ import annotations

import numpy as np

import attn_ref as A
import whisper_oracle
from front_ref import _flushed_lo

LN2 = float(np.log(2.0))
UNDERFLOW = 2.0**-125
BLOCK = 16          # positions per planted direction
DIAG_CONTRAST = 6.0  # the planted diagonal's height over its row's family scores (natural units)
DIAG_SHARP = 8.0    # the height of diagonal_head's bumps
JUNK = 40.0         # the score planted in frames >= F, which the softmax must not see


# ------------------------------------------------------------ restatement --
def weights64(q, k):
    """softmax_f(q . k / 8): q [n, 64], k [F, 64] -> (w [n, F], e = exp(s - max))."""
    return A.softmax64(np.asarray(q, np.float64) @ np.asarray(k, np.float64).T / 8.0)


def standardise(w):
    """Per frame column, (w - mean) / population std over the positions; std == 0
    gives 0.  The std is 0 exactly when the column's values are all equal (the
    rounded mean of equal float64 values need not equal them, so the test is
    made on the values)."""
    mu, sd = w.mean(axis=0, keepdims=True), w.std(axis=0, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(constant_columns(w), 0.0, (w - mu) / sd)


def constant_columns(w):
    return (w == w[:1]).all(axis=0, keepdims=True)


def _window_index(F):
    """[F, 7] frame indices of the median's window, reflect padding of 3."""
    assert F >= 4
    g = np.arange(F)[:, None] + np.arange(-3, 4)[None, :]
    g = np.abs(g)
    return np.where(g > F - 1, 2 * (F - 1) - g, g)


def median7(z):
    """Median of 7 along the last axis with reflect padding of 3."""
    return np.sort(z[..., _window_index(z.shape[-1])], axis=-1)[..., 3]


def window_max(z):
    return z[..., _window_index(z.shape[-1])].max(axis=-1)


def matrix64(heads, first_row):
    """heads: [(q [n, 64], k [F, 64])] of the alignment heads -> M [n - 1 - first_row, F]."""
    acc = 0.0
    for q, k in heads:
        acc = acc + median7(standardise(weights64(q, k)[0]))
    return (acc / len(heads))[first_row:-1]


def dtw(x, dtype=np.float32):
    """The stated DTW over x [N, F] in `dtype`, one add per cell, by
    anti-diagonals -> (jump [N], trace uint8 [N + 1, F + 1])."""
    x = np.asarray(x, dtype)
    N, F = x.shape
    cost = np.full((N + 1, F + 1), np.inf, dtype)
    cost[0, 0] = 0
    trace = np.full((N + 1, F + 1), 255, np.uint8)
    for d in range(2, N + F + 1):
        i = np.arange(max(1, d - F), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
        cost[i, j] = (x[i - 1, j - 1] + c).astype(dtype)
        trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    return backtrace(trace), trace


def dtw_loops(x, dtype=np.float32):
    """The same rule as two plain loops (the form of OpenAI's dtw_cpu)."""
    x = np.asarray(x, dtype)
    N, F = x.shape
    cost = np.full((N + 1, F + 1), np.inf, dtype)
    cost[0, 0] = 0
    trace = np.full((N + 1, F + 1), 255, np.uint8)
    for j in range(1, F + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = dtype(x[i - 1, j - 1]) + c
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    return backtrace(trace), trace


def backtrace(trace):
    """jump [N]: the frame of the first path point of every row, forward order."""
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    jump = np.full(i, -1, np.int32)
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            jump[i - 1] = j - 1
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return jump


def align_words(jump, word_lens):
    bnd = np.concatenate([[0], np.cumsum(word_lens)])
    assert bnd[-1] == len(jump) - 1
    t = np.asarray(jump, np.float64) / 50.0
    return t[bnd[:-1]], t[bnd[1:]]


# ------------------------------------------------------------------ bound --
def head_bound(q, k, prec):
    """(median7(z) [n, F], its bound [n, F]) of one head."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    w, e = weights64(q, k)
    aq, ak = np.abs(q), np.abs(k)
    Es = A.U2 * (aq @ ak.T) / 8.0
    Es = Es + (_flushed_lo(q, A.Q_SCALE * A.OP_SCALE) @ ak.T + aq @ _flushed_lo(k, A.OP_SCALE).T) / 8.0
    if prec == "f16":
        Es = Es + (A.hi_worst(q, A.Q_SCALE * A.OP_SCALE) @ ak.T + aq @ A.hi_worst(k, A.OP_SCALE).T) / 8.0
    ds = 2.0 * Es
    with np.errstate(divide="ignore"):
        lg = np.abs(np.log2(np.maximum(e, 2.0**-1000)))
    rel = A.C_REL + LN2 * 2.0**-24 * (lg + 2.0)
    dw = w * (ds + (w * ds).sum(axis=1, keepdims=True)) + w * (rel + (w * rel).sum(axis=1, keepdims=True)) + UNDERFLOW
    sd = w.std(axis=0, keepdims=True)
    z = standardise(w)
    same_rows = bool((q == q[:1]).all())
    with np.errstate(invalid="ignore", divide="ignore"):
        dz = (dw + dw.mean(axis=0, keepdims=True)) / sd + np.abs(z) * (np.abs(z) * dw).mean(axis=0, keepdims=True) / sd
        dz = dz + 2.0**-23 * np.abs(z)
        dz = np.where(constant_columns(w), 0.0 if same_rows else np.inf, dz)
    return median7(z), window_max(dz)


def matrix_ref(heads, first_row, prec):
    """heads: [(q, k)] -> (M, bound), each [n - 1 - first_row, F]."""
    med = [head_bound(q, k, prec) for q, k in heads]
    H = len(med)
    M = sum(m for m, _ in med) / H
    bound = sum(b for _, b in med) / H + (H + 1) * 2.0**-24 * sum(np.abs(m) for m, _ in med) / H
    return M[first_row:-1], bound[first_row:-1]


def path_is_stable(M, bound, n_patterns=8, seed=0):
    """The float64 path over -M is the path over -(M +- bound) under n random sign patterns."""
    want = dtw(-M, np.float64)[0]
    rng = np.random.default_rng(seed)
    fin = np.where(np.isfinite(bound), bound, 0.0)
    for _ in range(n_patterns):
        sign = rng.choice([-1.0, 1.0], size=M.shape)
        if not np.array_equal(dtw(-(M + sign * fin), np.float64)[0], want):
            return False
    return True


# ---------------------------------------------------------------- planting --
FAMILIES = ("spike_first", "spike_last", "gauss", "flat", "wide", "just_over", "ramp_down", "ramp_up")


def planted_head(n, F, T, seed, shift, diagonal=True):
    """q [n, 64], k [T, 64] of one (clip, head): every block of 16 positions
    shares a direction with its own attn_ref score family planted over the
    clip's F frames, plus (diagonal) a bump of DIAG_CONTRAST around frame
    (block + 0.5) F / blocks; frames >= F carry JUNK, a score the softmax over
    F frames never sees."""
    rng = np.random.default_rng(seed)
    nb = -(-n // BLOCK)
    blk = np.arange(n) // BLOCK
    fams = [A.rotate(shift + j, FAMILIES) for j in range(nb)]
    if diagonal:  # a flat block has no direction to carry a bump
        fams = [f if f != "flat" else "gauss" for f in fams]
    G = 2.0 * rng.standard_normal((nb, 64))
    G[[f == "flat" for f in fams]] = 0.0
    S = np.full((nb, T), JUNK)
    for j, f in enumerate(fams):
        S[j, :F] = A.family_scores(f, F, A.ENC_SUB, 2 * A.ENC_SUB, rng)
        if diagonal:
            c, sig = (j + 0.5) * F / nb, max(1.0, F / (2.0 * nb))
            S[j, :F] += DIAG_CONTRAST * np.exp(-0.5 * ((np.arange(F) - c) / sig) ** 2)
    a = np.array([1.0 if fams[j] in A.THRESHOLD_FAMILIES else 1.0 - (t % BLOCK) / 160.0 for t, j in enumerate(blk)])
    k = A.plant(G, S, rng.standard_normal((T, 64))).astype(np.float32)
    assert np.abs(k).max() < 2047.0, "planted keys leave the operand range"
    return (a[:, None] * G[blk]).astype(np.float32), k


def diagonal_head(n, F, T, seed):
    """q [n, 64], k [T, 64] of one (clip, head) whose every position has a
    direction of its own (n <= 48) and scores DIAG_SHARP exp(-((f - c_t) /
    sigma)^2 / 2) + 0.2 N(0, 1), c_t = (t + 0.5) F / n, sigma = F / (2 n): the
    bumps of neighbouring positions cross half way, steeply, so the frame at
    which the path changes rows is decided far above the bound."""
    assert n <= 48
    rng = np.random.default_rng(seed)
    G = 2.0 * rng.standard_normal((n, 64))
    f = np.arange(F)[None, :]
    c = ((np.arange(n) + 0.5) * F / n)[:, None]
    S = np.full((n, T), JUNK)
    S[:, :F] = DIAG_SHARP * np.exp(-0.5 * ((f - c) / (F / (2.0 * n))) ** 2) + 0.2 * rng.standard_normal((n, F))
    k = A.plant(G, S, rng.standard_normal((T, 64))).astype(np.float32)
    assert np.abs(k).max() < 2047.0, "planted keys leave the operand range"
    return G.astype(np.float32), k


def matrix_case(P, ns, Fs, T, H, heads, seed, kind="families"):
    """Inputs of align_matrix_check: clip b has ns[b] positions right-aligned in
    P (pad rows hold large junk) and Fs[b] frames; the heads in `heads` are
    planted, the others random.  kind: "families" (planted_head), "diagonal"
    (diagonal_head), "identical" (every position of a clip carries the same
    query).  Returns q [B P, 64 H], k [B, H, T, 64] f32 and per clip the
    heads' [(q, k[:F])]."""
    B = len(ns)
    rng = np.random.default_rng(seed)
    q = (1000.0 * rng.standard_normal((B, P, H, 64))).astype(np.float32)
    k = rng.standard_normal((B, H, T, 64)).astype(np.float32)
    per_clip = []
    for b, (n, F) in enumerate(zip(ns, Fs)):
        hs = []
        for h in heads:
            s = seed * 1000 + b * H + h
            if kind == "diagonal":
                qh, kh = diagonal_head(n, F, T, s)
            else:
                qh, kh = planted_head(n, F, T, s, b * H + h, diagonal=kind != "identical")
            if kind == "identical":
                qh[:] = qh[0]
            q[b, P - n:, h], k[b, h] = qh, kh
            hs.append((qh, kh[:F]))
        per_clip.append(hs)
    return q.reshape(B * P, 64 * H), k, per_clip


# the planted-diagonal case whose path the GPU must reproduce at WQ4_PREC_F16X2
# (test_align_ref.py shows its float64 path survives the bound; the hi-only
# operands of WQ4_PREC_F16 move a score by up to 2^-10 of sum |q k| / 8, a bound
# on M of the order of the crossing bumps' own slope per frame, which no
# contrast outgrows: the rows' crossings scale with it)
DIAGONAL_CASE = dict(P=48, ns=(48, 30), Fs=(300, 750), T=1500, H=6, heads=(1, 4), seed=11, kind="diagonal")
DIAGONAL_FIRST_ROW = 3


# ------------------------------------------------------------------ oracle --
class AlignOracle(whisper_oracle.SynthWhisper):
    """SynthWhisper whose sdpa records the cross-attention operands (q, k per
    layer, [B, heads, n, 64] / [B, heads, T, 64]) of decoder_pass(fresh=True)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cross = None

    def sdpa(self, q, k, v, n_heads, causal):
        if self.cross is not None and not causal:
            B, n, _ = q.shape
            self.cross.append((q.reshape(B, n, n_heads, 64).transpose(0, 2, 1, 3).astype(np.float64),
                               k.reshape(B, k.shape[1], n_heads, 64).transpose(0, 2, 1, 3).astype(np.float64)))
        return super().sdpa(q, k, v, n_heads, causal)

    def align_operands(self, enc, tokens):
        """The cross-attention (q, k) of every decoder layer for one clip's id
        sequence over its encoder output enc [1, T, D]."""
        cache = self.init_cache(enc)
        self.cross = []
        try:
            self.decoder_pass(np.asarray(tokens)[None, :], np.arange(len(tokens)), cache, fresh=True)
            return self.cross
        finally:
            self.cross = None

    def align_ref(self, enc, tokens, pairs, first_row, n_frames, prec="f16x2"):
        """(M, bound) of one clip for the (layer, head) pairs, grouped by layer as wa_align sums them."""
        ops = self.align_operands(enc, tokens)
        F = n_frames // 2
        pairs = sorted(pairs, key=lambda p: p[0])
        return matrix_ref([(ops[l][0][0, h], ops[l][1][0, h, :F]) for l, h in pairs], first_row, prec)
