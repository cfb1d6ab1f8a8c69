"""Float64 references and error bounds of the model's two ends: the conv stem
(conv_gelu_f16_kernel), LayerNorm (wq4_layernorm) and the decoder embedding
(embed_kernel / embed_fold_kernel).  numpy only, no GPU: test_front_ref.py
shows on the CPU that the bounds accept the kernels' arithmetic and reject
the mistakes they are meant to catch; test_front_gpu.py holds the kernels to
them.  Derivations: DESIGN.md "Numerics".
"""
from __future__ import annotations

import numpy as np

# ------------------------------------------------------------------ conv --
CONV_A_SCALE = 16.0    # kCvAScale: the input enters the MFMA as f16 pairs of a * 2^4
CONV_W_SCALE = 1024.0  # kCvBScale: the weights as f16 pairs of w * 2^10
CONV_C = 1e-6          # relative term of the pre-activation bound
GELU_SLOPE = 1.13      # max |gelu'|

# (B, C, T_in, N, stride, layout, pos, input) of test_front_gpu.py's conv cases
CONV_CASES = [
    (2, 80, 200, 384, 1, "channel", False, "mel"),
    (3, 128, 203, 1280, 1, "channel", False, "mel"),
    (2, 384, 200, 384, 2, "time", True, "gelu"),
    (2, 384, 201, 384, 2, "time", True, "gelu"),
    (2, 1280, 150, 1280, 2, "time", True, "gelu"),
    (1, 80, 3000, 384, 1, "channel", False, "mel"),
]


def lin_scale(k: int) -> float:
    """The loader's synthetic weight range (wa_weights.cpp lin_scale)."""
    return float(np.float32(1.5 / np.sqrt(float(k))))


def gelu64(z):
    """layers.rs:35-41 in float64 as z / (1 + exp(-2u)): no cancellation where tanh u -> -1."""
    z = np.asarray(z, np.float64)
    u = 0.7978845608028654 * (z + 0.044715 * z**3)
    with np.errstate(over="ignore"):
        return z / (1.0 + np.exp(-2.0 * u))


def conv_inputs(case, seed, t_cap=None):
    """Inputs of one conv case as the model sees them: x [B, C, T_in] f32 (mel
    range, or conv1's output gelu(2 N(0, 1))), w [N, C, 3] uniform within
    +-lin_scale(3C) with a few weights planted below 2^-13 and row `zero_row`
    zeroed, bias [N], pos [2 T_out, N] or None (the table proper is its first
    T_out rows; the rest is what a wrong clip offset would read).  t_cap cuts
    T_in (keeping its parity) for the CPU tests."""
    B, C, T_in, N, stride, layout, has_pos, kind = case
    if t_cap is not None and T_in > t_cap:
        T_in = t_cap - ((t_cap - T_in) & 1)
    rng = np.random.default_rng(seed)
    if kind == "mel":
        x = rng.uniform(-1.0, 1.5, (B, C, T_in)).astype(np.float32)
    else:
        x = gelu64(2.0 * rng.standard_normal((B, C, T_in))).astype(np.float32)
    s = lin_scale(3 * C)
    w = rng.uniform(-s, s, (N, C, 3)).astype(np.float32)
    flat = w.reshape(-1)
    planted = rng.choice(flat.size, 64, replace=False)
    flat[planted] = (rng.uniform(2.0**-20, 2.0**-13.5, 64) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    zero_row = N // 3
    w[zero_row] = 0.0
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    bias[zero_row] = 0.625
    T_out = (T_in - 1) // stride + 1
    pos = rng.uniform(-0.1, 0.1, (2 * T_out, N)).astype(np.float32) if has_pos else None
    return dict(x=x, w=w, bias=bias, pos=pos, stride=stride, zero_row=zero_row, T_out=T_out, layout=layout)


def im2col(x, stride, right_edge_repeats=False):
    """[B, C, T] -> [B * T_out, 3C] with k = kk * C + c (layers.rs:92-121,
    padding 1).  right_edge_repeats: the mistake of reading x[T - 1] where
    the right pad's zero belongs."""
    B, C, T = x.shape
    t_out = (T - 1) // stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1)))
    if right_edge_repeats:
        xp[:, :, -1] = x[:, :, -1]
    cols = [xp[:, :, k: k + stride * (t_out - 1) + 1: stride] for k in range(3)]
    return np.concatenate(cols, axis=1).transpose(0, 2, 1).reshape(B * t_out, 3 * C)


def conv_weight_rows(w):
    """[N, C, 3] -> [N, 3C] in im2col order (layers.rs:118-121)."""
    N, C, K = w.shape
    return w.transpose(0, 2, 1).reshape(N, K * C)


def _flushed_lo(v, scale):
    """delta of the bound: 2^-11 |v| where |scale v| < 2^-3 (there the lo half
    of the f16 pair is an f16 subnormal, which the MFMA flushes), else 0."""
    av = np.abs(v)
    return np.where(av * scale < 2.0**-3, 2.0**-11 * av, 0.0)


def conv_ref(x, w, bias, pos, stride):
    """The oracle's conv1d restated in float64, then bias, GELU and the
    positional rows.  Returns (out, bound), [B * T_out, N] each:
        bz    = c sum|a||w| + sum da |w| + sum |a| dw + 1e-7
        bound = 1.13 (bz + 2^-23 |z|) + 1e-6 |gelu(z)| + 2^-23 |out|"""
    col = im2col(np.asarray(x, np.float64), stride)
    wf = conv_weight_rows(np.asarray(w, np.float64))
    z = col @ wf.T + np.asarray(bias, np.float64)
    acol, awf = np.abs(col), np.abs(wf)
    bz = (CONV_C * (acol @ awf.T) + _flushed_lo(col, CONV_A_SCALE) @ awf.T + acol @ _flushed_lo(wf, CONV_W_SCALE).T
          + 1e-7)
    g = gelu64(z)
    out = g
    if pos is not None:
        t_out = col.shape[0] // x.shape[0]
        out = g + np.tile(np.asarray(pos[:t_out], np.float64), (x.shape[0], 1))
    bound = GELU_SLOPE * (bz + 2.0**-23 * np.abs(z)) + 1e-6 * np.abs(g) + 2.0**-23 * np.abs(out)
    return out, bound


def split_f16_pair(v, scale):
    """The kernel's operand: hi = RNE_f16(scale v), lo = RNE_f16(scale v - hi)
    (wq4_device.hpp split_f16), f16 subnormals flushed as the MFMA flushes
    them.  Returned as float64 (hi, lo)."""
    s = (np.asarray(v, np.float32) * np.float32(scale)).astype(np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    hi[np.abs(hi) < 2.0**-14] = 0.0
    lo[np.abs(lo) < 2.0**-14] = 0.0
    return hi, lo


def conv_emulate(x, w, bias, pos, stride, drop=None, right_edge_repeats=False, pos_clip_offset=False):
    """The kernel's arithmetic on the CPU: both operands split by RNE into
    f16 pairs at the kernel's scales, subnormals flushed, hi hi + lo hi +
    hi lo (no lo lo) summed in float64, the scale undone, then bias, GELU and
    the positional rows in float64.  The switches are the mistakes the bound
    must reject: drop = "lo_a*hi_w" or "hi_a*lo_w" leaves that MFMA out;
    right_edge_repeats (im2col); pos_clip_offset takes the positional row at
    m instead of m % T_out (pos then holds the rows a second clip would hit)."""
    col = im2col(np.asarray(x, np.float32), stride, right_edge_repeats)
    ha, la = split_f16_pair(col, CONV_A_SCALE)
    hw, lw = split_f16_pair(conv_weight_rows(np.asarray(w, np.float32)), CONV_W_SCALE)
    acc = ha @ hw.T
    if drop != "lo_a*hi_w":
        acc += la @ hw.T
    if drop != "hi_a*lo_w":
        acc += ha @ lw.T
    out = gelu64(acc / (CONV_A_SCALE * CONV_W_SCALE) + np.asarray(bias, np.float64))
    if pos is not None:
        B, t_out = x.shape[0], col.shape[0] // x.shape[0]
        m = np.arange(B * t_out)
        rows = m % (2 * t_out) if pos_clip_offset else m % t_out
        out = out + np.asarray(pos, np.float64)[rows]
    return out


# ------------------------------------------------------------- LayerNorm --
LN_EPS = 1e-5
LN_FAMILIES = ("normal", "large_mean", "constant", "outliers", "tiny")
LN_WIDTHS = (96, 384, 1024, 1280, 2048)


def ln_rows(family, m, d, rng):
    n = rng.standard_normal((m, d))
    if family == "normal":
        x = 3.0 * n + 0.7
    elif family == "large_mean":
        x = 100.0 + 0.05 * n
    elif family == "constant":
        x = np.full((m, d), 3.25)
    elif family == "outliers":
        x = 3.0 * n + 0.7
        for r in range(m):
            x[r, rng.choice(d, 2, replace=False)] *= 300.0
    elif family == "tiny":
        x = 1e-4 * n
    else:
        raise ValueError(family)
    return x.astype(np.float32)


def ln_params(d, rng):
    return rng.uniform(0.5, 1.5, d).astype(np.float32), rng.uniform(-0.2, 0.2, d).astype(np.float32)


def ln_ref(x, g, b):
    """layers.rs:12-32 in float64 (two-pass, biased variance, eps inside the
    sqrt).  Returns (y, bound), the bound per element:
        |g| 2.4e-6 max|x| / s + 2e-6 (|y| + |b|) + 1e-7,  s = sqrt(var + eps)"""
    x, g, b = (np.asarray(v, np.float64) for v in (x, g, b))
    mean = x.mean(axis=1, keepdims=True)
    c = x - mean
    s = np.sqrt((c * c).mean(axis=1, keepdims=True) + LN_EPS)
    y = c / s * g + b
    bound = np.abs(g) * 2.4e-6 * np.abs(x).max(axis=1, keepdims=True) / s + 2e-6 * (np.abs(y) + np.abs(b)) + 1e-7
    return y, bound


def ln_f32(x, g, b, mutation=None):
    """The oracle's f32 layer_norm (whisper_oracle.py) restated, and the
    mistakes the bound must reject: "unbiased" (variance over D - 1),
    "no_eps", "eps_outside" (sqrt(var) + eps), "one_pass" (E[x^2] - mean^2)."""
    f = np.float32
    x, g, b = (np.asarray(v, f) for v in (x, g, b))
    d = x.shape[1]
    mean = x.mean(axis=1, keepdims=True, dtype=f)
    c = x - mean
    if mutation == "one_pass":
        var = (x * x).mean(axis=1, keepdims=True, dtype=f) - mean * mean
    elif mutation == "unbiased":
        var = (c * c).sum(axis=1, keepdims=True, dtype=f) / f(d - 1)
    else:
        var = (c * c).mean(axis=1, keepdims=True, dtype=f)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mutation == "no_eps":
            den = np.sqrt(var)
        elif mutation == "eps_outside":
            den = np.sqrt(var) + f(LN_EPS)
        else:
            den = np.sqrt(var + f(LN_EPS))
        return ((c / den) * g + b).astype(f)


def violations(got, want, bound):
    """Elements outside the bound (a NaN is outside) and the worst error /
    bound (inf if any element is not finite)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = ~(err <= bound)
    r = err / bound
    return bad, (float(np.max(r, initial=0.0)) if np.all(np.isfinite(r)) else float("inf"))


# ------------------------------------------------------------- embedding --
def embed_ref(tokens, te_rows, pe_rows):
    """x = tok_emb[token] + pos_emb[p]: one f32 add (decoder.rs:326-343).
    te_rows / pe_rows: the gathered rows, f32."""
    return (np.asarray(te_rows, np.float32) + np.asarray(pe_rows, np.float32)).astype(np.float32)


def tile_stats64(x):
    """(mean, sum of squared deviations) of each 16-column tile, float64: [rows, D / 16] each."""
    t = np.asarray(x, np.float64).reshape(x.shape[0], -1, 16)
    mean = t.mean(axis=2)
    return mean, ((t - mean[..., None]) ** 2).sum(axis=2)


def atile_halves(rows, d, ns):
    """Index (in f16 halves) of element (row, k, plane) of the A-tiled
    operand (wq4_lnmath.hpp atile_index): int64 [rows, d, ns]."""
    kbp = ((d // 32 + 1) // 2) * 2
    row = np.arange(rows, dtype=np.int64)[:, None, None]
    k = np.arange(d, dtype=np.int64)[None, :, None]
    s = np.arange(ns, dtype=np.int64)[None, None, :]
    mt, r = row >> 5, row & 31
    b, kk, hh, j = k >> 5, (k >> 4) & 1, (k >> 3) & 1, k & 7
    return (((((mt * kbp + b) * 2 + kk) * ns + s) * 64 + (r + 32 * hh)) * 8 + j)
