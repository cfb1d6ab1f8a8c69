"""The attention bounds' teeth, on the CPU (attn_ref.py): the faithful numpy
emulation of each kernel stays at or under half its bound on every planted
family, every listed mistake leaves the bound on a named family, and at the
older tests' shapes and inputs the bound is no looser than the tolerance
those tests state.  Shapes are cut down for the CPU; test_attn_gpu.py holds
the kernels themselves to the same bounds at the kernels' own shapes.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import attn_ref as A
import oracle
import whisper_amd
import wq4

NS = {"f16x2": 2, "f16": 1}


def ratios(got, ref, bound):
    """worst error / bound per (row, head): [R, H]; inf where not finite."""
    r = np.abs(np.asarray(got, np.float64) - ref) / bound
    r = np.where(np.isfinite(r), r, np.inf)
    return r.reshape(r.shape[0], -1, 64).max(axis=2)


def by_family(r, names):
    out = {}
    for row in range(r.shape[0]):
        for h in range(r.shape[1]):
            out[names(row, h)] = max(out.get(names(row, h), 0.0), float(r[row, h]))
    return out


def outside(r, names):
    return {f for f, v in by_family(r, names).items() if not v <= 1.0}


def plan(T, rows, free_cus):
    return whisper_amd.xattn_plan_splits(T, rows, free_cus)


# ------------------------------------------------------------- the cases --
@functools.lru_cache(maxsize=None)
def weights(H, wtype=0):
    return A.xattn_weights(H, wtype, 3 + H, wq4.quantize_q4_0, oracle.dequantize_np)


@functools.lru_cache(maxsize=None)
def xattn_inputs(H, T, Tq, S, scale="unit", prec="f16x2", wtype=0, shift=0):
    w = weights(H, wtype)
    sp = A.xattn_splits(T, S, plan)
    q, enc, names = A.xattn_case(1, Tq, T, H, w, 4, sp[1][0] if len(sp) > 1 else A.XATTN_TC, shift, scale)
    ref, bound = A.xattn_ref(q, w["wk"], w["wv"], w["bv"], enc, Tq, H, prec)
    return w, sp, q, enc, names, ref, bound


def xattn_run(H, T, Tq, S, scale="unit", prec="f16x2", wtype=0, shift=0, **mistakes):
    w, sp, q, enc, names, ref, bound = xattn_inputs(H, T, Tq, S, scale, prec, wtype, shift)
    got = A.xattn_emulate(q, w["wk"], w["wv"], w["bv"], enc, Tq, H, sp, NS[prec], **mistakes)
    return ratios(got, ref, bound), (lambda row, h: names[row][h])


@functools.lru_cache(maxsize=None)
def encoder_inputs(T, H, prec="f16x2"):
    qkv, names = A.encoder_case(1, T, H, 1)
    ref, bound = A.encoder_ref(qkv, 1, T, H, prec)
    return qkv.reshape(T, 3, H, 64), names, ref, bound


def encoder_run(T, H, prec="f16x2", **mistakes):
    x, names, ref, bound = encoder_inputs(T, H, prec)
    got = np.concatenate([A.encoder_emulate(x[:, 0, h], x[:, 1, h], x[:, 2, h], NS[prec], **mistakes) for h in range(H)], axis=1)
    return ratios(got, ref, bound), (lambda row, h: names[0][h][1][row // A.ENC_BLOCK])


@functools.lru_cache(maxsize=None)
def kv_inputs(Tq, T, H, prec="f16x2"):
    q, k, v, names = A.kv_case(1, Tq, T, H, 2)
    ref, bound = A.f32_ref(q, k, v, Tq, prec)
    return q.reshape(Tq, H, 64), k[0], v[0], names, ref, bound


def kv_run(Tq, T, H, prec="f16x2", **mistakes):
    q, k, v, names, ref, bound = kv_inputs(Tq, T, H, prec)
    got = np.concatenate([A.f32_emulate(q[:, h], k[h], v[h], A.xkv_ranges(T), None, NS[prec], **mistakes) for h in range(H)], axis=1)
    return ratios(got, ref, bound), (lambda row, h: names[0][h][1][row])


@functools.lru_cache(maxsize=None)
def self_inputs(Tq, kv, H, prec="f16x2"):
    qkv, ck, cv, k, v, names = A.self_case(1, Tq, kv, H, 5)
    q = qkv.reshape(Tq, 3, H, 64)[:, 0]
    ref, bound = A.f32_ref(q.reshape(Tq, H * 64), k, v, Tq, prec, kv)
    return q, k[0], v[0], names, ref, bound


def self_run(Tq, kv, H, prec="f16x2", off=0, **mistakes):
    q, k, v, names, ref, bound = self_inputs(Tq, kv, H, prec)
    vis = A.causal_vis(Tq, kv, off)
    got = np.concatenate([A.f32_emulate(q[:, h], k[h], v[h], [(0, kv + Tq)], vis, NS[prec], **mistakes) for h in range(H)], axis=1)
    return ratios(got, ref, bound), (lambda row, h: names[0][h][1][row])


# (label, runner, arguments): every family appears in each kernel's set
FAITHFUL = [
    ("xattn H20 T53 S3", xattn_run, (20, 53, 2, 3)),
    ("xattn H20 T53 S1", xattn_run, (20, 53, 2, 1)),
    ("xattn H6 T37 Tq3", xattn_run, (6, 37, 3, 8)),
    ("xattn H6 T1", xattn_run, (6, 1, 3, 8)),
    ("xattn H6 T53 f16 weights", xattn_run, (6, 53, 3, 3, "unit", "f16x2", 1)),
    ("xattn H6 T53 tiny", xattn_run, (6, 53, 3, 3, "tiny")),
    ("xattn H6 T53 large", xattn_run, (6, 53, 3, 3, "large")),
    ("xattn H20 T53 f16", xattn_run, (20, 53, 2, 3, "unit", "f16")),
    ("encoder T70 H3", encoder_run, (70, 3)),
    ("encoder T33 H5", encoder_run, (33, 5)),
    ("encoder T70 H3 f16", encoder_run, (70, 3, "f16")),
    ("kv T203 Tq3 H5", kv_run, (3, 203, 5)),
    ("kv T401 Tq1 H15", kv_run, (1, 401, 15)),
    ("kv T203 Tq3 H5 f16", kv_run, (3, 203, 5, "f16")),
    ("self kv70 H15", self_run, (1, 70, 15)),
    ("self prompt Tq4 kv9 H4", self_run, (4, 9, 4)),
    ("self kv70 H15 f16", self_run, (1, 70, 15, "f16")),
]


@pytest.mark.parametrize("label,run,args", FAITHFUL, ids=[c[0] for c in FAITHFUL])
def test_emulation_within_half_the_bound(label, run, args):
    r, names = run(*args)
    fam = by_family(r, names)
    print(f"{label}: worst error / bound {r.max():.3f}  " + " ".join(f"{k}={v:.2f}" for k, v in sorted(fam.items())))
    assert r.max() <= 0.5, fam


def test_every_family_is_planted_in_every_kernel():
    for run, args in ((xattn_run, (20, 53, 2, 3)), (encoder_run, (70, 3)), (kv_run, (3, 203, 5)), (self_run, (1, 70, 15))):
        r, names = run(*args)
        assert set(by_family(r, names)) == set(A.FAMILIES), (run.__name__, args)


def test_planted_scores_are_reproduced():
    """The planting itself: the f32 inputs give the families' scores to 1e-5
    (float64 gives 3e-7 at H = 20, T = 203, two rows; the rest is the f32 rounding of enc)."""
    w, sp, q, enc, names, _, _ = xattn_inputs(20, 53, 2, 3)
    rng_free = {"wide", "gauss"}
    K = enc[0].astype(np.float64) @ w["wk"].astype(np.float64).T
    worst = 0.0
    for row in range(2):
        for h in range(20):
            if names[row][h] in rng_free:
                continue
            s = K[:, h * 64:(h + 1) * 64] @ q[row, h * 64:(h + 1) * 64].astype(np.float64) / 8.0
            want = A.family_scores(names[row][h], 53, A.XATTN_TC, sp[1][0], None)
            worst = max(worst, np.abs(s - want).max())
    print(f"planted scores: worst deviation {worst:.2e}, max |enc| {np.abs(enc).max():.2f}")
    assert worst <= 1e-5


# ---------------------------------------------------------- the mistakes --
# (mistake, runner, arguments, switches, the family that must leave the bound)
MISTAKES = [
    ("Z never rescaled (WA_XATTN_DIAG 5)", xattn_run, (20, 53, 2, 1), dict(no_rescale=True), "ramp_up"),
    ("o never rescaled, encoder", encoder_run, (70, 3), dict(no_rescale=True), "ramp_up"),
    ("o never rescaled, K/V form", kv_run, (3, 203, 5), dict(no_rescale=True), "ramp_up"),
    ("a frame past T counted as valid", xattn_run, (20, 53, 2, 3), dict(extra_frame=True), "flat"),
    ("a key past T counted as valid, encoder", encoder_run, (70, 3), dict(extra_frame=True), "flat"),
    ("the last valid key dropped", xattn_run, (20, 53, 2, 3), dict(t_valid=52), "spike_last"),
    ("the last valid key dropped, encoder", encoder_run, (70, 3), dict(t_valid=69), "spike_last"),
    ("the last valid key dropped, K/V form", kv_run, (3, 203, 5), dict(t_valid=202), "spike_last"),
    ("the appended key dropped, self-attention", self_run, (1, 70, 15), dict(t_valid=70), "spike_last"),
    ("splits merged with equal weights", xattn_run, (20, 53, 2, 3), dict(merge="equal"), "ramp_up"),
    ("splits merged with equal weights, K/V form", kv_run, (3, 203, 5), dict(merge="equal"), "ramp_up"),
    ("one split's partial dropped", xattn_run, (20, 53, 2, 3), dict(drop_split=1), "tied_spikes"),
    ("one split's partial dropped, K/V form", kv_run, (3, 203, 5), dict(drop_split=1), "tied_spikes"),
    ("the lo hi term of the score product dropped", xattn_run, (20, 53, 2, 3), dict(drop_lo_hi=True), "wide"),
    ("the lo hi term of the score product dropped, encoder", encoder_run, (70, 3), dict(drop_lo_hi=True), "wide"),
    ("P kept as a single f16", xattn_run, (20, 53, 2, 3), dict(p_single=True), "gauss"),
    ("P kept as a single f16, encoder", encoder_run, (70, 3), dict(p_single=True), "gauss"),
    ("a P scale of 2^15", xattn_run, (20, 53, 2, 1), dict(p_scale=32768.0), "brink"),
    ("a P scale of 2^15, encoder", encoder_run, (70, 3), dict(p_scale=32768.0), "brink"),
    ("a causal mask off by one in the prompt", self_run, (4, 9, 4), dict(off=1), "gauss"),
    ("the second head tile reading head 0..3's qt", xattn_run, (20, 53, 2, 3), dict(head_tile_mixup=True), "brink"),
    ("the value bias added once per key", xattn_run, (20, 53, 2, 3), dict(bias_per_key=True), "gauss"),
]


@pytest.mark.parametrize("label,run,args,switches,family", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_mistake_leaves_the_bound(label, run, args, switches, family):
    r, names = run(*args, **switches)
    out = outside(r, names)
    print(f"{label}: outside the bound on {sorted(out)}; worst error / bound {r.max():.3g}")
    assert family in out, (family, by_family(r, names))


def test_p_scale_2_15_overflows_on_brink_only():
    """p * 2^15 reaches the f16 infinity only for p >= 1.99951: `brink` (0.9998
    in base 2) gives a non-finite output; `creep` (0.98, p = 1.97, p * 2^15 =
    64634) stays finite -- the P scale 2^14 holds p <= 2 with a factor 2 to spare."""
    r, names = xattn_run(20, 53, 2, 1, p_scale=32768.0)
    fam = by_family(r, names)
    assert fam["brink"] == np.inf and np.isfinite(fam["creep"]), fam


def test_mfma_flush_would_leave_the_bound(monkeypatch):
    """An MFMA that read f16 subnormal operands as 0 (the documented model,
    attn_ref.MFMA_FLUSHES) loses a lo half under 2^-14 at any magnitude of x,
    an absolute 2^-19 at the x 2^5 operands: a spike, whose output is one
    value row, then leaves the bound.  The MI355X keeps them."""
    monkeypatch.setattr(A, "MFMA_FLUSHES", True)
    r, names = encoder_run(33, 5)
    out = outside(r, names)
    print(f"flushing MFMA: outside the bound on {sorted(out)}; worst error / bound {r.max():.3g}")
    assert any(f.startswith("spike_") for f in out), by_family(r, names)


def test_head_tile_mixup_is_confined_to_heads_16_up():
    r, _ = xattn_run(20, 53, 2, 3, head_tile_mixup=True)
    assert r[:, :16].max() <= 0.5 and (r[:, 16:] > 1.0).all(), r.round(2)


def test_c_is_the_smallest_admissible(monkeypatch):
    """C_REL is the smallest of {1, 2, 5} x 10^-k with every faithful case at
    or under half its bound: one step down (2e-7) a case is over."""
    caches = (xattn_inputs, encoder_inputs, kv_inputs, self_inputs)
    monkeypatch.setattr(A, "C_REL", 2e-7)
    for f in caches:
        f.cache_clear()
    try:
        worst = {label: float(run(*args)[0].max()) for label, run, args in FAITHFUL}
    finally:
        for f in caches:
            f.cache_clear()
    print(" ".join(f"{k}: {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) > 0.5, worst


# ------------------------------------------------------------- tightness --
def _sdpa_bound_max(q, k, v, prec, pair, vis=None):
    return A.sdpa_ref(q, k, v, prec, pair, vis)[1].max()


def test_bound_no_looser_than_the_older_tolerances():
    """At the older tests' shapes and inputs (test_kernels_gpu.py,
    test_xattn_gpu.py: same generators and seeds; one head or clip of each,
    every element of it) the bound's maximum is within the tolerance those
    tests state: 4e-6 max|v| (encoder), 2e-6 max|v| (decoder self-attention,
    the K / V form), 2e-5 max|ref| and, at WQ4_PREC_F16, 5e-3 max|ref|
    (cross-attention)."""
    # encoder attention, H = 20, B = 1, T = 1500: head 0, a third of the queries
    H, B, T = 20, 1, 1500
    D = 64 * H
    qkv = np.random.default_rng(H * 7 + B).standard_normal((B * T, 3 * D)).astype(np.float32)
    qkv[:, :D] *= 2.0
    q, k, v = qkv[::3, :64], qkv[:, D:D + 64], qkv[:, 2 * D:2 * D + 64]
    b = _sdpa_bound_max(q, k, v, "f16x2", True)
    print(f"encoder: bound {b / np.abs(v).max():.2e} max|v| (4e-6)")
    ok = [b <= 4e-6 * np.abs(v).max()]
    # decoder self-attention, H = 20, kv = 227: clip 0, head 0
    rng = np.random.default_rng(20)
    ck = rng.standard_normal((3, 20, 448, 64)).astype(np.float32)
    cv = rng.standard_normal((3, 20, 448, 64)).astype(np.float32)
    q = (3.0 * rng.standard_normal((1, 64))).astype(np.float32)
    b = _sdpa_bound_max(q, ck[0, 0, :228], cv[0, 0, :228], "f16x2", False)
    vmax = np.abs(cv[0, 0, :228]).max()
    print(f"decoder self-attention: bound {b / vmax:.2e} max|v| (2e-6)")
    ok.append(b <= 2e-6 * vmax)
    # the K / V form, (B, Tq, T, H) = (1, 1, 1500, 20): head 0
    rng = np.random.default_rng(1 * 100 + 1 * 10 + 20)
    q = (2.0 * rng.standard_normal((1, 1280))).astype(np.float32)
    k = rng.standard_normal((1, 20, 1500, 64)).astype(np.float32)
    v = rng.standard_normal((1, 20, 1500, 64)).astype(np.float32)
    b = _sdpa_bound_max(q[:, :64], k[0, 0], v[0, 0], "f16x2", False)
    print(f"K/V form: bound {b / np.abs(v).max():.2e} max|v| (2e-6)")
    ok.append(b <= 2e-6 * np.abs(v).max())
    # cross-attention, run_case(1, 1, 1500, 20) of test_xattn_gpu.py at both precisions
    for prec, tol, seed in (("f16x2", 2e-5, 0), ("f16", 5e-3, 5)):
        H, T = 20, 1500
        D = 64 * H
        rng = np.random.default_rng(seed)
        enc = rng.standard_normal((1, T, D)).astype(np.float32)
        q = (2.0 * rng.standard_normal((1, D))).astype(np.float32)
        wk = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
        wv = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
        bv = rng.uniform(-0.02, 0.02, D).astype(np.float32)
        wk = oracle.dequantize_np(wq4.quantize_q4_0(wk), D * D).reshape(D, D)
        wv = oracle.dequantize_np(wq4.quantize_q4_0(wv), D * D).reshape(D, D)
        ref, bound = A.xattn_ref(q, wk, wv, bv, enc, 1, H, prec)
        print(f"cross-attention {prec}: bound {bound.max() / np.abs(ref).max():.2e} max|ref| ({tol:g})")
        assert bound.shape == ref.shape and np.all(bound > 0) and np.all(np.isfinite(bound))
        ok.append(bound.max() <= tol * np.abs(ref).max())
    assert all(ok), ok


def test_every_element_is_compared():
    """violations() judges every output element: a single element off by
    twice its bound, anywhere, is found, and a NaN is outside."""
    _, _, _, _, _, ref, bound = xattn_inputs(6, 37, 3, 8)
    assert bound.shape == ref.shape and np.all(bound > 0)
    rng = np.random.default_rng(0)
    for _ in range(20):
        got = ref.copy()
        i, j = rng.integers(ref.shape[0]), rng.integers(ref.shape[1])
        got[i, j] += 2.0 * bound[i, j]
        bad, worst = A.violations(got, ref, bound)
        assert bad.sum() == 1 and bad[i, j] and 1.9 < worst < 2.1
    got = ref.copy()
    got[-1, -1] = np.nan
    bad, worst = A.violations(got, ref, bound)
    assert bad[-1, -1] and worst == np.inf
