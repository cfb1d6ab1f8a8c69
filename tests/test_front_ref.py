"""The teeth of front_ref.py's bounds, shown without a kernel (no GPU).

Conv: a CPU emulation of conv_gelu_f16_kernel's arithmetic (f16 pairs at the
kernel's scales, subnormals flushed, hi hi + lo hi + hi lo) stays within
half the bound at every shape of test_front_gpu.py (C, N and K intact, T cut
to at most 64), and the same emulation with one mistake planted -- a dropped
cross term, a right-edge tap that reads x[T_in - 1], a positional row from
the wrong clip offset -- leaves it.  LayerNorm: the oracle's f32 layer_norm
stays within half the bound on every row family and width; unbiased variance,
a missing eps, eps outside the sqrt and the one-pass variance leave it on
the family meant to catch each.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import front_ref as fr

CASES = list(range(len(fr.CONV_CASES)))


@functools.lru_cache(maxsize=None)
def _conv(i):
    d = fr.conv_inputs(fr.CONV_CASES[i], seed=100 + i, t_cap=64)
    want, bound = fr.conv_ref(d["x"], d["w"], d["bias"], d["pos"], d["stride"])
    for a in (want, bound):
        a.setflags(write=False)
    return d, want, bound


def _emulate(d, **kw):
    return fr.conv_emulate(d["x"], d["w"], d["bias"], d["pos"], d["stride"], **kw)


@pytest.mark.parametrize("i", CASES)
def test_conv_emulation_within_half_the_bound(i):
    d, want, bound = _conv(i)
    bad, ratio = fr.violations(_emulate(d), want, bound)
    print(f"conv case {i + 1}: emulation worst err / bound = {ratio:.3f}")
    assert not bad.any() and ratio <= 0.5, ratio


@pytest.mark.parametrize("drop", ["lo_a*hi_w", "hi_a*lo_w"])
@pytest.mark.parametrize("i", CASES)
def test_conv_bound_rejects_a_dropped_cross_term(i, drop):
    d, want, bound = _conv(i)
    bad, _ = fr.violations(_emulate(d, drop=drop), want, bound)
    # the zeroed weight row has no product to lose
    live = np.ones(bad.shape[1], bool)
    live[d["zero_row"]] = False
    frac = float(bad[:, live].mean())
    print(f"conv case {i + 1} without {drop}: {frac:.3f} of the outputs outside the bound")
    assert frac > 0.5, frac


@pytest.mark.parametrize("i", [i for i in CASES if fr.CONV_CASES[i][4] == 1])
def test_conv_bound_rejects_a_repeated_right_edge(i):
    """Only the last frame of each clip reads the right pad at stride 1."""
    d, want, bound = _conv(i)
    bad, _ = fr.violations(_emulate(d, right_edge_repeats=True), want, bound)
    B, t_out = d["x"].shape[0], d["T_out"]
    last = bad.reshape(B, t_out, -1)[:, -1]
    live = np.ones(last.shape[1], bool)
    live[d["zero_row"]] = False
    assert float(last[:, live].mean()) > 0.5
    assert not bad.reshape(B, t_out, -1)[:, :-1].any()


@pytest.mark.parametrize("i", [i for i in CASES if fr.CONV_CASES[i][4] == 2 and fr.CONV_CASES[i][2] % 2 == 1])
def test_conv_bound_rejects_a_repeated_right_edge_at_stride_2(i):
    """An odd T_in makes the last tap of the last frame read the right pad at stride 2 too."""
    d, want, bound = _conv(i)
    bad, _ = fr.violations(_emulate(d, right_edge_repeats=True), want, bound)
    last = bad.reshape(d["x"].shape[0], d["T_out"], -1)[:, -1]
    assert float(last.mean()) > 0.5


@pytest.mark.parametrize("i", [i for i in CASES if fr.CONV_CASES[i][6]])
def test_conv_bound_rejects_a_positional_row_of_the_wrong_clip(i):
    d, want, bound = _conv(i)
    bad, _ = fr.violations(_emulate(d, pos_clip_offset=True), want, bound)
    per_clip = bad.reshape(d["x"].shape[0], d["T_out"], -1)
    assert not per_clip[0].any()  # the first clip's rows are m % T_out either way
    assert float(per_clip[1].mean()) > 0.5


def test_conv_reference_is_the_oracles_conv1d():
    """conv_ref's pre-activation against the oracle's f32 conv1d (whisper_oracle.py) on a small case."""
    import whisper_oracle

    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 8, 11)).astype(np.float32)
    w = rng.standard_normal((5, 8, 3)).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    for stride in (1, 2):
        o = whisper_oracle.SynthWhisper.__new__(whisper_oracle.SynthWhisper)
        o.dt = np.float32
        o.w = {"c.weight": w, "c.bias": b}
        z32 = o.conv1d(x, "c", stride).transpose(0, 2, 1).reshape(-1, 5)
        z64 = fr.im2col(x.astype(np.float64), stride) @ fr.conv_weight_rows(w.astype(np.float64)).T + b
        assert np.allclose(z32, z64, rtol=0, atol=1e-4)


# ------------------------------------ the check entries' host validation --
def test_check_entries_reject_bad_arguments_on_the_host():
    """wa_conv_gelu_check and wa_embed_check return WQ4_EINVAL before they
    touch a device, so the refusals need none (the pointers are host scratch
    that a refused call never reads as device memory)."""
    import ctypes

    import whisper_amd

    L = whisper_amd.lib()
    buf = np.zeros(64, np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)

    def conv(bs, cs, ts, B, C, T, stride, N):
        return L.wa_conv_gelu_check(0, p, bs, cs, ts, B, C, T, stride, p, p, None, N, p)

    assert conv(6 * 16, 16, 1, 2, 6, 16, 1, 8) == 1  # C % 4
    for B, C, T, N in [(0, 8, 16, 8), (2, 0, 16, 8), (2, 8, 0, 8), (2, 8, 16, 0), (-1, 8, 16, 8), (2, 8, -16, 8)]:
        assert conv(C * T, T, 1, B, C, T, 1, N) == 1
    assert conv(8 * 16, 16, 1, 2, 8, 16, 3, 8) == 1  # stride
    assert conv(10 * 16, 1, 10, 2, 8, 16, 1, 8) == 1  # channel-contiguous, time stride 10
    assert conv(8 * 16 + 2, 1, 8, 2, 8, 16, 1, 8) == 1  # channel-contiguous, clip stride % 4
    assert b"multiples of 4" in L.wa_last_error()

    def embed(tokens, B, Tq, pos0, V=64, ctx=16, D=384, fold=False):
        tok = np.asarray(tokens, np.int32)
        f = p if fold else None
        return L.wa_embed_check(0, tok.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p, V, p, ctx, B, Tq, D, pos0, 0,
                                None, f, 0, p, f, f)

    for fold in (False, True):
        assert embed([0, 64, 1, 2], 2, 2, 0, fold=fold) == 1  # token == V
        assert embed([0, 1, -1, 2], 2, 2, 0, fold=fold) == 1
        assert embed([0, 1, 2, 3], 2, 2, 15, fold=fold) == 1  # pos0 + Tq == ctx + 1
        assert embed([0, 1, 2, 3], 2, 2, -1, fold=fold) == 1
        assert embed([0, 1, 2, 3], 0, 2, 0, fold=fold) == 1
        assert embed([0, 1, 2, 3], 2, 0, 0, fold=fold) == 1
    assert embed([0, 1, 2, 3], 2, 2, 0, D=48, fold=True) == 1  # the folded form needs D % 32 == 0


# ------------------------------------------------------------- LayerNorm --
@functools.lru_cache(maxsize=None)
def _ln(family, d):
    rng = np.random.default_rng(d * 7 + fr.LN_FAMILIES.index(family))
    x = fr.ln_rows(family, 67, d, rng)
    g, b = fr.ln_params(d, rng)
    want, bound = fr.ln_ref(x, g, b)
    return x, g, b, want, bound


@pytest.mark.parametrize("d", fr.LN_WIDTHS)
@pytest.mark.parametrize("family", fr.LN_FAMILIES)
def test_layernorm_f32_oracle_within_half_the_bound(family, d):
    x, g, b, want, bound = _ln(family, d)
    bad, ratio = fr.violations(fr.ln_f32(x, g, b), want, bound)
    print(f"LayerNorm {family} D={d}: f32 oracle worst err / bound = {ratio:.3f}")
    assert not bad.any() and ratio <= 0.5, ratio


@pytest.mark.parametrize("d", fr.LN_WIDTHS)
@pytest.mark.parametrize("mutation,family", [("unbiased", "normal"), ("no_eps", "tiny"), ("no_eps", "constant"),
                                             ("eps_outside", "tiny"), ("one_pass", "large_mean")])
def test_layernorm_bound_rejects(mutation, family, d):
    x, g, b, want, bound = _ln(family, d)
    bad, ratio = fr.violations(fr.ln_f32(x, g, b, mutation), want, bound)
    frac = float(bad.mean())
    print(f"LayerNorm {mutation} on {family} D={d}: {frac:.3f} of the elements outside the bound")
    assert frac > 0.5, (frac, ratio)


def test_layernorm_constant_row_gives_the_bias():
    """A constant 3.25 row: every partial sum and the mean are exact in f32, so y == b bit for bit."""
    for d in fr.LN_WIDTHS:
        x, g, b, want, _ = _ln("constant", d)
        assert np.array_equal(fr.ln_f32(x, g, b), b[None, :].repeat(x.shape[0], 0))
        assert np.array_equal(want, b.astype(np.float64)[None, :].repeat(x.shape[0], 0))
