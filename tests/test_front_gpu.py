"""Float64 parity of the kernels at the model's two ends (run on an MI355X):
conv_gelu_f16_kernel (the conv stem), wq4_layernorm's f32 rows, and
embed_kernel / embed_fold_kernel -- each through its product launcher
(wa_conv_gelu_check, wq4_layernorm, wa_embed_check), held to the bounds of
front_ref.py, which test_front_ref.py shows to reject a dropped MFMA term, a
wrong edge tap, a wrong positional row and the usual LayerNorm mistakes.
Each test prints its worst error / bound ratio (DESIGN.md "Numerics").
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import front_ref as fr
import oracle
import whisper_amd
import wq4

pytestmark = pytest.mark.gpu

EINVAL = 1


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available(), "GPU tests need an MI355X"
    return _t


@pytest.fixture(autouse=True)
def _reset_modes():
    wq4.set_precision(wq4.PREC_F16X2)
    wq4.set_kernel_policy(0)
    yield
    wq4.set_precision(wq4.PREC_F16X2)
    wq4.set_kernel_policy(0)


def dev(torch, a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # a copy: the shared references are read-only


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ conv --
CONV_IDS = [f"case{i + 1}" for i in range(len(fr.CONV_CASES))]


@functools.lru_cache(maxsize=None)
def _conv_case(i):
    """Inputs and the float64 reference of conv case i, computed once."""
    d = fr.conv_inputs(fr.CONV_CASES[i], seed=200 + i)
    pos = None if d["pos"] is None else d["pos"][: d["T_out"]]
    want, bound = fr.conv_ref(d["x"], d["w"], d["bias"], pos, d["stride"])
    for a in (want, bound, d["x"], d["w"], d["bias"]):
        a.setflags(write=False)
    return d, pos, want, bound


def _conv_device_inputs(torch, d, pos):
    """x as the model lays it out: channel-major [B, C, T] (the mel), or
    time-major [B, T, C] viewed as [B, C, T] (conv1's output, in_cs = 1)."""
    if d["layout"] == "time":
        x = dev(torch, d["x"].transpose(0, 2, 1)).permute(0, 2, 1)
        assert x.stride(1) == 1
    else:
        x = dev(torch, d["x"])
        assert x.stride(2) == 1
    return x, dev(torch, d["w"]), dev(torch, d["bias"]), None if pos is None else dev(torch, pos)


@pytest.mark.parametrize("i", range(len(fr.CONV_CASES)), ids=CONV_IDS)
def test_conv_gelu_vs_float64(torch, i):
    """Every output of the conv stem's kernel against float64 under
    front_ref.conv_ref's bound; every element written (poisoned output); the
    zeroed weight row gives gelu(bias) (+ pos) to the GELU's own rounding and,
    without pos, the same bits in every frame; clip b alone gives the bits it
    has inside the batch."""
    d, pos, want, bound = _conv_case(i)
    x, w, bias, posd = _conv_device_inputs(torch, d, pos)
    B, T_out, N = d["x"].shape[0], d["T_out"], d["w"].shape[0]
    out = torch.full((B, T_out, N), float("nan"), device="cuda:0")
    whisper_amd.conv_gelu_check(x, w, bias, d["stride"], posd, out=out)
    got = out.cpu().numpy().reshape(B * T_out, N)
    assert np.all(np.isfinite(got)), "an output element was not written"
    bad, ratio = fr.violations(got, want, bound)
    print(f"FRONT_RATIO conv {CONV_IDS[i]} {ratio:.3f}")
    assert not bad.any(), (ratio, np.argwhere(bad)[:4].tolist())
    # the zeroed weight row: z == bias exactly, so only the GELU and the positional add round
    n0 = d["zero_row"]
    g0 = float(fr.gelu64(d["bias"][n0]))
    col = got[:, n0].astype(np.float64)
    assert np.all(np.abs(col - want[:, n0]) <= 1e-6 * abs(g0) + 2.0**-23 * np.abs(want[:, n0]))
    if pos is None:
        assert np.all(got[:, n0].view(np.uint32) == got[0, n0].view(np.uint32))
    # batch invariance, bit for bit
    for b in sorted({0, B - 1}):
        if B == 1:
            break
        one = whisper_amd.conv_gelu_check(x[b: b + 1], w, bias, d["stride"], posd).cpu().numpy().reshape(T_out, N)
        assert np.array_equal(one.view(np.uint32), got[b * T_out: (b + 1) * T_out].view(np.uint32)), b


def test_conv_gelu_rejects_bad_arguments(torch):
    """C % 4 != 0, non-positive sizes and a channel-contiguous layout whose
    time stride is not a multiple of 4 are refused with WQ4_EINVAL before
    anything is launched: the poisoned output stays as it was."""
    L = whisper_amd.lib()
    x = torch.zeros(4096, device="cuda:0")
    w = torch.zeros(4096, device="cuda:0")
    b = torch.zeros(64, device="cuda:0")
    out = torch.full((4096,), 7.5, device="cuda:0")

    def call(bs, cs, ts, B, C, T, stride, N, xx=x, ww=w, bb=b, oo=out):
        return L.wa_conv_gelu_check(0, _p(xx), bs, cs, ts, B, C, T, stride, _p(ww), _p(bb), None, N, _p(oo))

    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 8) == 0  # the accepted shape the others depart from
    torch.cuda.synchronize()
    assert not bool((out[: 2 * 16 * 8] == 7.5).any())
    out.fill_(7.5)
    assert call(6 * 16, 16, 1, 2, 6, 16, 1, 8) == EINVAL  # C % 4
    assert call(8 * 16, 16, 1, 0, 8, 16, 1, 8) == EINVAL  # B
    assert call(8 * 16, 16, 1, 2, 0, 16, 1, 8) == EINVAL  # C
    assert call(8 * 16, 16, 1, 2, 8, 0, 1, 8) == EINVAL  # T_in
    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 0) == EINVAL  # N
    assert call(8 * 16, 16, 1, 2, -8, 16, 1, 8) == EINVAL
    assert call(8 * 16, 16, 1, 2, 8, 16, 0, 8) == EINVAL  # stride
    assert call(8 * 16, 16, 1, 2, 8, 16, 3, 8) == EINVAL
    assert call(10 * 16, 1, 10, 2, 8, 16, 1, 8) == EINVAL  # channel-contiguous, time stride 10
    assert call(8 * 16 + 2, 1, 8, 2, 8, 16, 1, 8) == EINVAL  # channel-contiguous, clip stride % 4
    assert call(8 * 16, 1, 8, 2, 8, 16, 1, 8) == 0  # channel-contiguous, time stride 8: accepted
    out.fill_(7.5)
    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 8, xx=None) == EINVAL
    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 8, ww=None) == EINVAL
    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 8, bb=None) == EINVAL
    assert call(8 * 16, 16, 1, 2, 8, 16, 1, 8, oo=None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())


# ------------------------------------------------------------- LayerNorm --
def _layernorm_rows(torch, x, g, b):
    m, d = x.shape
    y = torch.full((m, d), float("nan"), device="cuda:0")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wq4.check(wq4.lib().wq4_layernorm(_p(x), _p(g), _p(b), m, d, wq4.PREC_F16X2, None, _p(y), st))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("m", [1, 5, 67])
@pytest.mark.parametrize("d", fr.LN_WIDTHS)
def test_layernorm_rows_vs_float64(torch, d, m):
    """wq4_layernorm's f32 rows against float64 (two-pass, biased variance,
    eps inside the sqrt) under front_ref.ln_ref's bound, on every row family;
    a constant row gives the bias bit for bit."""
    worst = 0.0
    for fi, family in enumerate(fr.LN_FAMILIES):
        rng = np.random.default_rng(d * 31 + m * 5 + fi)
        x = fr.ln_rows(family, m, d, rng)
        g, b = fr.ln_params(d, rng)
        want, bound = fr.ln_ref(x, g, b)
        got = _layernorm_rows(torch, dev(torch, x), dev(torch, g), dev(torch, b)).cpu().numpy()
        bad, ratio = fr.violations(got, want, bound)
        assert not bad.any(), (family, ratio, np.argwhere(bad)[:4].tolist())
        if family == "constant":
            assert np.array_equal(got.view(np.uint32), np.broadcast_to(b, (m, d)).view(np.uint32))
        worst = max(worst, ratio)
    print(f"FRONT_RATIO layernorm D={d} M={m} {worst:.3f}")


@pytest.mark.parametrize("prec", [0, 1])
def test_layernorm_m_tile_kernel_vs_float64(torch, prec):
    """D = 1280, M = 2100 (> 2048 rows: layernorm_tiled_kernel; M % 32 != 0):
    the f32 rows pass the float64 bound, and the A-tiled form equals those
    rows tiled by wq4_tile_activations bit for bit, families interleaved."""
    m, d = 2100, 1280
    rng = np.random.default_rng(2100 + prec)
    x = np.empty((m, d), np.float32)
    for fi, family in enumerate(fr.LN_FAMILIES):
        rows = np.arange(fi, m, len(fr.LN_FAMILIES))
        x[rows] = fr.ln_rows(family, rows.size, d, rng)
    g, b = fr.ln_params(d, rng)
    want, bound = fr.ln_ref(x, g, b)
    xd, gd, bd = dev(torch, x), dev(torch, g), dev(torch, b)
    y = _layernorm_rows(torch, xd, gd, bd)
    bad, ratio = fr.violations(y.cpu().numpy(), want, bound)
    print(f"FRONT_RATIO layernorm D={d} M={m} prec={prec} {ratio:.3f}")
    assert not bad.any(), (ratio, np.argwhere(bad)[:4].tolist())
    L = wq4.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    atb = L.wq4_atiled_bytes(m, d, prec)
    got = torch.full((atb,), 0x5A, dtype=torch.uint8, device="cuda:0")  # poisoned: every byte must be written
    wq4.check(L.wq4_layernorm(_p(xd), _p(gd), _p(bd), m, d, prec, _p(got), None, st))
    tiled = torch.zeros((atb,), dtype=torch.uint8, device="cuda:0")
    wq4.check(L.wq4_tile_activations(_p(y), m, d, d, prec, _p(tiled), atb, st))
    torch.cuda.synchronize()
    ns = 2 if prec == 0 else 1
    kbp = ((d // 32 + 1) // 2) * 2
    nmt, kb = -(-m // 32), -(-d // 32)
    gb = got.cpu().numpy().reshape(-1, kbp, 2, ns, 1024)[:nmt, :kb]
    wb = tiled.cpu().numpy().reshape(-1, kbp, 2, ns, 1024)[:nmt, :kb]
    assert np.array_equal(gb, wb)


# ------------------------------------------------------------- embedding --
V, CTX = 51866, 448
_TABLES = {}


def _tables(torch, d):
    """tok_emb [V, D], pos_emb [CTX, D] and gamma [D] on the device, one width at a time."""
    if d not in _TABLES:
        _TABLES.clear()
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(9000 + d)
        te = torch.randn((V, d), device="cuda:0", generator=gen) * 0.05
        pe = torch.randn((CTX, d), device="cuda:0", generator=gen) * 0.02
        gamma = torch.rand((d,), device="cuda:0", generator=gen) + 0.5
        _TABLES[d] = (te, pe, gamma, pe.cpu().numpy(), gamma.cpu().numpy())
    return _TABLES[d]


def _tokens(B, Tq, rng):
    """Ids at the vocabulary's ends, a repeat, and random ones."""
    tok = rng.integers(0, V, B * Tq).astype(np.int32)
    tok[-1] = 0
    tok[0] = V - 1
    if tok.size > 2:
        tok[1] = V - 1  # a repeat
    if tok.size > 3:
        tok[2] = tok[3]
    return tok


GUARD = 4096


@pytest.mark.parametrize("B,Tq", [(1, 1), (33, 1), (2, 4), (5, 3)])
@pytest.mark.parametrize("d", [384, 1024, 1280])
def test_embed_vs_numpy(torch, d, B, Tq):
    """embed_kernel and embed_fold_kernel (planes 2 and 1) at pos0 = 0, 227 and
    ctx - Tq, the position from the host and from the device state: x equals
    numpy's f32 tok_emb[token] + pos_emb[p] bit for bit; the operand equals
    wq4_tile_activations of numpy's f32 x * gamma bit for bit on every half
    the rows own and no other byte of the buffer changes; the 16-column tile
    statistics match float64; poisoned guards after x and after the
    statistics stay untouched."""
    te, pe, gamma, pe_h, gamma_h = _tables(torch, d)
    R = B * Tq
    rng = np.random.default_rng(d + 17 * B + Tq)
    tok = _tokens(B, Tq, rng)
    te_rows = te[torch.from_numpy(tok.astype(np.int64)).to("cuda:0")].cpu().numpy()
    L = wq4.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    worst_mean = worst_m2 = 0.0
    for pos0 in (0, 227, CTX - Tq):
        p = pos0 + np.arange(R) % Tq
        x_want = fr.embed_ref(tok, te_rows, pe_h[p])
        mean64, m264 = fr.tile_stats64(x_want)
        xg = dev(torch, (x_want * gamma_h[None, :]).astype(np.float32))
        for use_state in (False, True):
            for prec in (None, wq4.PREC_F16X2, wq4.PREC_F16):
                what = (pos0, use_state, prec)
                x = torch.full((R * d + GUARD,), float("nan"), device="cuda:0")
                if prec is None:
                    whisper_amd.embed_check(tok, te, pe, B, Tq, pos0, use_state, x=x)
                else:
                    atb = L.wq4_atiled_bytes(R, d, prec)
                    tiled = torch.full((atb + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
                    stats = torch.full((R * (d // 16) * 2 + GUARD,), 12345.0, device="cuda:0")
                    whisper_amd.embed_check(tok, te, pe, B, Tq, pos0, use_state, gamma, prec, x=x, tiled=tiled,
                                            stats=stats)
                xs = x.cpu().numpy()
                assert np.array_equal(xs[: R * d].reshape(R, d).view(np.uint32), x_want.view(np.uint32)), what
                assert np.all(np.isnan(xs[R * d:])), what
                if prec is None:
                    continue
                want_t = torch.zeros((atb,), dtype=torch.uint8, device="cuda:0")
                wq4.check(L.wq4_tile_activations(_p(xg), R, d, d, prec, _p(want_t), atb, st))
                torch.cuda.synchronize()
                ns = 2 if prec == wq4.PREC_F16X2 else 1
                idx = fr.atile_halves(R, d, ns).reshape(-1)
                assert idx.max() < atb // 2
                got_h = tiled.cpu().numpy().view(np.uint16)
                want_h = want_t.cpu().numpy().view(np.uint16)
                assert np.array_equal(got_h[idx], want_h[idx]), what
                rest = np.ones(got_h.size, bool)
                rest[idx] = False
                assert np.all(got_h[rest] == 0x5A5A), what  # pad rows of the m-tile and the guard: not written
                s = stats.cpu().numpy()
                n = R * (d // 16) * 2
                assert np.all(s[n:] == 12345.0), what
                got_s = s[:n].reshape(R, d // 16, 2)
                assert np.allclose(got_s[..., 0], mean64, rtol=1e-5, atol=1e-5), what
                assert np.allclose(got_s[..., 1], m264, rtol=1e-4, atol=1e-4), what
                worst_mean = max(worst_mean, float(np.max(np.abs(got_s[..., 0] - mean64) / (1e-5 + 1e-5 * np.abs(mean64)))))
                worst_m2 = max(worst_m2, float(np.max(np.abs(got_s[..., 1] - m264) / (1e-4 + 1e-4 * np.abs(m264)))))
    print(f"FRONT_RATIO embed D={d} B={B} Tq={Tq} mean {worst_mean:.1e} M2 {worst_m2:.1e}")


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("kern", [3, 2])
def test_embed_fold_feeds_the_lnfold_consumer(torch, prec, kern):
    """D = 1280, B * Tq = 4: the entry's operand and statistics through the
    LayerNorm-fold consumer wq4_gemm_tiled_lnfold, and the entry's x through
    wq4_layernorm -> wq4_gemm_tiled, both against float64 LayerNorm(x) W^T + b
    under test_ln_fold_matches_layernorm_path's bound (c sum_k |W LN(x)| +
    1e-6, c = 8e-6 f16x2 / 1.2e-3 f16)."""
    d, n2, B, Tq, pos0 = 1280, 1280, 2, 2, 227
    m = B * Tq
    te, pe, gamma, pe_h, gamma_h = _tables(torch, d)
    rng = np.random.default_rng(77 + prec)
    tok = _tokens(B, Tq, rng)
    w2 = wq4.Q4Tensor.from_q4_bytes(oracle.quantize_convert_np((rng.standard_normal(n2 * d) * 0.04).astype(np.float32)),
                                    [n2, d])
    be = rng.uniform(-0.1, 0.1, d).astype(np.float32)
    b2 = (rng.standard_normal(n2) * 0.1).astype(np.float32)
    L = wq4.lib()
    wq4.set_kernel_policy(kern)
    assert L.wq4_lnfold_supported(w2.handle, m) == 1
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))  # noqa: E731
    x, at_f, stats = whisper_amd.embed_check(tok, te, pe, B, Tq, pos0, True, gamma, prec)
    # fold consumer on the entry's operand and statistics
    wg, b2f = np.zeros(n2, np.float32), np.zeros(n2, np.float32)
    wq4.check(L.wq4_ln_fold_vectors(w2.handle, fp(gamma_h), fp(be), fp(b2), fp(wg), fp(b2f)))
    wgd, b2fd = dev(torch, wg), dev(torch, b2f)
    cons = wq4.LnFold(None, None, None, stats.data_ptr(), wgd.data_ptr())
    z = torch.zeros((m, n2), device="cuda:0")
    wq4.check(L.wq4_gemm_tiled_lnfold(w2.handle, _p(b2fd), _p(at_f), None, _p(z), None, m, 0, prec, ctypes.byref(cons),
                                      st))
    # plain path on the entry's x
    at_ln = torch.zeros(L.wq4_atiled_bytes(m, d, prec), dtype=torch.uint8, device="cuda:0")
    bed, b2d = dev(torch, be), dev(torch, b2)
    wq4.check(L.wq4_layernorm(_p(x), _p(gamma), _p(bed), m, d, prec, _p(at_ln), None, st))
    z_ref = torch.zeros((m, n2), device="cuda:0")
    wq4.check(L.wq4_gemm_tiled(w2.handle, _p(b2d), _p(at_ln), None, _p(z_ref), None, m, 0, prec, 2, st))
    torch.cuda.synchronize()
    xs = x.cpu().numpy().astype(np.float64)
    mu = xs.mean(axis=1, keepdims=True)
    ln = (xs - mu) / np.sqrt(((xs - mu) ** 2).mean(axis=1, keepdims=True) + 1e-5) * gamma_h + be
    w2d = w2.dequantize_host().astype(np.float64)
    z64 = ln @ w2d.T + b2
    scale = np.abs(ln) @ np.abs(w2d).T
    c = 8e-6 if prec == 0 else 1.2e-3
    worst = 0.0
    for zz in (z_ref, z):
        err = np.abs(zz.cpu().numpy() - z64)
        worst = max(worst, float(np.max(err / (c * scale + 1e-6))))
        assert np.all(err <= c * scale + 1e-6), float(np.max(err / (scale + 1e-30)))
    print(f"FRONT_RATIO embed-chain prec={prec} kern={kern} {worst:.3f}")


def test_embed_rejects_bad_arguments(torch):
    """Out-of-range tokens and positions are refused with WQ4_EINVAL on the
    host side of the entry: no kernel runs (the poisoned x stays as it was)."""
    d = 384
    te = torch.zeros((64, d), device="cuda:0")
    pe = torch.zeros((16, d), device="cuda:0")
    gamma = torch.ones((d,), device="cuda:0")
    x = torch.full((4 * d,), 7.5, device="cuda:0")

    def status(tokens, B, Tq, pos0, use_state=False, g=None, D=d, Vv=64, ctx=16):
        tok = np.asarray(tokens, np.int32)
        tiled = torch.zeros(wq4.lib().wq4_atiled_bytes(4, d, 0), dtype=torch.uint8, device="cuda:0")
        stats = torch.zeros(4 * (d // 16) * 2, device="cuda:0")
        return whisper_amd.lib().wa_embed_check(0, tok.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _p(te), Vv,
                                                _p(pe), ctx, B, Tq, D, pos0, int(use_state), None, _p(g), 0, _p(x),
                                                _p(tiled) if g is not None else None,
                                                _p(stats) if g is not None else None)

    for g in (None, gamma):
        for use_state in (False, True):
            assert status([0, 64, 1, 2], 2, 2, 0, use_state, g) == EINVAL  # token == V
            assert status([0, 1, -1, 2], 2, 2, 0, use_state, g) == EINVAL  # negative token
            assert status([0, 1, 2, 3], 2, 2, 15, use_state, g) == EINVAL  # pos0 + Tq == ctx + 1
            assert status([0, 1, 2, 3], 2, 2, -1, use_state, g) == EINVAL
            assert status([0, 1, 2, 3], 0, 2, 0, use_state, g) == EINVAL
            assert status([0, 1, 2, 3], 2, 0, 0, use_state, g) == EINVAL
            assert status([0, 1, 2, 3], 2, 2, 0, use_state, g, D=0) == EINVAL
            assert status([0, 1, 2, 3], 2, 2, 0, use_state, g, Vv=3) == EINVAL  # token 3 with V = 3
    assert status([0, 1, 2, 3], 2, 2, 0, False, gamma, D=48) == EINVAL  # the folded form needs D % 32 == 0
    torch.cuda.synchronize()
    assert bool((x == 7.5).all())
    assert status([0, 63, 1, 2], 2, 2, 14) == 0  # the ends of both ranges are accepted
    torch.cuda.synchronize()
    assert not bool((x == 7.5).any())
