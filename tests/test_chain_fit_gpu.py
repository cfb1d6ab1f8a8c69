"""The decode chain's fit forms against the forms they replace, bit for bit.

The 8-wave Q4 f16x2 plans of q4_gemm_decode_kernel (2 or 3 block pairs per
wave) and xattn_out_kernel at 4 rows per workgroup have a form that needs at
most 128 registers, so that two workgroups share a CU (DESIGN.md section 10,
"chain fit"); it is the default for GEMMs of more than 16 rows and for
cross-attention plans of up to 6 splits.  WQ4_DECODE_FORM and
WA_XATTN_OUT_FORM, read at every launch, force it (1) or the earlier
one-per-CU instantiations (0) everywhere.  The arithmetic is the same, so
every output must be equal bitwise under all three settings: the f32 rows,
the A-tiled operands, the LayerNorm-fold statistics.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
import wq4
from q4_guard import gemm_guarded, tile_activations, to_dev

pytestmark = pytest.mark.gpu

GEMM_ENV, OUT_ENV, SPLITS_ENV = "WQ4_DECODE_FORM", "WA_XATTN_OUT_FORM", "WA_XATTN_SPLITS_RT"
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available(), "GPU tests need an MI355X"
    return _t


@pytest.fixture(autouse=True)
def _reset_modes():
    yield
    wq4.set_precision(wq4.PREC_F16X2)
    wq4.set_kernel_policy(0)


def _both_forms(monkeypatch, env, run):
    """run() under the fit form (env=1: at every row count / split count),
    under the default routing (fit for more than 16 GEMM rows and for plans
    of up to 6 splits) and under env=0, the one-per-CU form.  Returns (the
    fit form's and the default's outputs, the one-per-CU form's twice)."""
    monkeypatch.setenv(env, "1")
    fit = run()
    monkeypatch.delenv(env)
    default = run()
    monkeypatch.setenv(env, "0")
    old = run()
    monkeypatch.delenv(env)
    return fit + default, old + old


def _same(new, old, what):
    assert len(new) == len(old)
    for i, (a, b) in enumerate(zip(new, old)):
        name = f"{'fit' if i < len(new) // 2 else 'default'} form, output {i % (len(new) // 2)}"
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype
        diff = np.count_nonzero(a.view(np.uint8) != b.view(np.uint8))
        assert diff == 0, f"{what}: {name} differs from the one-per-CU form in {diff} of {a.nbytes} bytes"


# rows: 33 takes two m-tile launches; N = 96 is padded to 128 columns;
# K = 1280: 3 block pairs per wave, one K slice; K = 5120: 4 slices, slab merge
ROWS, NS, KS = (1, 5, 32, 33), (64, 96), (1280, 5120)
PLAN = {1280: {"w": 8, "per": 3, "ks": 1, "chunk": 3}, 5120: {"w": 8, "per": 3, "ks": 4, "chunk": 3}}


class Operands:
    """Random Q4_0 weights [96, 5120] and 33 rows of activations, made once;
    a case uses the leading rows, columns and whole Q4 blocks."""

    def __init__(self):
        rng = np.random.default_rng(950)
        self.q = oracle.quantize_convert_np((rng.standard_normal(96 * 5120) * 0.05).astype(np.float32)).reshape(96, 160, 18)
        self.x = rng.standard_normal((33, 5120)).astype(np.float32)
        self.bias = (rng.standard_normal(96) * 0.1).astype(np.float32)
        self.res = rng.standard_normal((33, 96)).astype(np.float32)
        self.gamma = rng.uniform(0.8, 1.2, 96).astype(np.float32)

    def weights(self, n, k):
        return wq4.Q4Tensor.from_q4_bytes(np.ascontiguousarray(self.q[:n, :k // 32]).ravel(), [n, k])


@pytest.fixture(scope="module")
def ops():
    return Operands()


def _assert_plan(n, k, rows):
    plan = wq4.gemm_plan(n, k, rows, 0)
    want = dict(PLAN[k], kernel=2, launches=-(-rows // 32))
    assert plan == want, (plan, want)


@pytest.mark.parametrize("prec", [wq4.PREC_F16X2, wq4.PREC_F16])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_gemm_fit_form_equals_one_per_cu_form(torch, monkeypatch, ops, n, k, prec):
    """Plain, residual and GELU-tiled epilogues at every row count."""
    wq4.set_kernel_policy(2)
    wq4.set_precision(prec)
    t = ops.weights(n, k)
    bias_d = to_dev(torch, ops.bias[:n], (n,))
    for rows in ROWS:
        _assert_plan(n, k, rows)
        at = tile_activations(torch, np.ascontiguousarray(ops.x[:rows, :k]), rows, k, prec)
        res_d = to_dev(torch, ops.res[:rows, :n], (rows, n))
        for flags in (0, 2, 5):
            what = f"rows {rows} n {n} k {k} prec {prec} flags {flags}"
            new, old = _both_forms(monkeypatch, GEMM_ENV, lambda: (
                gemm_guarded(torch, t, at, bias_d, res_d, rows, n, flags, False, prec, 2, what),))
            _same(new, old, what)


def _lnfold(torch, t, bias_d, at, res_d, out_tiled, rows, n, flags, prec, fold):
    L = wq4.lib()
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda a: vp(a.data_ptr()) if a is not None else None  # noqa: E731
    y = None if out_tiled is not None else (res_d.clone() if res_d is not None else torch.zeros((rows, n), device="cuda:0"))
    wq4.check(L.wq4_gemm_tiled_lnfold(t.handle, p(bias_d), p(at), p(y) if flags & 2 else None, p(y), p(out_tiled), rows,
                                      flags, prec, ctypes.byref(fold), st))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("prec", [wq4.PREC_F16X2, wq4.PREC_F16])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_lnfold_producer_fit_form(torch, monkeypatch, ops, n, k, prec):
    """The residual GEMM that also emits tiled(x gamma) and the 16-column
    tile statistics: x, the operand and the statistics."""
    wq4.set_precision(prec)
    L = wq4.lib()
    t = ops.weights(n, k)
    bias_d, gam_d = to_dev(torch, ops.bias[:n], (n,)), to_dev(torch, ops.gamma[:n], (n,))
    for rows in (1, 5, 32):
        wq4.set_kernel_policy(2)
        _assert_plan(n, k, rows)
        wq4.set_kernel_policy(0)
        assert L.wq4_lnfold_supported(t.handle, rows) == 1
        at = tile_activations(torch, np.ascontiguousarray(ops.x[:rows, :k]), rows, k, prec)
        res_d = to_dev(torch, ops.res[:rows, :n], (rows, n))

        def run():
            at_f = torch.full((L.wq4_atiled_bytes(rows, n, prec),), 0x5A, dtype=torch.uint8, device="cuda:0")
            stats = torch.zeros(rows * (n // 16) * 2, device="cuda:0")
            fold = wq4.LnFold(gam_d.data_ptr(), at_f.data_ptr(), stats.data_ptr(), None, None)
            x = _lnfold(torch, t, bias_d, at, res_d, None, rows, n, 2, prec, fold)
            return x.cpu().numpy(), at_f.cpu().numpy(), stats.cpu().numpy()

        new, old = _both_forms(monkeypatch, GEMM_ENV, run)
        _same(new, old, f"producer rows {rows} n {n} k {k} prec {prec}")


@pytest.mark.parametrize("prec", [wq4.PREC_F16X2, wq4.PREC_F16])
@pytest.mark.parametrize("n", NS)
def test_lnfold_consumer_fit_form(torch, monkeypatch, ops, n, prec):
    """The GEMM on LayerNorm(x) from the tile statistics (K = 1280): f32 and
    GELU-tiled outputs."""
    k = 1280
    wq4.set_precision(prec)
    L = wq4.lib()
    t = ops.weights(n, k)
    bias_d = to_dev(torch, ops.bias[:n], (n,))
    wg_d = to_dev(torch, ops.res[0, :n] * 0.1, (n,))
    for rows in (1, 5, 32):
        wq4.set_kernel_policy(2)
        _assert_plan(n, k, rows)
        wq4.set_kernel_policy(0)
        assert L.wq4_lnfold_supported(t.handle, rows) == 1
        x = np.ascontiguousarray(ops.x[:rows, :k])
        at = tile_activations(torch, x, rows, k, prec)
        tiles = x.reshape(rows, k // 16, 16).astype(np.float64)
        mean = tiles.mean(axis=2)
        m2 = ((tiles - mean[:, :, None]) ** 2).sum(axis=2)
        stats = to_dev(torch, np.stack([mean, m2], axis=2).astype(np.float32), (rows * (k // 16) * 2,))
        fold = wq4.LnFold(None, None, None, stats.data_ptr(), wg_d.data_ptr())
        for flags in (0, 5):

            def run():
                zt = None
                if flags & 4:
                    zt = torch.full((L.wq4_atiled_bytes(rows, n, prec),), 0x5A, dtype=torch.uint8, device="cuda:0")
                z = _lnfold(torch, t, bias_d, at, None, zt, rows, n, flags, prec, fold)
                return ((zt if zt is not None else z).cpu().numpy(),)

            new, old = _both_forms(monkeypatch, GEMM_ENV, run)
            assert np.all(np.isfinite(new[0])) if not flags & 4 else True
            _same(new, old, f"consumer rows {rows} n {n} prec {prec} flags {flags}")


# ------------------------------------------------------------- xattn_out --
# forced splits 1, 5, 6, 8: the instantiated split maxima are 5, 6 and 8, so
# S = 1 and 5 run SM = 5 (5 exactly), 6 runs SM = 6, 8 runs SM = 8; T = 40 has
# fewer sub-chunks than splits and clamps.  Rows 1 and 4 take the few-rows
# path (4 workgroups per head), 5 and 32 the fused one; 5 leaves a workgroup
# with one real row of four.
@pytest.mark.parametrize("T", [40, 1500])
@pytest.mark.parametrize("H", [20, 6])
def test_xattn_out_fit_form_equals_one_per_cu_form(torch, monkeypatch, H, T):
    import whisper_amd

    D = 64 * H
    rng = np.random.default_rng(100 * H + T)
    enc = torch.from_numpy(rng.standard_normal((1, T, D)).astype(np.float32)).cuda()
    q_all = torch.from_numpy((2.0 * rng.standard_normal((32, D))).astype(np.float32)).cuda()
    rk = torch.from_numpy(wq4.quantize_q4_0(rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32))).cuda()
    rv = torch.from_numpy(wq4.quantize_q4_0(rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32))).cuda()
    bv = torch.from_numpy(rng.uniform(-0.02, 0.02, D).astype(np.float32)).cuda()
    monkeypatch.delenv("WA_XATTN_SMALL_ROWS", raising=False)
    for R in (1, 4, 5, 32):
        q = q_all[:R].contiguous()
        for S in (1, 5, 6, 8):
            monkeypatch.setenv(SPLITS_ENV, str(S))
            # one clip, R query positions: R rows over the same encoder planes
            new, old = _both_forms(monkeypatch, OUT_ENV, lambda: (
                whisper_amd.xattn_check(q, rk, rv, bv, enc, R, H).cpu().numpy(),))
            assert np.all(np.isfinite(new[0]))
            _same(new, old, f"xattn_out H {H} T {T} rows {R} splits {S}")
