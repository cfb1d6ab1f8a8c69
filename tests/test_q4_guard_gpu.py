"""Guard bands past every output of the Q4 kernels, and float64 parity of the
encoder-size GEMM kernels above 128 rows (run on an MI355X).

Every output -- f32 rows, head-major f32, the A-tiled operand of a following
GEMM -- is the interior of a poisoned allocation (q4_guard.py): after the
launch both guards still hold the poison bit for bit and every f32 element of
the interior was written.  The f32 epilogue of the tile and wide kernels
(wq4_tile_epi.hpp, EPI == kEpiF32) drops padded rows only through the buffer
descriptor's range check on voffset + soffset, and masked columns through
kEpiOob + soffset; these tests are what establishes that on the hardware.

Above 128 rows each mode's kernel is named before it runs (wq4_gemm_kernel_name
against q4_shapes.expected_kernel), mode 0 (the tile kernel) is held to float64
with TOL of test_q4_gpu.py and every other mode to mode 0's bits.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import q4_shapes
import wq4
from q4_guard import check_guards, guarded_bytes, guarded_f32
from q4_guard import gemm_guarded as _gemm_guarded, problem as _problem, small_gemm as _small_gemm
from test_q4_gpu import assert_q4_close, to_dev

pytestmark = pytest.mark.gpu

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


def _stream(torch):
    return vp(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ----------------------------------------------------- rows > 128: kernel 1 --
@pytest.mark.parametrize("rows,n,k,flags,inplace,prec", q4_shapes.CASES)
def test_enc_gemm_guards_and_float64(torch, rows, n, k, flags, inplace, prec):
    """wq4_gemm_tiled, kernel 1, at the covering set of q4_shapes.py: the tile
    kernel (mode 0), the ring kernel's three geometries (2, 3, 4; f16x2 only)
    and the wide kernel (5).  Per mode: the routing as named, guards
    untouched, the interior fully written, bits equal to mode 0's.  Mode 0
    itself against float64 where the epilogue is linear (flags 0 and 2: bias
    included, the residual added to the truth), TOL unchanged."""
    rng = np.random.default_rng(rows * 7 + n * 3 + k)
    t, deq, x, at, bias, res = _problem(torch, rng, rows, n, k, prec)
    bias_d, res_d = to_dev(torch, bias, (n,)), to_dev(torch, res, (rows, n))
    L = wq4.lib()
    modes = [m for m in q4_shapes.enc_modes(prec) if m != 1]
    outs = {}
    prev = L.wq4_debug_set_enc_kernel(0)
    try:
        for mode in modes:
            assert L.wq4_debug_set_enc_kernel(mode) >= 0
            wq4.set_kernel_policy(1)
            wq4.set_precision(prec)
            assert wq4.gemm_kernel_name(n, k, rows) == q4_shapes.expected_kernel(mode, rows, n, prec), f"mode {mode}"
            outs[mode] = _gemm_guarded(torch, t, at, bias_d, res_d, rows, n, flags, inplace, prec, 1,
                                       f"mode {mode} {(rows, n, k)} flags {flags} prec {prec}")
    finally:
        L.wq4_debug_set_enc_kernel(prev)
    for mode in modes[1:]:
        diff = np.count_nonzero(_bits(outs[mode]) != _bits(outs[0]))
        assert diff == 0, f"mode {mode}: {diff} of {outs[0].size} outputs differ from the tile kernel's bits"
    if flags in (0, 2):
        worst = assert_q4_close(outs[0], x, deq, prec=prec, bias=bias, residual=res if flags & 2 else None,
                                what=f"tile kernel {(rows, n, k)} flags {flags}")
        print(f"rows {rows} n {n} k {k} flags {flags} prec {prec}: err/bound {worst:.3f}")


@pytest.mark.parametrize("prec", [0, 1])
def test_headmajor_guards(torch, prec):
    """wq4_gemm_tiled_headmajor, 3 groups of 50 rows (an m-tile spans two
    groups), K | V of d = 128, K = 64, on the tile, ring (f16x2) and wide
    kernels: guards on both sides of the [part][g][head][t][64] output, every
    element written, bits equal to the row-major tile-kernel result permuted
    -- which is itself held to float64."""
    groups, trows, d, k = 3, 50, 128, 64
    m, n = groups * trows, 2 * d
    rng = np.random.default_rng(150 + prec)
    t, deq, x, at, bias, res = _problem(torch, rng, m, n, k, prec)
    bias_d = to_dev(torch, bias, (n,))
    L = wq4.lib()
    prev = L.wq4_debug_set_enc_kernel(0)
    try:
        wq4.set_kernel_policy(1)
        wq4.set_precision(prec)
        assert wq4.gemm_kernel_name(n, k, m) == q4_shapes.TILE
        ref = _gemm_guarded(torch, t, at, bias_d, None, m, n, 0, False, prec, 1, "row-major reference")
        assert_q4_close(ref, x, deq, prec=prec, bias=bias, what="head-major reference")
        want = ref.reshape(groups, trows, 2, d // 64, 64).transpose(2, 0, 3, 1, 4).ravel()
        for mode in (0, 3, 5) if prec == 0 else (0, 5):
            assert L.wq4_debug_set_enc_kernel(mode) >= 0
            assert wq4.gemm_kernel_name(n, k, m) == q4_shapes.expected_kernel(mode, m, n, prec), f"mode {mode}"
            whole, view, ptr = guarded_f32(torch, m, n)
            wq4.check(L.wq4_gemm_tiled_headmajor(t.handle, vp(bias_d.data_ptr()), vp(at.data_ptr()), vp(ptr), m, trows,
                                                 d, prec, 1, _stream(torch)))
            torch.cuda.synchronize()
            check_guards(whole, view, what=f"head-major mode {mode}")
            got = view.cpu().numpy().ravel()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"head-major mode {mode}"
    finally:
        L.wq4_debug_set_enc_kernel(prev)


def test_guard_check_sees_one_row_past_the_end(torch):
    """Sensitivity, on the GPU and without any kernel misbehaving: a real
    300 x 100 GEMM on the wide kernel, its interior then declared as 299 rows
    -- the check must fail and name row 299, the one row past that end."""
    rows, n, k = 300, 100, 96
    rng = np.random.default_rng(299)
    t, deq, x, at, bias, res = _problem(torch, rng, rows, n, k, 0)
    bias_d = to_dev(torch, bias, (n,))
    L = wq4.lib()
    prev = L.wq4_debug_set_enc_kernel(5)
    try:
        wq4.set_kernel_policy(1)
        assert wq4.gemm_kernel_name(n, k, rows) == q4_shapes.WIDE
        whole, view, ptr = guarded_f32(torch, rows, n)
        wq4.check(L.wq4_gemm_tiled(t.handle, vp(bias_d.data_ptr()), vp(at.data_ptr()), None, vp(ptr), None, rows, 0, 0,
                                   1, _stream(torch)))
        torch.cuda.synchronize()
    finally:
        L.wq4_debug_set_enc_kernel(prev)
    check_guards(whole, view)
    with pytest.raises(AssertionError, match=r"100 guard elements written past the end.*first at row 299 column 0, "
                                             r"last at row 299 column 99 \(1 \.\. 1 rows past the end of 299 x 100\)"):
        check_guards(whole, view, rows=299)


# ------------------------------------------- rows <= 128: kernels 2 and 3 --
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("n,k", [(96, 160), (100, 96), (1312, 128)])
@pytest.mark.parametrize("rows", [1, 5, 33, 100])
def test_decode_kernel_guards(torch, rows, n, k, prec):
    """The K-split decode kernel (kernel 2) at 1, 5, 33 and 100 rows."""
    _small_gemm(torch, rows, n, k, prec, 2, "q4_gemm_decode_kernel", 32)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("n,k", [(96, 128), (1312, 384)])
@pytest.mark.parametrize("rows", [1, 7, 32])
def test_decode_step_kernel_guards(torch, rows, n, k, prec):
    """The decode-step ("skinny") kernel (kernel 3; K % 128 == 0, N % 16 == 0)
    at 1, 7 and 32 rows; N = 96 and 1312 end in half a 64-column slab.  Its
    A-tiled output comes in 16-row tiles: at up to 16 rows the m-tile's other
    16 rows are not written (they feed only output rows no one reads)."""
    _small_gemm(torch, rows, n, k, prec, 3, "skinny_gemm_kernel", 16)


# ------------------------------------ wq4_layernorm, wq4_tile_activations --
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("m,d", [(1, 96), (33, 160), (129, 1280), (2049, 96)])
def test_layernorm_and_tiling_guards(torch, prec, m, d):
    """wq4_layernorm's f32 rows and its A-tiled output (one wave per row up to
    2048 rows, layernorm_tiled_kernel above) and wq4_tile_activations' output,
    each inside guards: nothing before or after the operand is touched, every
    f32 element is written, and -- as in test_layernorm_tiled_equals_f32_then_tile
    -- the A-tiled LayerNorm equals the f32 LayerNorm rows tiled, bit for bit,
    over the m-tiles and blocks the LayerNorm writes."""
    rng = np.random.default_rng(m * 3 + d + prec)
    x = to_dev(torch, (rng.standard_normal(m * d) * 3 + 0.7).astype(np.float32), (m, d))
    g = to_dev(torch, rng.uniform(0.5, 1.5, d).astype(np.float32), (d,))
    be = to_dev(torch, rng.uniform(-0.2, 0.2, d).astype(np.float32), (d,))
    L = wq4.lib()
    st = _stream(torch)
    p = lambda a: vp(a.data_ptr())  # noqa: E731
    atb, guard = L.wq4_atiled_bytes(m, d, prec), L.wq4_atiled_bytes(256, d, prec)
    yw, y, yptr = guarded_f32(torch, m, d)
    wq4.check(L.wq4_layernorm(p(x), p(g), p(be), m, d, prec, None, vp(yptr), st))
    gw, got, gptr = guarded_bytes(torch, atb, guard)
    wq4.check(L.wq4_layernorm(p(x), p(g), p(be), m, d, prec, vp(gptr), None, st))
    ww, want, wptr = guarded_bytes(torch, atb, guard)
    wq4.check(L.wq4_tile_activations(vp(yptr), m, d, d, prec, vp(wptr), atb, st))
    torch.cuda.synchronize()
    check_guards(yw, y, what="wq4_layernorm f32 rows")
    check_guards(gw, got, what="wq4_layernorm A-tiled")
    check_guards(ww, want, what="wq4_tile_activations")
    ns = 2 if prec == 0 else 1
    kbp = ((d // 32 + 1) // 2) * 2
    nmt, kb = -(-m // 32), -(-d // 32)  # m-tiles and Q4 blocks the LayerNorm writes
    gb = got.cpu().numpy().reshape(-1, kbp, 2, ns, 1024)[:nmt, :kb]
    wb = want.cpu().numpy().reshape(-1, kbp, 2, ns, 1024)[:nmt, :kb]
    assert np.array_equal(gb, wb)
