"""The Q4 GEMM kernels at 128 rows and below -- q4_gemm_decode_kernel (rows
<= 128) and skinny_gemm_kernel (rows <= 32, the decode step) -- at a covering
set of shapes chosen by launch plan (q4_small_shapes.py), run on an MI355X.

Both kernels choose waves, block pairs per wave, K slices per n-tile and
subtiles per workgroup from (N, K); with more than one K slice the partial sums
meet through write-through slabs, an arrival counter and a last-arriver merge
on the stream's one workspace.  Per case, on the kernel the case names:

  * wq4.gemm_plan equals the plan restated in q4_small_shapes.py, before the
    launch;
  * the output lies between the poisoned guards of q4_guard.py: guards
    untouched, every f32 element written;
  * the f32 result (bias included; flags 0) is held to float64 by
    assert_q4_close under TOL of test_q4_gpu.py, unchanged -- for f16 weights
    against the f16 values themselves, as test_f16_weights_gemm does;
  * the case's epilogue variant: the residual (in place or separate) held to
    float64 the same way; the A-tiled output bit-equal to
    wq4_tile_activations of the checked f32 result; GELU (flags 1, 3) applied
    to the checked f32 result -- the kernel's pre-activation, bit for bit --
    in float64, under the bound of test_gelu_epilogue_vs_float64
    (2e-6 |x| + 1e-6 |gelu x|; plus one f32 rounding of the sum with a
    residual);
  * with ks > 1: the variant's launch three times in a row with identical
    bits, then a launch of another (N, K) whose ks differs, held to float64
    (the counters' re-arm; the merge in slice order whatever arrived last).

test_rows_are_batch_invariant: per (kernel, ks), rows 0, 15, 16 and the last
of a full call equal one-row calls bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import q4_small_shapes as S
import wq4
from q4_guard import assert_atiled_equals_tiled_f32, gemm_guarded, tile_activations
from test_q4_gpu import assert_q4_close, to_dev

pytestmark = pytest.mark.gpu

NB, KB, MB = 1312, 12288, 128  # the base problem every case is cut from


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


class Base:
    """One set of random operands, made once and never changed: Q4_0 blocks
    and f16 weights [1312, 12288], activations and a residual of 128 rows, a
    bias.  A case uses rows [:n] and columns [:k] (whole Q4 blocks: the slice
    of the quantized weight is the quantized slice)."""

    def __init__(self):
        rng = np.random.default_rng(128)
        w = (rng.standard_normal(NB * KB) * 0.05).astype(np.float32)
        self.q = oracle.quantize_convert_np(w).reshape(NB, KB // 32, 18)
        self.deq = oracle.dequantize_np(self.q.ravel(), NB * KB).reshape(NB, KB)
        self.w16 = (w.reshape(NB, KB) * 0.6).astype(np.float16)
        self.x = rng.standard_normal((MB, KB)).astype(np.float32)
        self.bias = (rng.standard_normal(8208) * 0.1).astype(np.float32)
        self.res = rng.standard_normal((MB, NB)).astype(np.float32)

    def weights(self, n, k, wt):
        """(tensor, the float32 values it stands for) of [n, k]."""
        if n <= NB:
            q, deq, w16 = self.q[:n, :k // 32], self.deq[:n, :k], self.w16[:n, :k]
        else:  # the decode-step cases past N = 1312: small K, made on the spot
            rng = np.random.default_rng(n + k)
            w = (rng.standard_normal(n * k) * 0.05).astype(np.float32)
            q = oracle.quantize_convert_np(w)
            deq, w16 = oracle.dequantize_np(q, n * k).reshape(n, k), (w.reshape(n, k) * 0.6).astype(np.float16)
        if wt == S.F16W:
            w16 = np.ascontiguousarray(w16)
            return wq4.Q4Tensor.from_f16(w16), w16.astype(np.float32)
        return wq4.Q4Tensor.from_q4_bytes(np.ascontiguousarray(q).ravel(), [n, k]), np.ascontiguousarray(deq)

    def residual(self, rows, n):
        if n <= NB:
            return np.ascontiguousarray(self.res[:rows, :n])
        return np.random.default_rng(n).standard_normal((rows, n)).astype(np.float32)


@pytest.fixture(scope="module")
def base():
    return Base()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _gelu64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):  # far negative v: x / inf = -0, as wanted
        return v / (1.0 + np.exp(-2.0 * 0.7978845608028654 * (v + 0.044715 * v**3)))


def _plan_tag(kernel, p):
    return f"kernel 2 per {p['per']} ks {p['ks']}" if kernel == 2 else f"kernel 3 ks {p['ks']} nt {p['nt']} rt {p['row_tiles']}"


def _run_case(torch, base, kernel, rows, n, k, flags, inplace, prec, wt, repeat):
    """One case of the table; returns (plan, worst err / bound)."""
    wq4.set_kernel_policy(kernel)
    wq4.set_precision(prec)
    plan = wq4.gemm_plan(n, k, rows, wt)
    assert plan == S.expected_plan(kernel, n, k, rows) and plan["kernel"] == kernel, plan
    t, wval = base.weights(n, k, wt)
    if kernel == 3:
        assert t.has_decode_step
    x, bias, res = np.ascontiguousarray(base.x[:rows, :k]), base.bias[:n], base.residual(rows, n)
    at = tile_activations(torch, x, rows, k, prec)
    bias_d, res_d = to_dev(torch, bias, (n,)), to_dev(torch, res, (rows, n))
    what = f"{_plan_tag(kernel, plan)} {(rows, n, k)} prec {prec} weights {wt}"

    def launch(f, ip):
        return gemm_guarded(torch, t, at, bias_d, res_d, rows, n, f, ip, prec, kernel, f"{what} flags {f}")

    y0 = launch(0, False)
    worst = assert_q4_close(y0, x, wval, prec=prec, bias=bias, what=what + " flags 0")
    out = y0
    if flags:
        out = launch(flags, inplace)
    if flags == 2:
        worst = max(worst, assert_q4_close(out, x, wval, prec=prec, bias=bias, residual=res, what=what + " flags 2"))
    elif flags & 1:
        # GELU of the kernel's own pre-activation (y0, bit for bit); the bound of test_gelu_epilogue_vs_float64
        v = y0.astype(np.float64)
        want = _gelu64(v)
        bound = 2e-6 * np.abs(v) + 1e-6 * np.abs(want) + 1e-37
        if flags & 2:
            want = want + res.astype(np.float64)
            bound = bound + 2.0**-24 * np.abs(want)
        err = np.abs(out.astype(np.float64) - want)
        assert np.all(err <= bound), f"{what} flags {flags}: max err/bound {float(np.max(err / bound)):.3g}"
    elif flags == 4:
        assert_atiled_equals_tiled_f32(torch, out, y0, rows, n, prec, 32 if kernel == 2 else 16, what + " flags 4")
    if repeat:
        for i in (2, 3):
            again = launch(flags, inplace)
            diff = np.count_nonzero(_bits(again) != _bits(out))
            assert diff == 0, f"{what} flags {flags}: launch {i} differs from the first in {diff} of {out.size} places"
        # another (N, K) with another ks on the same workspace and counters
        n2, k2, rows2 = S.FOLLOW[kernel][1 if S.expected_plan(kernel, *S.FOLLOW[kernel][0])["ks"] == plan["ks"] else 0]
        plan2 = wq4.gemm_plan(n2, k2, rows2)
        assert plan2 == S.expected_plan(kernel, n2, k2, rows2) and plan2["kernel"] == kernel and plan2["ks"] != plan["ks"]
        t2, wval2 = base.weights(n2, k2, S.Q4)
        x2 = np.ascontiguousarray(base.x[:rows2, :k2])
        at2 = tile_activations(torch, x2, rows2, k2, prec)
        b2 = to_dev(torch, base.bias[:n2], (n2,))
        y = gemm_guarded(torch, t2, at2, b2, None, rows2, n2, 0, False, prec, kernel, what + f" then {(rows2, n2, k2)}")
        assert_q4_close(y, x2, wval2, prec=prec, bias=base.bias[:n2], what=what + f" then {(rows2, n2, k2)} ks {plan2['ks']}")
    return plan, worst


def _id(c):
    return "k{}-m{}-n{}-K{}-f{}{}-p{}-w{}".format(c[0], c[1], c[2], c[3], c[4], "i" if c[5] else "", c[6], c[7])


@pytest.mark.parametrize("case", S.CASES, ids=_id)
def test_small_gemm_by_plan(torch, base, case):
    """Every case of q4_small_shapes.CASES as the module docstring describes;
    the launch-independence part for every case with ks > 1."""
    kernel, rows, n, k, flags, inplace, prec, wt = case
    repeat = S.expected_plan(kernel, n, k, rows)["ks"] > 1
    plan, worst = _run_case(torch, base, kernel, rows, n, k, flags, inplace, prec, wt, repeat)
    print(f"q4small {_plan_tag(kernel, plan)} prec {prec} weights {wt} rows {rows} n {n} k {k} flags {flags}: "
          f"err/bound {worst:.3f}")


@pytest.mark.parametrize("case", S.CONTROLS, ids=_id)
def test_launch_independence_control_ks1(torch, base, case):
    """The launch-independence sequence at ks = 1 (no slabs, no counter):
    three launches with identical bits, then a ks > 1 launch of another
    shape."""
    kernel, rows, n, k, flags, inplace, prec, wt = case
    plan, worst = _run_case(torch, base, kernel, rows, n, k, flags, inplace, prec, wt, True)
    assert plan["ks"] == 1
    print(f"q4small control {_plan_tag(kernel, plan)} prec {prec} rows {rows} n {n} k {k}: err/bound {worst:.3f}")


@pytest.mark.parametrize("kernel,rows,n,k", S.BATCH, ids=lambda v: str(v))
def test_rows_are_batch_invariant(torch, base, kernel, rows, n, k):
    """Per (kernel, ks): rows 0, 15, 16 and the last row of the full call
    equal, bit for bit, a one-row call on that row -- a row's arithmetic
    depends on K only (the plan's ks and the wave split are functions of K;
    nt and the row tiles only move work between workgroups)."""
    prec = wq4.PREC_F16X2
    wq4.set_kernel_policy(kernel)
    wq4.set_precision(prec)
    full, one = wq4.gemm_plan(n, k, rows), wq4.gemm_plan(n, k, 1)
    assert full == S.expected_plan(kernel, n, k, rows) and full["kernel"] == kernel
    assert one["kernel"] == kernel and one["ks"] == full["ks"]
    t, wval = base.weights(n, k, S.Q4)
    bias_d = to_dev(torch, base.bias[:n], (n,))
    x = np.ascontiguousarray(base.x[:rows, :k])
    what = f"{_plan_tag(kernel, full)} {(rows, n, k)}"
    y = gemm_guarded(torch, t, tile_activations(torch, x, rows, k, prec), bias_d, None, rows, n, 0, False, prec, kernel, what)
    assert_q4_close(y, x, wval, prec=prec, bias=base.bias[:n], what=what)
    for r in (0, 15, 16, rows - 1):
        y1 = gemm_guarded(torch, t, tile_activations(torch, x[r:r + 1], 1, k, prec), bias_d, None, 1, n, 0, False, prec,
                          kernel, what + f" row {r} alone")
        diff = np.count_nonzero(y1.view(np.uint32) != y[r:r + 1].view(np.uint32))
        assert diff == 0, f"{what}: row {r} alone differs from the full call in {diff} of {n} columns"
