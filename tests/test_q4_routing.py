"""CPU tests behind the Q4 guard tests (test_q4_guard_gpu.py): which kernel an
encoder-size GEMM runs, the covering shape table, and the guard check itself.
No GPU: wq4_gemm_kernel_name and wq4_debug_set_enc_kernel are host code."""
from __future__ import annotations

import numpy as np
import pytest

import q4_guard
import q4_shapes
import wq4


@pytest.fixture(autouse=True)
def _reset_modes():
    prev = wq4.lib().wq4_debug_set_enc_kernel(1)
    wq4.lib().wq4_debug_set_enc_kernel(prev)
    yield
    wq4.lib().wq4_debug_set_enc_kernel(prev)
    wq4.set_precision(wq4.PREC_F16X2)
    wq4.set_kernel_policy(0)


def test_shape_table_is_a_covering_set():
    """Every (rows, N) and every (N, K) pair once, every axis value used, at
    most 40 cases; both precisions and every epilogue variant occur, the
    A-tiled output only where N % 32 == 0."""
    c = q4_shapes.CASES
    assert len(c) <= 40
    assert sorted((r, n) for r, n, *_ in c) == sorted((r, n) for r in q4_shapes.ROWS for n in q4_shapes.NS)
    assert sorted((n, k) for _, n, k, *_ in c) == sorted((n, k) for n in q4_shapes.NS for k in q4_shapes.KS)
    assert {(f, ip) for *_, f, ip, _ in c} >= set(q4_shapes.VARIANTS)
    for prec in (q4_shapes.PREC_F16X2, q4_shapes.PREC_F16):
        assert {r for r, *_, p in c if p == prec} == set(q4_shapes.ROWS)
        assert {f for *_, f, _, p in c if p == prec} >= {0, 1, 2, 4}
    assert all(n % 32 == 0 for _, n, _, f, *_ in c if f & 4)
    assert all(f & 2 for *_, f, ip, _ in c if ip)


def test_enc_routing_of_every_tested_shape():
    """wq4_gemm_kernel_name against enc_gemm_pick's rule in literal numbers
    (q4_shapes.expected_kernel: rows > 128; the wide kernel from a grid of
    170; the ring kernel's S geometry below a tile grid of 400; the ring
    kernel only at f16x2) over the whole table of q4_shapes.py and the shapes
    of test_enc_kernel_bit_identical, under every encoder-kernel mode and both
    precisions -- so a GEMM test that silently ran another kernel than it
    names fails here, without a GPU.

    The wide kernel asks for an even n-tile count.  make_geom pads N to a
    multiple of 64 and counts n-tiles of 32, so the count is always even and
    a rows > 128 Q4_0 GEMM never falls back from mode 5: N = 96 and N = 1312
    (4 and 42 n-tiles) run on the wide kernel like every other N, K = 160
    included."""
    shapes = [(r, n, k) for r, n, k, *_ in q4_shapes.CASES] + [(m, n, k) for m, n, k, *_ in q4_shapes.ENC_BIT_IDENTICAL]
    L = wq4.lib()
    wq4.set_kernel_policy(1)
    seen = set()
    for prec in (wq4.PREC_F16X2, wq4.PREC_F16):
        wq4.set_precision(prec)
        for mode in range(6):
            assert L.wq4_debug_set_enc_kernel(mode) >= 0
            for rows, n, k in shapes:
                want = q4_shapes.expected_kernel(mode, rows, n, prec)
                assert wq4.gemm_kernel_name(n, k, rows) == want, (mode, prec, rows, n, k)
                seen.add((mode, want))
            for n in (32, 64, 96, 100, 1312, 5120):  # never a fallback from the wide kernel
                if mode == 5:
                    assert wq4.gemm_kernel_name(n, 160, 129) == q4_shapes.WIDE
            assert wq4.gemm_kernel_name(1280, 1280, 128) == q4_shapes.TILE  # rows > 128 only
    # the rule's every branch is taken by some tested shape
    assert seen >= {(0, q4_shapes.TILE), (1, q4_shapes.TILE), (1, q4_shapes.RING), (1, q4_shapes.WIDE),
                    (2, q4_shapes.RING), (3, q4_shapes.RING), (4, q4_shapes.RING), (2, q4_shapes.TILE),
                    (5, q4_shapes.WIDE)}


def test_enc_routing_thresholds():
    """Mode 1's thresholds from both sides: N = 1280 (5 n-groups) is on the
    wide kernel from 34 wide m-groups (170 workgroups: rows > 33 * 256) and on
    the ring kernel below; N = 64 (1 n-group) from 170 m-groups (rows > 169 *
    256); 128 rows are the tile kernel's, 129 the ring kernel's.  The tile grid
    has at most two workgroups per wide workgroup, so below 170 wide workgroups
    it stays under 340 < 400: at f16x2 operands mode 1 never picks the tile
    kernel above 128 rows, and the 400 in the rule decides nothing.  At f16
    operands it runs every grid the wide kernel does not take."""
    L = wq4.lib()
    wq4.set_kernel_policy(1)
    prev = L.wq4_debug_set_enc_kernel(1)
    try:
        for rows, n, want in ((33 * 256, 1280, q4_shapes.RING), (33 * 256 + 1, 1280, q4_shapes.WIDE),
                              (169 * 256, 64, q4_shapes.RING), (169 * 256 + 1, 64, q4_shapes.WIDE),
                              (128, 64, q4_shapes.TILE), (129, 64, q4_shapes.RING)):
            assert q4_shapes.expected_kernel(1, rows, n, wq4.PREC_F16X2) == want
            assert wq4.gemm_kernel_name(n, 64, rows) == want, (rows, n)
        wq4.set_precision(wq4.PREC_F16)  # f16 operands: never the ring kernel
        assert wq4.gemm_kernel_name(1280, 1280, 1500) == q4_shapes.TILE
        assert wq4.gemm_kernel_name(1280, 1280, 33 * 256 + 1) == q4_shapes.WIDE
    finally:
        L.wq4_debug_set_enc_kernel(prev)


# ------------------------------------------------------------- check_guards --
def test_check_guards_f32_self_test():
    """An untouched guarded f32 buffer whose interior is written passes; one
    planted element in either guard fails and is named by row; one interior
    element left unwritten fails."""
    import torch

    rows, n = 5, 12
    whole, view, ptr = q4_guard.guarded_f32(torch, rows, n, device="cpu")
    assert whole.numel() == (2 * q4_guard.G + rows) * n and ptr == whole.data_ptr() + q4_guard.G * n * 4
    bits = whole.view(torch.int32)
    assert bool((bits == q4_guard.POISON_F32).all()) and bool(torch.isnan(whole).all())
    with pytest.raises(AssertionError, match="60 of 5 x 12 outputs never written"):
        q4_guard.check_guards(whole, view)
    view.copy_(torch.arange(rows * n, dtype=torch.float32).view(rows, n))
    q4_guard.check_guards(whole, view)
    lo, hi = q4_guard.G * n, (q4_guard.G + rows) * n
    for idx, pattern in ((hi, "past the end.*first at row 5 column 0, last at row 5 column 0 \\(1 \\.\\. 1 rows"),
                         (hi + 255 * n + 11, "past the end.*first at row 260 column 11.*256 \\.\\. 256 rows"),
                         (lo - 1, "before the start.*first at row -1 column 11"),
                         (0, "before the start.*first at row -256 column 0")):
        keep = int(bits[idx])
        bits[idx] = keep ^ 1  # one flipped bit: still a NaN, only a bit-for-bit compare sees it
        with pytest.raises(AssertionError, match=pattern):
            q4_guard.check_guards(whole, view, what="planted")
        bits[idx] = keep
        q4_guard.check_guards(whole, view)
    # an interior declared one row short: the last real row counts as a stray write
    with pytest.raises(AssertionError, match="12 guard elements written past the end.*first at row 4 column 0"):
        q4_guard.check_guards(whole, view, rows=4)
    view[2, 3] = torch.tensor([q4_guard.POISON_F32], dtype=torch.int32).view(torch.float32)[0]
    with pytest.raises(AssertionError, match="1 of 5 x 12 outputs never written: first at row 2 column 3"):
        q4_guard.check_guards(whole, view)


def test_check_guards_bytes_self_test():
    import torch

    nbytes, guard = 3 * 1024, 2048
    whole, view, ptr = q4_guard.guarded_bytes(torch, nbytes, guard, device="cpu")
    off = view.storage_offset()
    assert ptr % 1024 == 0 and off >= guard and whole.numel() - off - nbytes >= guard
    assert np.all(whole.numpy() == q4_guard.POISON_U8)
    q4_guard.check_guards(whole, view)  # a byte interior may keep its poison (fragment padding)
    view.zero_()
    q4_guard.check_guards(whole, view)
    for idx, pattern in ((off + nbytes, "past the end.*first at byte 3072, last at byte 3072"),
                         (whole.numel() - 1, "past the end"), (off - 1, "before the start.*first at byte -1"),
                         (0, "before the start")):
        whole[idx] = 0x5B
        with pytest.raises(AssertionError, match=pattern):
            q4_guard.check_guards(whole, view)
        whole[idx] = q4_guard.POISON_U8
        q4_guard.check_guards(whole, view)
