"""Guard bands around the outputs of the Q4 kernels (used by
test_q4_guard_gpu.py and test_q4_small_gpu.py on the GPU and self-tested on
the CPU in test_q4_routing.py; no GPU import at module level: `torch` is
handed in), and the guarded GEMM launches those two files share.

An output is carved out of the middle of one larger allocation whose every
element holds a poison pattern.  The kernel gets the interior pointer through
the C ABI; afterwards both guards must still hold the poison bit for bit, and
-- for f32 outputs -- no poison may be left inside the rows x n interior.

Guard-size condition: each guard is at least as large as the farthest write a
wrong kernel of this family could make past its output, so even a failing run
writes only memory the test owns.  The kernels pad rows to at most 256 (the
wide kernel's group of 8 m-tiles of 32 rows), so an f32 guard is G = 256 rows
of n floats and an A-tiled guard is wq4_atiled_bytes(256, n, prec).
"""
from __future__ import annotations

import ctypes

import numpy as np

import oracle
import wq4

vp = ctypes.c_void_p

G = 256                    # guard rows on either side of an f32 output
POISON_F32 = 0x7FC5A5A5    # a quiet NaN no kernel here computes (payload 0x45A5A5)
POISON_U8 = 0x5A
ALIGN = 1024               # A-tiled fragments are 1 KiB


def guarded_f32(torch, rows, n, device="cuda:0"):
    """(whole, view, ptr): `whole` is one f32 tensor of (G + rows + G) * n
    elements, all POISON_F32; `view` its rows x n interior and `ptr` the
    interior's address for the C ABI."""
    whole = torch.full(((2 * G + rows) * n,), POISON_F32, dtype=torch.int32, device=device).view(torch.float32)
    view = whole[G * n:(G + rows) * n].view(rows, n)
    return whole, view, view.data_ptr()


def guarded_bytes(torch, nbytes, guard, device="cuda:0"):
    """(whole, view, ptr): a uint8 allocation filled with POISON_U8 whose
    `nbytes` interior starts on a 1 KiB boundary with at least `guard` bytes
    on either side."""
    whole = torch.full((2 * guard + nbytes + ALIGN,), POISON_U8, dtype=torch.uint8, device=device)
    off = guard + (-(whole.data_ptr() + guard)) % ALIGN
    view = whole[off:off + nbytes]
    assert view.data_ptr() % ALIGN == 0 and off >= guard and whole.numel() - off - nbytes >= guard
    return whole, view, view.data_ptr()


def check_guards(whole, view, rows=None, what=""):
    """Both guards of `whole` around `view` (from guarded_f32 / guarded_bytes)
    are unchanged bit for bit; an f32 interior holds no poison (every element
    was written).  `rows` declares an f32 interior of fewer rows than `view`
    has: the rows from there on count as guard.  An AssertionError names the
    first and last touched element by its row and column relative to the
    interior (rows >= the row count are past the end, negative rows before the
    start), or by its byte offset for a byte buffer."""
    tag = what + ": " if what else ""
    off = view.storage_offset()
    if whole.element_size() == 4:
        n = view.shape[1]
        rows = view.shape[0] if rows is None else rows
        w = whole.cpu().numpy().view(np.int32)  # a copy of the bytes: NaN payloads survive
        size, unit, poison = rows * n, "elements", np.int32(POISON_F32)
    else:
        assert whole.element_size() == 1 and rows is None
        w = whole.cpu().numpy().view(np.uint8)
        size, unit, poison = view.numel(), "bytes", np.uint8(POISON_U8)

    def where(i):  # i: offset from the interior's first element
        return f"row {i // n} column {i % n}" if unit == "elements" else f"byte {i}"

    for name, lo, hi in (("before the start", 0, off), ("past the end", off + size, w.size)):
        t = np.flatnonzero(w[lo:hi] != poison)
        if t.size:
            first, last = int(t[0]) + lo - off, int(t[-1]) + lo - off
            msg = f"{tag}{t.size} guard {unit} written {name} of the output: first at {where(first)}, last at {where(last)}"
            if unit == "elements" and lo:
                msg += f" ({first // n - rows + 1} .. {last // n - rows + 1} rows past the end of {rows} x {n})"
            raise AssertionError(msg)
    if unit == "elements":
        p = np.flatnonzero(w[off:off + size] == poison)
        if p.size:
            raise AssertionError(f"{tag}{p.size} of {rows} x {n} outputs never written: first at {where(int(p[0]))}, "
                                 f"last at {where(int(p[-1]))}")


# ------------------------------------------------- guarded GEMM launches --
def _stream(torch):
    return vp(torch.cuda.current_stream().cuda_stream)


def to_dev(torch, a, shape):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(shape)).to("cuda:0")


def tile_activations(torch, x, m, k, prec):
    """The A-tiled operand of x [m, k] (host f32) on the device."""
    xd = to_dev(torch, x, (m, k))
    L = wq4.lib()
    at = torch.zeros(L.wq4_atiled_bytes(m, k, prec), dtype=torch.uint8, device="cuda:0")
    wq4.check(L.wq4_tile_activations(vp(xd.data_ptr()), m, k, k, prec, vp(at.data_ptr()), at.numel(), _stream(torch)))
    return at


def problem(torch, rng, m, n, k, prec, wscale=0.05):
    """Q4_0 weights [n, k], their dequantized values, activations [m, k] (host
    and A-tiled on the device), a bias and a residual."""
    q = oracle.quantize_convert_np((rng.standard_normal(n * k) * wscale).astype(np.float32))
    deq = oracle.dequantize_np(q, n * k).reshape(n, k)
    t = wq4.Q4Tensor.from_q4_bytes(q, [n, k])
    x = rng.standard_normal(m * k).astype(np.float32).reshape(m, k)
    at = tile_activations(torch, x, m, k, prec)
    bias = (rng.standard_normal(n) * 0.1).astype(np.float32)
    res = rng.standard_normal(m * n).astype(np.float32).reshape(m, n)
    return t, deq, x, at, bias, res


def gemm_guarded(torch, t, at, bias_d, res_d, m, n, flags, inplace, prec, kernel, what):
    """One wq4_gemm_tiled launch into a guarded output; returns the interior
    (f32 [m, n] or the A-tiled bytes) on the host after the guard checks."""
    L = wq4.lib()
    if flags & 4:
        whole, view, ptr = guarded_bytes(torch, L.wq4_atiled_bytes(m, n, prec), L.wq4_atiled_bytes(256, n, prec))
        wq4.check(L.wq4_gemm_tiled(t.handle, vp(bias_d.data_ptr()), vp(at.data_ptr()), None, None, vp(ptr), m, flags,
                                   prec, kernel, _stream(torch)))
    else:
        whole, view, ptr = guarded_f32(torch, m, n)
        rptr = None
        if flags & 2:
            rptr = res_d.data_ptr()
            if inplace:
                view.copy_(res_d)
                rptr = ptr
        wq4.check(L.wq4_gemm_tiled(t.handle, vp(bias_d.data_ptr()), vp(at.data_ptr()), vp(rptr), vp(ptr), None, m,
                                   flags, prec, kernel, _stream(torch)))
    torch.cuda.synchronize()
    check_guards(whole, view, what=what)
    return view.cpu().numpy().copy()


def assert_atiled_equals_tiled_f32(torch, got, y0, rows, n, prec, tile_rows, what):
    """An A-tiled GEMM output `got` (host bytes) is bit-equal to
    wq4_tile_activations of the f32 result y0 [rows, n] over the rows the
    kernel writes: whole tiles of `tile_rows` rows, zero-padded."""
    L = wq4.lib()
    y0d = to_dev(torch, y0, (rows, n))
    want = torch.zeros(got.size, dtype=torch.uint8, device="cuda:0")
    wq4.check(L.wq4_tile_activations(vp(y0d.data_ptr()), rows, n, n, prec, vp(want.data_ptr()), want.numel(),
                                     _stream(torch)))
    torch.cuda.synchronize()
    ns, kbp = 2 - prec, (n // 32 + 1) // 2 * 2
    nmt, kb = -(-rows // 32), n // 32  # the m-tiles and blocks that hold real rows and columns
    # [m-tile][block][kk][split][half h][row r][16 B]: lane = 32 h + r holds row 32 mt + r
    gb = got.reshape(-1, kbp, 2, ns, 2, 32, 16)[:nmt, :kb]
    wb = want.cpu().numpy().reshape(-1, kbp, 2, ns, 2, 32, 16)[:nmt, :kb]
    # rows up to the kernel's own tile height are written, zeros past `rows`
    real = (np.arange(nmt)[:, None] * 32 + np.arange(32)[None, :]) < -(-rows // tile_rows) * tile_rows
    gb, wb = gb.transpose(0, 5, 1, 2, 3, 4, 6)[real], wb.transpose(0, 5, 1, 2, 3, 4, 6)[real]
    assert np.array_equal(gb, wb), what + ": A-tiled output differs from the tiled f32 result"


def small_gemm(torch, rows, n, k, prec, kernel, name, tile_rows):
    """Flags 0, 2 (in place) and -- N % 32 == 0 -- the A-tiled output of one
    small-M kernel: guards untouched, f32 results against float64, the A-tiled
    output bit-equal to wq4_tile_activations of the checked f32 result over
    the rows the kernel writes (whole tiles of `tile_rows` rows, zero-padded)."""
    from test_q4_gpu import assert_q4_close

    rng = np.random.default_rng(rows * 11 + n + k + prec)
    t, deq, x, at, bias, res = problem(torch, rng, rows, n, k, prec)
    bias_d, res_d = to_dev(torch, bias, (n,)), to_dev(torch, res, (rows, n))
    wq4.set_kernel_policy(kernel)
    wq4.set_precision(prec)
    assert wq4.gemm_kernel_name(n, k, rows) == name
    what = f"{name} {(rows, n, k)} prec {prec}"
    y0 = gemm_guarded(torch, t, at, bias_d, res_d, rows, n, 0, False, prec, kernel, what + " flags 0")
    assert_q4_close(y0, x, deq, prec=prec, bias=bias, what=what + " flags 0")
    y2 = gemm_guarded(torch, t, at, bias_d, res_d, rows, n, 2, True, prec, kernel, what + " flags 2")
    assert_q4_close(y2, x, deq, prec=prec, bias=bias, residual=res, what=what + " flags 2")
    if n % 32 == 0:
        got = gemm_guarded(torch, t, at, bias_d, res_d, rows, n, 4, False, prec, kernel, what + " flags 4")
        assert_atiled_equals_tiled_f32(torch, got, y0, rows, n, prec, tile_rows, what + " flags 4")
