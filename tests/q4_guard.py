"""Guard bands around the outputs of the Q4 kernels (used by
test_q4_guard_gpu.py on the GPU and self-tested on the CPU in
test_q4_routing.py; no GPU import at module level: `torch` is handed in).

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

import numpy as np

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
