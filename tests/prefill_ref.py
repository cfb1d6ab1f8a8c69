"""A numpy emulation of prefill_attention_kernel, for the CPU test of the
bound it is held to (test_prefill_ref.py).

The kernel runs the encoder kernel's arithmetic, which attn_ref.encoder_emulate
restates (f16-pair operands at the kernel's scales, 32-key sub-tiles, the lazy
reference maximum).  A causal row t of a clip whose keys start at slot pad
sees keys [pad, t]: the keys past t enter its sub-tiles as exact zeros of p and
the sub-tiles wholly past t are skipped, so the row is the emulation over
k[pad : t + 1] alone.  The kernel's compensated sums over the sub-tiles are
not modelled: the emulation adds them as the encoder's does, which is the
larger error.  `mistake` plants what the bound has to catch:
  mask_off_by_one  row t also sees key t + 1
  pad_visible      row t also sees the pad row before its clip's first key
  drop_last_tile   the last 64-key tile of the row's keys is left out
"""
from __future__ import annotations

import numpy as np

import attn_ref as A


def self_emulate(q, k, v, pad, ns=2, mistake=None):
    """q, k, v [P, 64] of one (clip, head), rows [pad, P) real -> [P - pad, 64]."""
    P = q.shape[0]
    out = np.zeros((P - pad, 64))
    for t in range(pad, P):
        lo, hi = pad, t + 1
        if mistake == "mask_off_by_one":
            hi = min(P, hi + 1)
        elif mistake == "pad_visible":
            lo = max(0, lo - 1)
        elif mistake == "drop_last_tile" and hi - lo > 64:
            hi = lo + (hi - lo - 1) // 64 * 64
        out[t - pad] = A.encoder_emulate(q[t:t + 1], k[lo:hi], v[lo:hi], ns)[0]
    return out


def cross_emulate(q, k, v, ns=2, mistake=None):
    """q [P, 64], k, v [T, 64] -> [P, 64]."""
    T = k.shape[0]
    if mistake == "drop_last_tile" and T > 64:
        T = (T - 1) // 64 * 64
    return A.encoder_emulate(q, k[:T], v[:T], ns)
