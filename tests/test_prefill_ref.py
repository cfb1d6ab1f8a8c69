"""The bound the prefill attention kernels are held to (the encoder
self-attention's, attn_ref.sdpa_ref with pair=True and the causal / pad
visibility) has teeth for them, on the CPU: a numpy emulation of the kernel
(prefill_ref.py) stays at or under half the bound on the planted cases of
test_prefill_attn_gpu.py's generator, and planted mistakes -- a causal mask off
by one, a pad key visible, a dropped last key tile -- exceed it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import attn_ref as A
import prefill_ref as PR
from test_prefill_attn_gpu import H, planted

NS = {"f16x2": 2, "f16": 1}
SELF = [(70, 0), (90, 23), (5, 1), (65, 0)]  # (P, pad): one and two key tiles, a padded clip, a short one
CROSS = [(20, 203), (17, 37), (33, 65)]      # (P, T)


@functools.lru_cache(maxsize=None)
def self_inputs(P, pad, prec):
    n = P - pad
    rng = np.random.default_rng(P + pad)
    junk = lambda: (3.0 * rng.standard_normal((pad, 64))).astype(np.float32)  # the pad rows: no real row may see them
    out = []
    for h in range(H):
        q, k, v, names = planted(n, n, 900 + 10 * P + h, h)
        ref, bound = A.sdpa_ref(q, k, v, prec, True, np.tril(np.ones((n, n), bool)))
        out.append((np.concatenate([junk(), q]), np.concatenate([junk(), k]), np.concatenate([junk(), v]), ref, bound))
    return out


def self_ratio(P, pad, prec, mistake=None):
    return max(float((np.abs(PR.self_emulate(q, k, v, pad, NS[prec], mistake) - ref) / bound).max())
               for q, k, v, ref, bound in self_inputs(P, pad, prec))


@functools.lru_cache(maxsize=None)
def cross_inputs(P, T, prec):
    out = []
    for h in range(H):
        q, k, v, _ = planted(P, T, 700 + P + T + h, h)
        out.append((q, k, v) + A.sdpa_ref(q, k, v, prec, True))
    return out


def cross_ratio(P, T, prec, mistake=None):
    return max(float((np.abs(PR.cross_emulate(q, k, v, NS[prec], mistake) - ref) / bound).max())
               for q, k, v, ref, bound in cross_inputs(P, T, prec))


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("P,pad", SELF)
def test_self_emulation_within_half_the_bound(P, pad, prec):
    r = self_ratio(P, pad, prec)
    print(f"prefill self P{P} pad{pad} {prec}: worst error / bound {r:.3f}")
    assert r <= 0.5, r


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("P,T", CROSS)
def test_cross_emulation_within_half_the_bound(P, T, prec):
    r = cross_ratio(P, T, prec)
    print(f"prefill cross P{P} T{T} {prec}: worst error / bound {r:.3f}")
    assert r <= 0.5, r


@pytest.mark.parametrize("prec", A.PRECS)
def test_planted_mistakes_exceed_the_bound(prec):
    assert self_ratio(70, 0, prec, "mask_off_by_one") > 1.0
    assert self_ratio(90, 23, prec, "mask_off_by_one") > 1.0
    assert self_ratio(90, 23, prec, "pad_visible") > 1.0
    assert self_ratio(70, 0, prec, "drop_last_tile") > 1.0  # 70 keys: the second tile's six
    assert self_ratio(90, 23, prec, "drop_last_tile") > 1.0
    assert cross_ratio(20, 203, prec, "drop_last_tile") > 1.0
    assert cross_ratio(33, 65, prec, "drop_last_tile") > 1.0  # 65 keys: the second tile's one
    assert self_ratio(70, 0, prec, "pad_visible") == self_ratio(70, 0, prec)  # no pad: nothing to see
