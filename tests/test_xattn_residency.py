"""Host rule of the encoder planes' Infinity Cache residency (wa_xattn.hip
xattn_residency / wa_kernels.hpp xattn_chunk_resident, through
wa_xattn_resident_share / wa_xattn_chunk_resident; no GPU): which 64ths of
every clip's 16-frame sub-chunks the cross-attention loads with the default
cache policy when the planes of all concurrently decoding clips exceed what
the cache keeps."""
from __future__ import annotations

import pytest

import whisper_amd

DEN = whisper_amd.XATTN_SHARE_DEN
LARGE = dict(T=1500, planes=2, D=1280)  # Large-V3, f16x2: 7.68 MB of planes per clip


def live_bytes(clips, T, planes, D):
    return clips * T * planes * D * 2


def resident_bytes(clips, T, planes, D, q):
    frames = sum(min(16, T - 16 * c) for c in range((T + 15) // 16) if whisper_amd.xattn_chunk_resident(c, q))
    return clips * frames * planes * D * 2


@pytest.fixture(autouse=True)
def no_override(monkeypatch):
    monkeypatch.delenv("WA_XATTN_RESIDENT_MB", raising=False)


@pytest.mark.parametrize("budget_mb", [0.5, 50.0, 196.6, 300.0])
def test_everything_resident_when_the_planes_fit(budget_mb):
    for clips in range(1, 130):
        q = whisper_amd.xattn_resident_share(clips, budget_mb=budget_mb, **LARGE)
        fits = live_bytes(clips, **LARGE) <= budget_mb * 1e6
        assert (q == DEN) == fits, (clips, q)


def test_default_rule_keeps_todays_shapes_resident_and_bounds_a_pair():
    # up to 32 Large-V3 clips (245.8 MB) everything loads as before; a pair of
    # 32-clip batches (491.5 MB) keeps a strict part
    for clips in range(1, 33):
        assert whisper_amd.xattn_resident_share(clips, **LARGE) == DEN
    q = whisper_amd.xattn_resident_share(64, **LARGE)
    assert 0 < q < DEN
    # other models derive their share from the same byte budget: tiny planes always fit
    assert whisper_amd.xattn_resident_share(64, 1500, 2, 384) == DEN


@pytest.mark.parametrize("budget_mb", [-1.0, 0.0, 10.0, 196.6])
def test_share_is_monotone_and_within_budget(budget_mb):
    last = DEN
    for clips in range(1, 200):
        q = whisper_amd.xattn_resident_share(clips, budget_mb=budget_mb, **LARGE)
        assert 0 <= q <= last, (clips, q, last)
        last = q
        if budget_mb >= 0 and q < DEN:
            assert resident_bytes(clips, q=q, **LARGE) <= budget_mb * 1e6


def test_default_budget_bounds_resident_bytes():
    q = whisper_amd.xattn_resident_share(64, **LARGE)
    q1 = whisper_amd.xattn_resident_share(64, budget_mb=172.0, **LARGE)
    assert q == q1 == 22
    assert resident_bytes(64, q=q, **LARGE) <= 172.0e6


def test_environment_override(monkeypatch):
    monkeypatch.setenv("WA_XATTN_RESIDENT_MB", "0")
    assert whisper_amd.xattn_resident_share(1, **LARGE) == 0
    monkeypatch.setenv("WA_XATTN_RESIDENT_MB", "1000000")
    assert whisper_amd.xattn_resident_share(128, **LARGE) == DEN
    monkeypatch.setenv("WA_XATTN_RESIDENT_MB", "123")  # a quarter of a pair's 491.5 MB of planes
    assert whisper_amd.xattn_resident_share(64, **LARGE) == DEN // 4


@pytest.mark.parametrize("T", [1500, 100])
def test_every_walk_has_the_same_mix(T):
    """A (row, split) workgroup walks `ch` consecutive sub-chunks (the last
    split of T = 1500 only 10 of 12, so equal counts are not possible across
    all walks at large shares): every walk of n sub-chunks holds floor or
    ceil(n q / 64) resident ones, hence walks of equal length differ by at
    most one."""
    splits, ch = whisper_amd.xattn_plan(T)
    nchunk = (T + 15) // 16
    assert (splits, ch) == ((8, 12) if T == 1500 else (7, 1))
    for q in range(DEN + 1):
        res = [whisper_amd.xattn_chunk_resident(c, q) for c in range(nchunk)]
        assert sum(res) == nchunk * q // DEN
        by_len = {}
        for s in range(splits):
            walk = res[s * ch:min(nchunk, (s + 1) * ch)]
            n, k = len(walk), sum(walk)
            assert n * q // DEN <= k <= -(-n * q // DEN), (T, q, s, k)
            by_len.setdefault(n, []).append(k)
        for ks in by_len.values():
            assert max(ks) - min(ks) <= 1


def test_bad_arguments():
    with pytest.raises(ValueError):
        whisper_amd.xattn_resident_share(0, **LARGE)
    with pytest.raises(ValueError):
        whisper_amd.xattn_chunk_resident(3, DEN + 1)
