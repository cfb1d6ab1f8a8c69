"""Host rule of the cross-attention's frame split (wa_xattn.hip xattn_plan,
through wa_xattn_plan_splits; no GPU): a decode whose largest concurrently
decoding group has `rows` rows, and whose launches may take free_cus CUs (what
the masked encoder stream and the decode's other groups leave), gets the most
splits S <= 8 with S * rows <= free_cus (at least one), normalised so that no
split is empty -- xattn_main holds a CU to itself and its workgroups last the
whole launch, so whatever else needs one of S * rows CUs waits for it.  With
every CU free and 8 splits fitting, the plan is the one the kernel always
had."""
from __future__ import annotations

import pytest

import whisper_amd

KTC, SMAX = 16, 8  # frames per sub-chunk, most splits


def nchunks(T):
    return (T + KTC - 1) // KTC


def normalised(T, S):
    n = nchunks(T)
    S = max(1, min(S, SMAX, n))
    ch = -(-n // S)
    return -(-n // ch), ch


@pytest.fixture(autouse=True)
def no_override(monkeypatch):
    monkeypatch.delenv("WA_XATTN_SPLITS_RT", raising=False)


def test_all_cus_free_is_todays_plan():
    for T in range(1, 1537):
        today = normalised(T, SMAX)
        assert whisper_amd.xattn_plan(T) == today
        for rows in range(1, 65):
            if rows * SMAX <= 256:
                assert whisper_amd.xattn_plan_splits(T, rows, 256) == today, (T, rows)
            assert whisper_amd.xattn_plan_splits(T, rows, 0) == today, (T, rows)  # nothing beside the decode


@pytest.mark.parametrize("T", [1, 16, 17, 37, 100, 200, 1000, 1499, 1500, 1536])
def test_fits_free_cus_no_empty_split_monotone(T):
    n = nchunks(T)
    for rows in range(1, 65):
        last = 0
        for free in range(1, 321):
            splits, ch = whisper_amd.xattn_plan_splits(T, rows, free)
            assert 1 <= splits <= SMAX and ch >= 1
            if rows <= free:
                assert splits * rows <= free, (T, rows, free, splits)
            assert (splits - 1) * ch < n <= splits * ch, (T, rows, free, splits, ch)
            assert (splits, ch) == normalised(T, max(1, free // rows))
            assert splits >= last, (T, rows, free)
            last = splits


def test_bench_shape():
    assert whisper_amd.xattn_plan_splits(1500, 32, 256) == (8, 12)
    assert whisper_amd.xattn_plan_splits(1500, 32, 224) == (7, 14)
    assert whisper_amd.xattn_plan_splits(1500, 32, 208) == (6, 16)
    assert whisper_amd.xattn_plan_splits(1500, 32, 192) == (6, 16)
    assert whisper_amd.xattn_plan_splits(1500, 32, 160) == (5, 19)  # a 32-row pair beside the 32-CU masked stream
    assert whisper_amd.xattn_plan_splits(1500, 16, 160) == (8, 12)  # 16-row groups keep 8


def test_override_is_not_part_of_the_rule(monkeypatch):
    monkeypatch.setenv("WA_XATTN_SPLITS_RT", "3")
    assert whisper_amd.xattn_plan_splits(1500, 32, 224) == (7, 14)
    assert whisper_amd.xattn_plan(1500) == (8, 12)


def test_bad_arguments():
    import wq4

    with pytest.raises(wq4.WQ4Error):
        whisper_amd.xattn_plan_splits(0, 1, 256)
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.xattn_plan_splits(1500, 0, 256)
