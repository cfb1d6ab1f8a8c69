"""The decode step graph's key (wa_model.hpp graph_key, through
wa_decode_graph_key_check; no GPU): a mixed-radix number over everything a
captured step bakes in.  Its layout is a contract -- the GPU tests read the
plane residency as key % 65 and the frame split as key // 65 % 16, and a group
keeps graphs of several layouts apart by it -- so it is restated here as the
formula the key was first written as, with literal radices, and compared
exactly.  A digit outside its radix would alias another layout's key: -1."""
from __future__ import annotations

import random

import pytest

import whisper_amd

# most significant first, as wa_decode_graph_key_check takes them
NAMES = ("mode", "lane", "b0", "nb", "eot", "trace", "group_kv", "range_tier", "splits", "residency")
RADIX = (8, 3, 512, 512, 2, 2, 2, 4, 16, 65)


def parent_key(mode, lane, b0, nb, eot, trace, group_kv, range_tier, splits, q):
    """The hand-written number: the layout digits, and the three mode bits as
    multiples of the product of every radix below them."""
    score, ts, sample = mode & 1, mode >> 1 & 1, mode >> 2 & 1
    base = ((((((((lane * 512 + b0) * 512 + nb) * 2 + eot) * 2 + trace) * 2 + group_kv) * 4 + range_tier) * 16
             + splits) * 65 + q)
    top = 3 * 512 * 512 * 2 * 2 * 2 * 4 * 16 * 65
    return base + (top if score else 0) + (2 * top if ts else 0) + (4 * top if sample else 0)


def test_exported_declared_and_radices_are_the_products():
    assert hasattr(whisper_amd.lib(), "wa_decode_graph_key_check")
    assert "wa_decode_graph_key_check" in open(whisper_amd.CHECKS_HEADER_PATH).read()
    assert whisper_amd.XATTN_SHARE_DEN + 1 == RADIX[-1]


@pytest.mark.parametrize("others", ["zero", "max"])
@pytest.mark.parametrize("i", range(len(RADIX)), ids=NAMES)
def test_every_digit_at_its_ends(i, others):
    for v in (0, RADIX[i] - 1):
        d = [0 if others == "zero" else r - 1 for r in RADIX]
        d[i] = v
        assert whisper_amd.decode_graph_key_check(*d) == parent_key(*d), d


def test_random_tuples_and_the_digits_the_gpu_tests_read():
    rng = random.Random(20240611)
    for _ in range(1000):
        d = [rng.randrange(r) for r in RADIX]
        key = whisper_amd.decode_graph_key_check(*d)
        assert key == parent_key(*d), d
        assert key % 65 == d[9]  # the plane residency (test_xattn_residency_gpu.py)
        assert key // 65 % 16 == d[8]  # the frame split's splits (plan_child.py)


@pytest.mark.parametrize("i", range(len(RADIX)), ids=NAMES)
def test_a_digit_outside_its_radix_is_an_error(i):
    for others in (0, 1):
        d = [others] * len(RADIX)
        assert whisper_amd.decode_graph_key_check(*d) >= 0
        d[i] = RADIX[i]
        assert whisper_amd.decode_graph_key_check(*d) == -1, d
        d[i] = -1
        assert whisper_amd.decode_graph_key_check(*d) == -1, d


def test_the_eight_modes_have_eight_keys():
    layout = [1, 3, 17, 1, 0, 0, 2, 6, 38]
    keys = {whisper_amd.decode_graph_key_check(mode, *layout) for mode in range(8)}
    assert len(keys) == 8 and -1 not in keys
    # an unscored, unsampled, timestamp-free key is the layout's number alone
    assert whisper_amd.decode_graph_key_check(0, *layout) == parent_key(0, *layout) < 3 * 512 * 512 * 2 * 2 * 2 * 4 * 16 * 65
