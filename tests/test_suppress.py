"""Suppress-token lists (wa_model_set_suppress): what can be tested without a
GPU -- the exports, the host-only validity rule against suppress_ref.py, and
the pre-masking step composed with the timestamp rules' reference.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import suppress_ref as sr
import ts_rules as tr
import whisper_amd

EINVAL = 1
TS0 = 50365  # Large-V3 / TINY_TEST
V = 51866
EOT = 50257

NEW = ("wa_suppress_check", "wa_model_set_suppress", "wa_model_suppress_ids", "wa_logits_pick_check",
       "wa_row_pick_check", "wa_beam_topk_check")


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    L = whisper_amd.lib()
    assert hasattr(L, name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def test_python_surface():
    assert callable(whisper_amd.WhisperModel.set_suppress_tokens)
    assert isinstance(whisper_amd.WhisperModel.suppress_tokens, property)
    for n in ("suppress_check", "logits_suppress_check", "row_suppress_check", "beam_topk_suppress_check"):
        assert callable(getattr(whisper_amd, n))


def c_check(always, first, ts0=TS0):
    i32p = ctypes.POINTER(ctypes.c_int32)
    a, f = np.asarray(always, np.int32), np.asarray(first, np.int32)
    return whisper_amd.lib().wa_suppress_check(a.ctypes.data_as(i32p) if a.size else None, int(a.size),
                                               f.ctypes.data_as(i32p) if f.size else None, int(f.size), ts0)


ALL_TEXT = list(range(EOT))
CASES = [
    # (always, first, accepted)
    ([], [], True),
    ([1, 7, 50256] + sr.SPECIALS, [220, EOT], True),  # OpenAI's shape: EOT in `first` is accepted
    ([5, 5, 5, 9, 9], [220, 220, EOT, EOT], True),  # duplicates
    ([0, EOT - 1, EOT + 1, TS0 - 1], [0, TS0 - 1], True),  # every boundary of the allowed ranges
    ([3, EOT], [], False),  # EOT in `always`
    ([TS0], [], False),  # an id >= ts0
    ([], [TS0], False),
    ([V - 1], [], False),
    ([-1], [], False),  # a negative id
    ([], [-1], False),
    (ALL_TEXT[:EOT - 15], [], False),  # only 15 text ids left
    (ALL_TEXT[:EOT - 20], ALL_TEXT[EOT - 20:EOT - 15], False),  # 15 left, through the union
    (ALL_TEXT[:EOT - 16], [], True),  # exactly 16 left
    (ALL_TEXT[:EOT - 16] + ALL_TEXT[:100], [EOT] + sr.SPECIALS, True),  # duplicates and specials count for nothing
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_suppress_check_matches_reference(case):
    always, first, accepted = CASES[case]
    assert sr.valid(always, first, TS0) == accepted
    st = c_check(always, first)
    assert (st == 0) == accepted and st in (0, EINVAL)
    assert whisper_amd.suppress_check(always, first, TS0) == accepted


def test_suppress_check_arguments():
    L = whisper_amd.lib()
    assert c_check([1], [], ts0=EOT) == EINVAL  # ts0 must lie above EOT
    assert c_check([TS0 - 1], [], ts0=TS0 - 1) == EINVAL  # the bound is the caller's ts0 (Medium: 50364)
    assert L.wa_suppress_check(None, 1, None, 0, TS0) == EINVAL  # a count without ids
    assert L.wa_suppress_check(None, -1, None, 0, TS0) == EINVAL
    # a null model: nothing to set, nothing to read
    assert L.wa_model_set_suppress(None, None, 0, None, 0) == EINVAL
    n = ctypes.c_int(7)
    assert L.wa_model_suppress_ids(None, 0, None, 0, ctypes.byref(n)) == EINVAL


def test_random_lists_match_reference():
    rng = np.random.default_rng(5)
    pool = [-1, 0, 1, 31, 32, EOT - 1, EOT, EOT + 1, TS0 - 1, TS0, V - 1, 220, 1000]
    seen = set()
    for _ in range(200):
        a = [int(x) for x in rng.choice(pool, int(rng.integers(0, 4)))]
        f = [int(x) for x in rng.choice(pool, int(rng.integers(0, 4)))]
        want = sr.valid(a, f, TS0)
        seen.add(want)
        assert (c_check(a, f) == 0) == want, (a, f)
    assert seen == {True, False}


def test_premask_composes_with_rule_f():
    """Text A = 16 is the best text logit; 200 timestamps at 8 have logsumexp
    13.3.  Without the list the rule does not fire and A wins; with A
    suppressed the best text logit is 8 and rule f fires: a timestamp wins."""
    A, NEXT = 1000, 2000
    z = np.full(V, -4.0)
    z[A], z[NEXT] = 16.0, 8.0
    z[TS0 + 400:TS0 + 600] = 8.0
    hist = [TS0 + 10, A]  # text after a timestamp: text, or a later timestamp
    zc, fired, _ = tr.apply_rules(z, hist, TS0, False)
    assert not fired and tr.pick(zc) == A
    zm = sr.premask(z, [A])
    assert zm[A] == -np.inf and z[A] == 16.0 and zm.dtype == z.dtype  # a copy
    zs, fired, margin = tr.apply_rules(zm, hist, TS0, False)
    assert fired and margin > 1.0
    assert tr.pick(zs) == TS0 + 599 and not np.isfinite(zs[:TS0]).any()
    # the union of pick 0 and a 2-D row block
    assert sr.union([1, 2], [3]) == [1, 2, 3]
    blk = sr.premask(np.zeros((2, 8), np.float32), [0, 7])
    assert blk.dtype == np.float32 and np.isinf(blk[:, [0, 7]]).all() and (blk[:, 1:7] == 0).all()
