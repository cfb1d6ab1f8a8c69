"""Timestamp decoding (wa_transcribe_timestamps): what can be tested without a
GPU -- the exports, the argument checks that precede every device call, the
host-only segment slicing and rule record, and the numpy restatement of the
rules (ts_rules.py) that the GPU tests lean on.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import ts_rules as tr
import whisper_amd
import wq4

EINVAL = 1
TS0 = 50365  # Large-V3 / TINY_TEST
TS0_MEDIUM = 50364
V = 51866
EOT = 50257

NEW = ("wa_transcribe_timestamps", "wa_transcribe_batches_timestamps", "wa_segments_from_tokens",
       "wa_timestamp_rule", "wa_logits_pick_check", "wa_row_pick_check", "wa_timestamp_bookkeep_check")


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    L = whisper_amd.lib()
    assert hasattr(L, name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def test_python_surface():
    for n in ("transcribe_timestamps", "transcribe_batches_timestamps"):
        assert callable(getattr(whisper_amd.WhisperModel, n))
    assert callable(whisper_amd.segments_from_tokens)


def test_transcribe_timestamps_rejects_bad_arguments():
    L = whisper_amd.lib()
    model, mel = (ctypes.c_uint8 * 4096)(), (ctypes.c_float * 16)()
    tok, nt = (ctypes.c_int32 * 1024)(), (ctypes.c_int32 * 16)()
    addr = lambda b: ctypes.c_void_p(ctypes.addressof(b))
    f, g = L.wa_transcribe_timestamps, L.wa_transcribe_batches_timestamps
    assert f(None, addr(mel), 1, 50259, 8, 1, 50, tok, nt, None, None) == EINVAL
    assert "null" in L.wa_last_error().decode()
    assert f(addr(model), addr(mel), 1, 50259, 225, 1, 50, tok, nt, None, None) == EINVAL
    assert "max_tokens" in L.wa_last_error().decode()
    assert g(None, addr(mel), 2, 1, 50259, 8, 1, 50, tok, nt, None, None) == EINVAL
    assert g(addr(model), addr(mel), 2, 1, 50259, 0, 1, 50, tok, nt, None, None) == EINVAL
    assert "max_tokens" in L.wa_last_error().decode()


# ----------------------------------------------------------------- segments --
def ts(sec, ts0=TS0):
    return ts0 + int(round(sec / 0.02))


A, B_, C = 400, 500, 600  # text ids


def f32(x):
    return float(np.float32(x))


SEGMENT_CASES = {
    "empty": ([], TS0, [], 3000),
    "text only": ([A, B_, C], TS0, [(0.0, 30.0, [A, B_, C])], 3000),
    # <0.0> a b <2.0>: no cut; the last timestamp is nonzero, so the segment ends there
    "one open pair": ([ts(0), A, B_, ts(2.0)], TS0, [(0.0, f32(100 * 0.02), [ts(0), A, B_, ts(2.0)])], 3000),
    "only <0.00>": ([ts(0), A], TS0, [(0.0, 30.0, [ts(0), A])], 3000),
    "two full pairs": ([ts(0), A, ts(1.5), ts(1.5), B_, C, ts(4.0), ts(4.0)], TS0,
                       [(0.0, f32(75 * 0.02), [ts(0), A, ts(1.5)]),
                        (f32(75 * 0.02), f32(200 * 0.02), [ts(1.5), B_, C, ts(4.0)])], 400),
    # the tail <t> a b is dropped: the next window re-decodes it from seek_frames
    "pairs then open tail": ([ts(0), A, ts(1.0), ts(1.0), B_, ts(2.5), ts(2.5), A, B_], TS0,
                             [(0.0, f32(50 * 0.02), [ts(0), A, ts(1.0)]),
                              (f32(50 * 0.02), f32(125 * 0.02), [ts(1.0), B_, ts(2.5)])], 250),
    # single_end: the window is consumed whole
    "pairs then single end": ([ts(0), A, ts(1.0), ts(1.0), B_, ts(2.5)], TS0,
                              [(0.0, f32(50 * 0.02), [ts(0), A, ts(1.0)]),
                               (f32(50 * 0.02), f32(125 * 0.02), [ts(1.0), B_, ts(2.5)])], 3000),
    "ends <t><t>": ([ts(0.5), A, ts(3.0), ts(3.0)], TS0, [(f32(25 * 0.02), f32(150 * 0.02), [ts(0.5), A, ts(3.0)])],
                    300),
    "ids at ts0 + 1500": ([ts(0), A, TS0 + 1500, TS0 + 1500], TS0, [(0.0, 30.0, [ts(0), A, TS0 + 1500])], 3000),
    "medium": ([TS0_MEDIUM, A, TS0_MEDIUM + 100, TS0_MEDIUM + 100], TS0_MEDIUM,
               [(0.0, f32(100 * 0.02), [TS0_MEDIUM, A, TS0_MEDIUM + 100])], 200),
    # the same ids under Large-V3's ts0 are one unit later, and 50364 is NO_TIMESTAMPS, a non-timestamp
    "medium ids, large ts0": ([TS0_MEDIUM, A, TS0_MEDIUM + 100, TS0_MEDIUM + 100], TS0,
                              [(f32(-0.02), f32(99 * 0.02), [TS0_MEDIUM, A, TS0_MEDIUM + 100])], 198),
}


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segments_from_tokens(name):
    tokens, ts0, want, seek = SEGMENT_CASES[name]
    got, got_seek = whisper_amd.segments_from_tokens(tokens, ts0)
    assert got_seek == seek
    assert len(got) == len(want), got
    for (s, e, t), (ws, we, wt) in zip(got, want):
        assert t == wt
        assert abs(s - ws) <= 1e-6 and abs(e - we) <= 1e-6, (got, want)


def test_segments_cap_too_small():
    tokens, ts0, want, _ = SEGMENT_CASES["two full pairs"]
    L = whisper_amd.lib()
    arr = np.asarray(tokens, np.int32)
    segs = (whisper_amd.Segment * 1)()
    n, seek = ctypes.c_int(-1), ctypes.c_int(-1)
    st = L.wa_segments_from_tokens(arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), arr.size, ts0, segs, 1,
                                   ctypes.byref(n), ctypes.byref(seek))
    assert st == EINVAL and n.value == len(want) == 2
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.segments_from_tokens(tokens, ts0, cap=1)
    got, _ = whisper_amd.segments_from_tokens(tokens, ts0, cap=2)
    assert len(got) == 2


# ------------------------------------------------ the numpy rule, by hand --
def allowed(s, suppress_eot=False, max_initial=50, ts0=TS0):
    z = tr.masks_ae(np.zeros(V), s, ts0, suppress_eot, max_initial)
    return np.isfinite(z)


def ranges(*spans):
    ok = np.zeros(V, bool)
    for lo, hi in spans:  # inclusive
        ok[lo:hi + 1] = True
    return ok


T1, T2 = TS0 + 40, TS0 + 90

HAND_MASKS = [
    # (history, suppress_eot, max_initial, allowed id ranges, inclusive)
    ([], True, 50, [(TS0, TS0 + 50)]),  # e: the first pick
    ([], True, -1, [(TS0, V - 1)]),  # e without an upper bound
    ([], True, 0, [(TS0, TS0)]),
    ([T1], True, 50, [(0, EOT - 1)]),  # last & penult (len < 2): text only, EOT suppressed at step 0
    ([T1], False, 50, [(0, EOT)]),
    ([T1, A], False, 50, [(0, EOT), (T1 + 1, V - 1)]),  # text after a timestamp: strictly later timestamps
    ([T1, A, B_], False, 50, [(0, EOT), (T1 + 1, V - 1)]),
    ([T1, A, T2], False, 50, [(EOT, EOT), (T2, V - 1)]),  # last & !penult: EOT or a timestamp >= the last
    ([T1, A, T2], True, 50, [(T2, V - 1)]),
    ([T1, A, T2, T2], False, 50, [(0, EOT)]),  # a closed pair: text, no timestamp
    ([T1, A, T2, T2, C], False, 50, [(0, EOT), (T2 + 1, V - 1)]),
    ([A], False, 50, [(0, EOT), (TS0, V - 1)]),  # no timestamp yet (a history the first pick never produces)
    ([T1, A, V - 1], False, 50, [(EOT, EOT), (V - 1, V - 1)]),
    ([T1, A, V - 1, V - 1, A], False, 50, [(0, EOT)]),  # nothing later than <|30.00|>
]


@pytest.mark.parametrize("case", range(len(HAND_MASKS)))
def test_numpy_masks_by_hand(case):
    s, sup, mi, spans = HAND_MASKS[case]
    assert np.array_equal(allowed(s, sup, mi), ranges(*spans))


def test_numpy_mass_rule_and_pick_by_hand():
    s = [T1, A]  # text and timestamps > T1 allowed
    z = np.full(V, -20.0)
    z[A] = 5.0
    z[T2:T2 + 200] = 2.0  # lse = 2 + log 200 = 7.30 > 5: text masked, no single timestamp beats z[A]
    z[T1 - 3] = 9.0  # masked by d: must not count
    z[50300] = 50.0  # a special: masked by b
    out, fired, margin = tr.apply_rules(z, s, TS0, False)
    assert fired and not np.isfinite(out[:TS0]).any()
    assert tr.pick(out) == T2 + 199  # equal maxima: the largest index
    assert abs(margin - (tr.lse(out[TS0:]) - 5.0)) < 1e-12  # the mass margin; the 200 equal maxima are one value
    z[T2:T2 + 200] = -1.0  # lse = -1 + log 200 = 4.30 (+ the -20 floor) < 5
    out, fired, margin = tr.apply_rules(z, s, TS0, False)
    assert not fired and tr.pick(out) == A
    assert abs(margin - (5.0 - tr.lse(out[TS0:]))) < 1e-12


def test_numpy_allowed_set_never_empty():
    rng = np.random.default_rng(0)
    for _ in range(300):
        n = int(rng.integers(0, 7))
        s = [int(rng.choice([A, EOT, TS0, T1, T2, V - 1, int(rng.integers(0, V))])) for _ in range(n)]
        for sup in (False, True):
            assert allowed(s, sup).any(), s


# --------------------------------------- the product's record, on the host --
@pytest.mark.parametrize("ts0,vocab", [(TS0, V), (TS0_MEDIUM, V - 1)])
def test_rule_record_matches_numpy(ts0, vocab):
    """wa_timestamp_rule (the C++ statement the bookkeeping kernel shares)
    against the record and the masks restated from the history in numpy."""
    rng = np.random.default_rng(ts0)
    pool = [A, B_, EOT, ts0, ts0 + 1, ts0 + 40, ts0 + 90, vocab - 1, ts0 - 1, 50300]
    hist = [[], [ts0 + 1500], [A], [ts0, ts0], [ts0, A, vocab - 1], [ts0, A, vocab - 1, vocab - 1]]
    hist += [[int(rng.choice(pool)) for _ in range(int(rng.integers(1, 9)))] for _ in range(200)]
    for s in hist:
        for mi in (50, 0, -1):
            got = whisper_amd.timestamp_rule(s, ts0, vocab, mi)
            assert got.tolist() == tr.record(s, ts0, vocab, mi), (s, mi)
            for sup in (False, True):
                z = tr.masks_ae(np.zeros(vocab), s, ts0, sup, mi)
                assert np.array_equal(tr.allowed_from_record(got, ts0, vocab, sup), np.isfinite(z)), (s, mi, sup)


# ------------------------------- the GPU tests' planted rows, reference only --
@pytest.mark.parametrize("D", [128, 384])
def test_planted_rows_own_their_branches(D):
    """The float64 reference of test_timestamps_gpu.py's planted rows, without
    a kernel: every row's winner is the intended one, the mass rule fires and
    holds where planned, and every row decides with >= 100 x the logit bound."""
    import test_timestamps_gpu as g

    _, _, ref, hist = g.planted_host(D)
    for step in (g.STEP, 0):
        want, wtok, wfired, margins = g.rule_rows(ref, hist, 32, step)
        assert (margins >= 100 * (4e-6 * np.abs(ref).max(axis=1) + 1e-6)).all(), margins
        if step == g.STEP:
            assert [int(t) for t in wtok[:len(g.PLANTS)]] == [p[2] for p in g.PLANTS]
            assert wfired[6] and not wfired[7] and not wfired[2]
    assert ref[0].argmax() == g.A and ref[8].argmax() == 50300 and ref[10].argmax() == g.TS0 - 1
    assert ref[6, g.T(100):g.T(300)].max() < ref[6, g.A]  # no single timestamp beats the text
    assert ref[9, g.T(800)] == ref[9, g.T(900)]
