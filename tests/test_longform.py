"""Long-form transcription (wa_transcribe_long): what can be tested without a
GPU -- the exports, the host rules wa_long_advance and wa_long_round against
their restatements here (the skip and advance rules and the scheduling rule of
include/whisper_amd.h, written out), and the argument checks that precede
every device call.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import whisper_amd

EINVAL = 1
TS0 = 50365
NAN = float("nan")

NEW = ("wa_long_mel_max", "wa_long_mel_windows", "wa_long_advance", "wa_long_round", "wa_transcribe_long",
       "wa_long_result_free", "wa_long_result_streams", "wa_long_result_max_tokens", "wa_long_result_stream",
       "wa_long_result_windows", "wa_long_result_window", "wa_long_result_segments")


def ts(seconds: float) -> int:
    return TS0 + int(round(seconds / 0.02))


def seek_frames(tokens, ts0=TS0) -> int:
    """wa_segments_from_tokens' seek_frames, restated: the frame of the last
    closed timestamp pair, 3000 without one or after a single ending timestamp."""
    t = list(tokens)
    n = len(t)
    is_ts = [x >= ts0 for x in t]
    single_end = n >= 2 and not is_ts[n - 2] and is_ts[n - 1]
    cuts = [i for i in range(1, n) if is_ts[i - 1] and is_ts[i]]
    if not cuts or single_end:
        return 3000
    return (t[cuts[-1] - 1] - ts0) * 2


def advance_rule(tokens, size, ns, avg, lp_thr, ns_thr, ts0=TS0):
    """Steps 3-4 of the loop: (skipped, advance)."""
    rescued = not math.isnan(lp_thr) and avg > float(np.float32(lp_thr))
    skip = not math.isnan(ns_thr) and np.float32(ns) > np.float32(ns_thr) and not rescued
    if skip:
        return True, size
    adv = min(seek_frames(tokens, ts0), size)
    return False, adv if adv >= 1 else size


def round_rule(content, seek, windows, max_batch, max_windows):
    return [r for r in range(len(content)) if seek[r] < content[r] and windows[r] < max_windows][:max_batch]


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    assert hasattr(whisper_amd.lib(), name)
    assert name in open(whisper_amd.HEADER_PATH).read()


def test_python_surface():
    assert callable(whisper_amd.WhisperModel.transcribe_long)
    for n in ("long_mel_max", "long_mel_windows", "long_advance", "long_round"):
        assert callable(getattr(whisper_amd, n))
    assert [f[0] for f in whisper_amd.LongOptions._fields_] == [
        "max_tokens", "max_windows", "lang_token", "max_initial", "temperatures", "n_temperatures",
        "logprob_threshold", "no_speech_threshold", "seed"]
    assert ctypes.sizeof(whisper_amd.LongWindow) == 56 and ctypes.sizeof(whisper_amd.LongSegment) == 32


CUT = [ts(0.0), 7, 8, ts(2.5), ts(2.5), 9, ts(6.2), ts(6.2), 11, 12]  # closed pairs, then open text
CUT_CLOSED = [ts(0.0), 7, ts(4.0), ts(4.0), 9, ts(11.36), ts(11.36)]
SINGLE_END = [ts(0.0), 7, 8, ts(3.0), ts(3.0), 9, ts(12.0)]  # a lone ending timestamp: the whole window
NO_TS = [7, 8, 9, 10]
ONE_TS = [ts(0.0), 7, 8, 9]
ZERO = [ts(0.0), 7, ts(0.0), ts(0.0)]  # OpenAI's loop would not advance
ROWS = {"cut": CUT, "cut_closed": CUT_CLOSED, "single_end": SINGLE_END, "no_ts": NO_TS, "one_ts": ONE_TS,
        "zero": ZERO, "empty": []}


def test_hand_rows_mean_what_they_say():
    """The restatement on the rows above, by hand."""
    assert seek_frames(CUT) == 620 and seek_frames(CUT_CLOSED) == 1136
    assert seek_frames(SINGLE_END) == 3000 and seek_frames(NO_TS) == 3000 and seek_frames(ONE_TS) == 3000
    assert seek_frames(ZERO) == 0 and seek_frames([]) == 3000
    for name, row in ROWS.items():  # and the library's own slicing agrees
        assert whisper_amd.segments_from_tokens(row, TS0)[1] == seek_frames(row), name
    assert advance_rule(CUT, 3000, 0.1, -0.5, -1.0, 0.6) == (False, 620)
    assert advance_rule(CUT, 500, 0.1, -0.5, -1.0, 0.6) == (False, 500)
    assert advance_rule(ZERO, 3000, 0.1, -0.5, -1.0, 0.6) == (False, 3000)
    assert advance_rule(ZERO, 77, 0.1, -0.5, -1.0, 0.6) == (False, 77)
    assert advance_rule(CUT, 3000, 0.9, -1.5, -1.0, 0.6) == (True, 3000)
    assert advance_rule(CUT, 3000, 0.9, -0.5, -1.0, 0.6) == (False, 620)  # rescued by its log-probability


@pytest.mark.parametrize("name", sorted(ROWS))
@pytest.mark.parametrize("size", [3000, 2999, 1136, 621, 620, 619, 77, 1])
def test_long_advance_matches_restatement(name, size):
    row = ROWS[name]
    cases = [(0.1, -0.5, -1.0, 0.6),   # speech: never skipped
             (0.9, -1.5, -1.0, 0.6),   # silence and a low log-probability: skipped
             (0.9, -0.5, -1.0, 0.6),   # silence, rescued by the log-probability
             (0.9, -1.0, -1.0, 0.6),   # avg == threshold: not above it, skipped
             (0.6, -1.5, -1.0, 0.6),   # no_speech == threshold: not above it, kept
             (0.9, -1.5, NAN, 0.6),    # no log-probability test: nothing rescues
             (0.9, -0.5, NAN, 0.6),
             (0.9, -1.5, -1.0, NAN),   # no no-speech test: never skipped
             (0.9, -1.5, NAN, NAN),
             (0.9, 0.0, -1.0, 0.6)]    # a window without stored log-probabilities (avg 0)
    for ns, avg, lp_thr, ns_thr in cases:
        got = whisper_amd.long_advance(row, TS0, size, ns, avg, None if math.isnan(lp_thr) else lp_thr,
                                       None if math.isnan(ns_thr) else ns_thr)
        assert got == advance_rule(row, size, ns, avg, lp_thr, ns_thr), (name, size, ns, avg, lp_thr, ns_thr)
        assert 1 <= got[1] <= size


def test_long_advance_other_vocabulary():
    """Medium's <|0.00|> is 50364: the same row shifted by one."""
    row = [t - 1 if t >= TS0 else t for t in CUT]
    assert whisper_amd.long_advance(row, TS0 - 1, 3000, 0.0, 0.0) == (False, 620)


def test_long_advance_rejects_bad_arguments():
    L = whisper_amd.lib()
    sk, adv = ctypes.c_int(), ctypes.c_int()
    toks = (ctypes.c_int32 * 4)(*NO_TS)
    args = lambda **k: [k.get("tokens", toks), k.get("n", 4), TS0, k.get("size", 3000), 0.1, -0.5, -1.0, 0.6,
                        k.get("sk", ctypes.byref(sk)), k.get("adv", ctypes.byref(adv))]
    assert L.wa_long_advance(*args()) == 0
    for bad in (dict(size=0), dict(size=3001), dict(n=-1), dict(tokens=None), dict(sk=None), dict(adv=None)):
        assert L.wa_long_advance(*args(**bad)) == EINVAL, bad
    assert L.wa_long_advance(*args(tokens=None, n=0)) == 0  # an empty window needs no tokens


def test_long_round_matches_restatement():
    rng = np.random.default_rng(5)
    cases = [
        # more recordings than max_batch: the first max_batch that still have work
        ([900, 4700, 9500, 300, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], 2, 5),
        ([900, 4700, 9500, 300, 1], [900, 3000, 0, 0, 0], [1, 1, 0, 0, 0], 2, 5),
        # exhausted max_windows: seek < C but no window left
        ([9500, 9500, 9500], [6000, 3000, 9000], [2, 1, 3], 4, 2),
        ([9500, 9500, 9500], [6000, 3000, 9000], [2, 2, 3], 4, 2),
        # C == 0: never scheduled
        ([0, 0, 10], [0, 0, 0], [0, 0, 0], 3, 5),
        ([0, 0], [0, 0], [0, 0], 3, 5),
        # seek past the end (advance is clamped, but the rule is seek < C)
        ([100], [100], [1], 1, 5),
        ([100], [99], [4], 1, 5),
    ]
    for _ in range(50):
        n = int(rng.integers(1, 12))
        c = rng.integers(0, 8000, n)
        cases.append((c.tolist(), rng.integers(0, 8000, n).tolist(), rng.integers(0, 4, n).tolist(),
                      int(rng.integers(1, 6)), int(rng.integers(1, 4))))
    seen_full = seen_empty = False
    for content, seek, windows, mb, mw in cases:
        want = round_rule(content, seek, windows, mb, mw)
        assert whisper_amd.long_round(content, seek, windows, mb, mw) == want, (content, seek, windows, mb, mw)
        seen_full |= len(want) == mb and len(round_rule(content, seek, windows, 99, mw)) > mb
        seen_empty |= not want
    assert seen_full and seen_empty
    assert whisper_amd.long_round([900, 4700, 9500, 300, 1], [0] * 5, [0] * 5, 2, 5) == [0, 1]
    assert whisper_amd.long_round([0, 0, 10], [0] * 3, [0] * 3, 3, 5) == [2]


def test_long_round_whole_schedule():
    """The rule iterated to the end with a fixed advance: a waiting recording
    enters when another finishes, and every recording gets its windows."""
    content, mb, mw, step = [900, 4700, 9500, 0, 2999], 2, 3, 3000
    seek, wins, rounds = [0] * 5, [0] * 5, []
    for _ in range(100):
        got = whisper_amd.long_round(content, seek, wins, mb, mw)
        assert got == round_rule(content, seek, wins, mb, mw)
        if not got:
            break
        rounds.append(got)
        for r in got:
            seek[r] += min(step, content[r] - seek[r])
            wins[r] += 1
    assert rounds == [[0, 1], [1, 2], [2, 4], [2]]
    assert wins == [1, 2, 3, 0, 1] and seek[2] == 9000 < content[2]  # recording 2 is truncated


def test_long_round_rejects_bad_arguments():
    L = whisper_amd.lib()
    a = (ctypes.c_int32 * 4)()
    out, n = (ctypes.c_int * 4)(), ctypes.c_int()
    assert L.wa_long_round(a, a, a, 4, 2, 1, out, ctypes.byref(n)) == 0
    for args in ((None, a, a, 4, 2, 1, out, ctypes.byref(n)), (a, None, a, 4, 2, 1, out, ctypes.byref(n)),
                 (a, a, None, 4, 2, 1, out, ctypes.byref(n)), (a, a, a, 4, 2, 1, None, ctypes.byref(n)),
                 (a, a, a, 4, 2, 1, out, None), (a, a, a, 0, 2, 1, out, ctypes.byref(n)),
                 (a, a, a, 4, 0, 1, out, ctypes.byref(n)), (a, a, a, 4, 2, 0, out, ctypes.byref(n))):
        assert L.wa_long_round(*args) == EINVAL


def test_transcribe_long_rejects_bad_arguments():
    """Null pointers, counts, negative offsets and lengths, max_tokens,
    max_windows, the rung count and the temperatures are WQ4_EINVAL before any
    device work: the model here is not a model, and nothing may touch it."""
    L = whisper_amd.lib()
    model, audio = (ctypes.c_uint8 * 4096)(), (ctypes.c_float * 16)()
    addr = lambda b: ctypes.c_void_p(ctypes.addressof(b))
    off, n = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int64 * 2)(8, 8)
    temps, seed = (ctypes.c_float * 8)(0.0, 0.4), (ctypes.c_uint64 * 2)(1, 2)
    f32p, u64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)

    def options(**k):
        t = k.get("temps", temps)
        return whisper_amd.LongOptions(k.get("max_tokens", 12), k.get("max_windows", 5), 50259, 50,
                                       ctypes.cast(t, f32p) if t is not None else None, k.get("n_temperatures", 2),
                                       -1.0, 0.6, ctypes.cast(seed, u64p) if k.get("seed", True) else None)

    def call(m=model, a=audio, S=2, o=off, ns=n, opt=None, want_out=True):
        h = ctypes.c_void_p(0xDEAD)
        opt = options() if opt is None else opt
        st = L.wa_transcribe_long(addr(m) if m is not None else None, addr(a) if a is not None else None, S, o, ns,
                                  ctypes.byref(opt) if opt is not False else None,
                                  ctypes.byref(h) if want_out else None, None)
        assert not want_out or h.value is None  # never a dangling handle
        return st

    assert call(m=None) == EINVAL and "null" in L.wa_last_error().decode()
    assert call(a=None) == EINVAL
    assert call(o=None) == EINVAL and call(ns=None) == EINVAL
    assert call(opt=False) == EINVAL and call(want_out=False) == EINVAL
    assert call(opt=options(temps=None)) == EINVAL and call(opt=options(seed=False)) == EINVAL
    assert call(S=0) == EINVAL and call(S=-1) == EINVAL
    for mt in (0, -1, 225):
        assert call(opt=options(max_tokens=mt)) == EINVAL and "max_tokens" in L.wa_last_error().decode()
    assert call(opt=options(max_windows=0)) == EINVAL and "max_windows" in L.wa_last_error().decode()
    for nt in (0, 9):
        assert call(opt=options(n_temperatures=nt)) == EINVAL and "rungs" in L.wa_last_error().decode()
    for bad in (-0.1, NAN, math.inf):
        assert call(opt=options(temps=(ctypes.c_float * 8)(0.0, bad))) == EINVAL
        assert "temperature" in L.wa_last_error().decode()
    assert call(o=(ctypes.c_int64 * 2)(0, -1)) == EINVAL
    assert call(ns=(ctypes.c_int64 * 2)(8, -1)) == EINVAL
    assert call(ns=(ctypes.c_int64 * 2)(8, 1 << 40)) == EINVAL


def test_long_mel_entries_reject_bad_arguments():
    L = whisper_amd.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    off, n = (ctypes.c_int64 * 1)(0), (ctypes.c_int64 * 1)(1600)
    sk, mi = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 1)(0)
    assert L.wa_long_mel_max(0, None, 1, off, n, 80, p, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 0, off, n, 80, p, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 1, None, n, 80, p, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 1, off, n, 0, p, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 1, off, n, 80, None, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 1, (ctypes.c_int64 * 1)(-1), n, 80, p, None) == EINVAL
    assert L.wa_long_mel_max(0, p, 1, off, (ctypes.c_int64 * 1)(-1), 80, p, None) == EINVAL
    W = lambda **k: L.wa_long_mel_windows(0, k.get("a", p), k.get("B", 1), k.get("off", off), k.get("n", n),
                                          k.get("sk", sk), k.get("mi", mi), k.get("mx", p), k.get("mels", 80),
                                          k.get("out", p), None)
    for bad in (dict(a=None), dict(B=0), dict(off=None), dict(n=None), dict(sk=None), dict(mi=None), dict(mx=None),
                dict(mels=257), dict(out=None), dict(sk=(ctypes.c_int32 * 1)(-1)), dict(sk=(ctypes.c_int32 * 1)(10)),
                dict(mi=(ctypes.c_int32 * 1)(-1)), dict(n=(ctypes.c_int64 * 1)(159))):
        assert W(**bad) == EINVAL, bad


def test_result_accessors_are_null_safe():
    L = whisper_amd.lib()
    L.wa_long_result_free(None)
    assert L.wa_long_result_streams(None) == 0 and L.wa_long_result_max_tokens(None) == 0
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.wa_long_result_stream(None, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == EINVAL
    assert L.wa_long_result_windows(None, 0, None, 0, ctypes.byref(a)) == EINVAL
    assert L.wa_long_result_segments(None, 0, None, 0, ctypes.byref(a)) == EINVAL
    assert L.wa_long_result_window(None, 0, 0, None, 0, ctypes.byref(a), None, 0) == EINVAL
