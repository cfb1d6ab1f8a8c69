"""GPU tests of long-form transcription: the window mel front-end
(wa_long_mel_max / wa_long_mel_windows) against oracle/mel_oracle.py, and the
driver wa_transcribe_long against its own composition from public pieces.

Window oracle.  raw = log10(max(filterbank(power_spectrum(x ++ 800 zeros)),
1e-10)) frame by frame: mel_oracle's reflect padding of the zero-extended
signal reads x[1 .. 200] on the left and zeros on the right, which is the
extended signal of include/whisper_amd.h; frames past the oracle's are exactly
-10.  M = max(-10, raw), a window is (max(raw, M - 8) + 4) / 4 over its content
frames and exact zeros after them.  Tolerances are test_mel_gpu.py's: the GPU
accumulates the DFT in f64 and rounds once, like the oracle, so max 1e-4 and
mean 1e-6 on the normalised values cover f32 rounding ties and the log10 ulp.

Driver.  The loop is restated here from long_mel_max / long_mel_windows,
transcribe_fallback(timestamps=True) on each round's batch in scheduling order,
segments_from_tokens and the skip / advance rules written out; every field of
every window and segment must be equal, floats bit for bit.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import mel_oracle as mo

pytestmark = pytest.mark.gpu

ATOL_MAX = 1e-4  # tests/test_mel_gpu.py
ATOL_MEAN = 1e-6
N_MELS = 80
f32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def wa():
    import whisper_amd

    return whisper_amd


# ---------------------------------------------------------------- window mel --
LENGTHS = (70000, 531337, 50000)  # the last one is silence


def oracle_raw(x: np.ndarray, fb: np.ndarray) -> np.ndarray:
    """[frames, n_mels] raw log-mel of the zero-extended recording."""
    power = mo.power_spectrum(np.concatenate([x, np.zeros(800, f32)]))
    return mo._rnd(np.log10, np.maximum(mo.apply_filterbank(power, fb), f32(1e-10)))


def oracle_window(raw: np.ndarray, M: np.float32, C: int, seek: int) -> np.ndarray:
    size = min(3000, C - seek)
    out = np.zeros((raw.shape[1], 3000), f32)
    v = np.maximum(raw[seek:seek + size], f32(M) - f32(8.0))
    out[:, :size] = ((v + f32(4.0)) / f32(4.0)).astype(f32).T
    return out


@pytest.fixture(scope="module")
def recordings(torch, wa):
    """Three recordings back to back in one device buffer (behind 37 samples
    that belong to none), their oracle raw frames and maxima, and every window
    under test computed in one batch."""
    audio = mo.synthetic_audio(2, max(LENGTHS), seed=13)
    xs = [audio[0, :LENGTHS[0]].copy(), audio[1, :LENGTHS[1]].copy(), np.zeros(LENGTHS[2], f32)]
    off = np.cumsum([37] + [len(x) for x in xs])[:-1].astype(np.int64)
    n = np.array([len(x) for x in xs], np.int64)
    buf = torch.from_numpy(np.concatenate([np.full(37, 0.5, f32)] + xs)).cuda()
    fb = mo.mel_filterbank(N_MELS)
    raws = [oracle_raw(x, fb) for x in xs]
    Ms = [max(f32(-10.0), f32(r.max())) for r in raws]
    cases = []  # (recording, seek)
    for r, x in enumerate(xs):
        C = len(x) // 160
        for seek in (0, 137, C - 3000 - 1, C - 1):
            if 0 <= seek < C:
                cases.append((r, seek))
    max_dev = wa.long_mel_max(buf, off, n, N_MELS)
    rr = [c[0] for c in cases]
    wins = wa.long_mel_windows(buf, off[rr], n[rr], [c[1] for c in cases], rr, max_dev, N_MELS)
    return dict(buf=buf, off=off, n=n, raws=raws, Ms=Ms, cases=cases, max_dev=max_dev, wins=wins)


def test_maxima_match_oracle(recordings):
    got = recordings["max_dev"].cpu().numpy()
    assert got.shape == (3,)
    for r in range(3):
        assert abs(float(got[r]) - float(recordings["Ms"][r])) <= 1e-4, (r, got[r], recordings["Ms"][r])
    assert got[2] == f32(-10.0)  # silence: the floor, exactly


def test_windows_match_oracle(recordings):
    wins = recordings["wins"].cpu().numpy()
    assert wins.shape == (len(recordings["cases"]), N_MELS, 3000)
    assert (1, 319) in recordings["cases"] and (0, 436) in recordings["cases"]  # C - 3000 - 1 and C - 1
    for i, (r, seek) in enumerate(recordings["cases"]):
        C = int(recordings["n"][r]) // 160
        size = min(3000, C - seek)
        assert np.all(wins[i][:, size:] == 0.0), (r, seek)  # the zero tail, exactly
        if r == 2:
            assert np.all(wins[i][:, :size] == f32(-1.5))  # silence, exactly
            continue
        ref = oracle_window(recordings["raws"][r], recordings["Ms"][r], C, seek)
        d = np.abs(wins[i] - ref)
        print(f"recording {r} seek {seek}: max|d| {d.max():.3e} mean|d| {d.mean():.3e}")
        assert d.max() <= ATOL_MAX, (r, seek, d.max(), np.unravel_index(d.argmax(), d.shape))
        assert d.mean() <= ATOL_MEAN, (r, seek, d.mean())


def test_frame_independence_bit_for_bit(torch, wa, recordings):
    cases, wins = recordings["cases"], recordings["wins"]
    a, b = wins[cases.index((1, 0))], wins[cases.index((1, 137))]
    assert torch.equal(a[:, 137:], b[:, :3000 - 137])
    # a batch of windows equals the same windows computed one per call
    for i, (r, seek) in enumerate(cases):
        one = wa.long_mel_windows(recordings["buf"], recordings["off"][[r]], recordings["n"][[r]], [seek], [r],
                                  recordings["max_dev"], N_MELS)
        assert torch.equal(one[0], wins[i]), (r, seek)
    # and the maxima do not depend on the other recordings of the call
    for r in range(3):
        one = wa.long_mel_max(recordings["buf"], recordings["off"][[r]], recordings["n"][[r]], N_MELS)
        assert torch.equal(one, recordings["max_dev"][r:r + 1])


def test_window_past_two_to_the_31_samples(torch, wa):
    """Sample indices are 64-bit: the frames of a window that starts past sample
    2^31 of a recording are, bit for bit, those of the same samples seen as a
    short recording of their own (from its frame 2 on, where no reflected
    sample is read), under the same maximum."""
    K = (1 << 31) // 160 + 7  # first frame of the tail, past 2^31 samples
    tail = mo.synthetic_audio(1, 200000, seed=17)[0]
    n_big = 160 * K + len(tail)
    big = torch.empty(n_big, device="cuda", dtype=torch.float32)  # only the tail is read
    big[160 * K:] = torch.from_numpy(tail).cuda()
    small = big[160 * K:]
    mx = wa.long_mel_max(small, [0], [len(tail)], N_MELS)
    a = wa.long_mel_windows(big, [0], [n_big], [K + 2], [0], mx, N_MELS)
    b = wa.long_mel_windows(small, [0], [len(tail)], [2], [0], mx, N_MELS)
    size = len(tail) // 160 - 2
    assert float(b[0, :, :size].std()) > 0.01  # not a constant
    assert torch.equal(a, b)


# -------------------------------------------------------------------- driver --
SEED = 1234
TOKENS, WINDOWS, LADDER = 12, 5, (0.0, 0.4)
REC_SAMPLES = (9 * 16000 + 123, 47 * 16000 + 17, 95 * 16000 + 333)  # about 9 s, 47 s and 95 s
REC_SEEDS = (101, 202, 303)


@pytest.fixture(scope="module")
def model(wa):
    m = wa.WhisperModel("tiny_test", SEED, max_batch=2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def audio(torch):
    a = mo.synthetic_audio(3, max(REC_SAMPLES), seed=29)
    return [torch.from_numpy(a[r, :n].copy()).cuda() for r, n in enumerate(REC_SAMPLES)]


def avg_logprob(slots) -> float:
    s, cnt = 0.0, 0
    for v in slots:  # f64, in slot order
        if not np.isnan(v):
            s += float(v)
            cnt += 1
    return s / cnt if cnt else 0.0


def restate(wa, torch, m, audio, seeds, lp_thr, ns_thr, max_windows=WINDOWS, max_tokens=TOKENS):
    """The loop of include/whisper_amd.h from public pieces -> (per recording
    dicts as transcribe_long returns them, the rounds' recording lists)."""
    S = len(audio)
    n = np.array([a.numel() for a in audio], np.int64)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    buf = torch.cat(audio)
    C = [int(x) // 160 for x in n]
    M = wa.long_mel_max(buf, off, n, N_MELS)
    seek, w = [0] * S, [0] * S
    out = [{"windows": [], "segments": [], "truncated": False} for _ in range(S)]
    rounds = []
    lp_f = None if lp_thr is None else float(f32(lp_thr))
    ns_f = None if ns_thr is None else float(f32(ns_thr))
    while True:
        rec = [r for r in range(S) if seek[r] < C[r] and w[r] < max_windows][:m.max_batch]
        if not rec:
            break
        rounds.append((list(rec), [w[r] for r in rec]))
        mel = wa.long_mel_windows(buf, off[rec], n[rec], [seek[r] for r in rec], rec, M, N_MELS)
        clips = m.transcribe_fallback(mel, np.array([seeds[r] + 8 * w[r] for r in rec], np.uint64), LADDER, lp_thr,
                                      ns_thr, 50259, max_tokens=max_tokens, timestamps=True, max_initial=50)
        for clip, r in zip(clips, rec):
            size = min(3000, C[r] - seek[r])
            avg = avg_logprob(clip["logprob_slots"])
            skip = ns_f is not None and clip["no_speech_prob"] > ns_f and not (lp_f is not None and avg > lp_f)
            if skip:
                advance = size
            else:
                segs, seek_frames = wa.segments_from_tokens(clip["tokens"], m.timestamp_begin)
                advance = min(seek_frames, size)
                if advance < 1:
                    advance = size
                for s0, s1, toks in segs:
                    out[r]["segments"].append((seek[r] * 0.01 + s0, seek[r] * 0.01 + s1, toks))
            win = dict(clip, avg_logprob=avg, seek=seek[r], size=size, advance=advance, skipped=skip)
            win.pop("segments"), win.pop("seek_frames")
            out[r]["windows"].append(win)
            seek[r] += advance
            w[r] += 1
    for r in range(S):
        out[r]["truncated"] = seek[r] < C[r]
    return out, rounds


def same(got, want):
    assert len(got) == len(want)
    for r, (g, x) in enumerate(zip(got, want)):
        assert g["truncated"] == x["truncated"], r
        assert len(g["windows"]) == len(x["windows"]), (r, len(g["windows"]), len(x["windows"]))
        for i, (a, b) in enumerate(zip(g["windows"], x["windows"])):
            for k in ("seek", "size", "advance", "skipped", "rung", "tokens", "lang_token", "temperature"):
                assert a[k] == b[k], (r, i, k, a[k], b[k])
            assert np.array_equal(a["logprob_slots"].view(np.uint32), b["logprob_slots"].view(np.uint32)), (r, i)
            assert np.array_equal(a["token_logprob"].view(np.uint32), b["token_logprob"].view(np.uint32)), (r, i)
            for k in ("no_speech_prob", "lang_prob", "avg_logprob"):
                assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (r, i, k, a[k], b[k])
        assert g["segments"] == x["segments"], (r, g["segments"], x["segments"])  # f64 times, exactly


def describe(tag, res, rounds):
    for r, x in enumerate(res):
        print(tag, "recording", r, "truncated", x["truncated"],
              [(w["seek"], w["size"], w["advance"], int(w["skipped"]), w["rung"], round(w["no_speech_prob"], 4),
                round(w["avg_logprob"], 4)) for w in x["windows"]])
    print(tag, "rounds", rounds)


def test_driver_equals_its_composition(wa, torch, model, audio):
    """More recordings than max_batch, unequal lengths, one shorter than a
    window.  Run 0 (ladder off) only records the mean log-probabilities run 1's
    threshold is chosen from; run 1 makes some windows fall back; run 2 puts the
    no-speech threshold at run 1's median no_speech_prob and the
    log-probability threshold above every mean, so windows are skipped."""
    go = lambda lp, ns: model.transcribe_long(audio, seed=REC_SEEDS, temperatures=LADDER, logprob_threshold=lp,
                                              no_speech_threshold=ns, max_tokens=TOKENS, max_windows=WINDOWS)
    want0, rounds0 = restate(wa, torch, model, audio, REC_SEEDS, None, None)
    describe("run0", want0, rounds0)
    same(go(None, None), want0)
    avgs = np.sort([w["avg_logprob"] for x in want0 for w in x["windows"]])
    i = int(np.argmax(np.diff(avgs)))  # the widest gap: some windows pass rung 0, some do not
    lp1 = float(f32((avgs[i] + avgs[i + 1]) / 2))

    want1, rounds1 = restate(wa, torch, model, audio, REC_SEEDS, lp1, None)
    describe("run1", want1, rounds1)
    same(go(lp1, None), want1)
    t = model.last_timings()
    assert t["steps"] > 0 and t["encoder_ms"] > 0 and t["decode_ms"] > 0

    w1 = [w for x in want1 for w in x["windows"]]
    ns2 = float(f32(np.median([w["no_speech_prob"] for w in w1])))
    lp2 = float(f32(max(w["avg_logprob"] for x in (want0, want1) for y in x for w in y["windows"]) + 1.0))
    want2, rounds2 = restate(wa, torch, model, audio, REC_SEEDS, lp2, ns2)
    describe("run2", want2, rounds2)
    same(go(lp2, ns2), want2)

    every = [w for x in (want0, want1, want2) for y in x for w in y["windows"]]
    assert any(not w["skipped"] and w["advance"] < w["size"] for w in every), "no window advanced by a cut"
    assert any(not w["skipped"] and w["advance"] == w["size"] for w in every), "no window advanced by its size"
    assert any(w["rung"] == 0 for w in w1) and any(w["rung"] == 1 for w in w1), "run 1 kept one rung only"
    assert any(w["skipped"] for x in want2 for w in x["windows"]), "run 2 skipped nothing"
    for rounds in (rounds0, rounds1, rounds2):
        # max_batch is 2: recording 2 waits, and enters a later round with its first window once another has finished
        assert rounds[0][0] == [0, 1]
        assert any(2 in rec and ws[rec.index(2)] == 0 for rec, ws in rounds[1:]), "recording 2 never entered"


def test_one_window_per_recording(wa, torch, model, audio):
    """max_windows = 1, through the 2-D form of `audio` with n_samples per row;
    the last row has no content frame (C == 0) and yields no window."""
    L = max(REC_SAMPLES)
    rows = torch.zeros((4, L), device="cuda")
    n = list(REC_SAMPLES) + [159]
    for r, a in enumerate(audio):
        rows[r, :a.numel()] = a
    rows[3] = 0.25  # never read past its 159 samples
    got = model.transcribe_long(rows, n_samples=n, seed=REC_SEEDS + (404,), temperatures=LADDER,
                                logprob_threshold=None, no_speech_threshold=None, max_tokens=TOKENS, max_windows=1)
    want, _ = restate(wa, torch, model, audio, REC_SEEDS, None, None, max_windows=1)
    same(got[:3], want)
    for r in range(3):
        assert len(got[r]["windows"]) == 1
        assert got[r]["truncated"] == (n[r] // 160 > got[r]["windows"][0]["advance"])
    assert got[0]["windows"][0]["size"] == REC_SAMPLES[0] // 160 < 3000
    assert got[3] == {"windows": [], "segments": [], "truncated": False}
    assert got[1]["truncated"] and got[2]["truncated"]  # longer than one window
