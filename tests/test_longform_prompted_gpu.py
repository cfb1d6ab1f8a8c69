"""wa_transcribe_long_prompted: the long-form driver with initial prompts and
previous-text conditioning equals its restatement from public pieces --
wa_long_round's rule, long_mel_windows, fallback_prompted, wa_long_advance's
rule and the prompt rule of prompt_ref.py -- bit for bit, on the recordings of
test_longform_gpu.py; without prompts it equals transcribe_long."""
from __future__ import annotations

import math

import numpy as np
import pytest

import mel_oracle as mo
import prompt_ref as R

pytestmark = pytest.mark.gpu

N_MELS = 80
SEED = 1234
TOKENS, WINDOWS, LADDER = 12, 5, (0.0, 0.4, 0.8)
REC_SAMPLES = (9 * 16000 + 123, 47 * 16000 + 17, 95 * 16000 + 333)  # test_longform_gpu.py's three recordings
REC_SEEDS = (101, 202, 303)
INITIAL = ([], R.make_prompt(30, 30)[1:26], [])  # one initial prompt: 25 text ids for recording 1
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


def restate(wa, torch, m, audio, seeds, lp_thr, ns_thr, initial, condition, reset_temperature=0.5):
    """The loop of include/whisper_amd.h with the prompt handling, from public pieces."""
    S = len(audio)
    n = np.array([a.numel() for a in audio], np.int64)
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    buf = torch.cat(audio)
    C = [int(x) // 160 for x in n]
    M = wa.long_mel_max(buf, off, n, N_MELS)
    ctx, ts0 = m.config["n_text_ctx"], m.timestamp_begin
    seek, w = [0] * S, [0] * S
    prev, reset = [list(p) for p in initial], [0] * S
    out = [{"windows": [], "segments": [], "truncated": False} for _ in range(S)]
    lp_f = None if lp_thr is None else float(f32(lp_thr))
    ns_f = None if ns_thr is None else float(f32(ns_thr))
    while True:
        rec = wa.long_round(C, seek, w, m.max_batch, WINDOWS)
        if not rec:
            break
        mel = wa.long_mel_windows(buf, off[rec], n[rec], [seek[r] for r in rec], rec, M, N_MELS)
        built = [R.long_prompt_window(prev[r], reset[r], ctx, TOKENS) for r in rec]
        clips = m.fallback_prompted(mel, [p for p, _ in built], np.array([seeds[r] + 8 * w[r] for r in rec], np.uint64),
                                    LADDER, lp_thr, ns_thr, max_tokens=TOKENS, timestamps=True, max_initial=50)
        for clip, r, (_, k) in zip(clips, rec, built):
            size = min(3000, C[r] - seek[r])
            avg = avg_logprob(clip["logprob_slots"])
            skip, advance = wa.long_advance(clip["tokens"], ts0, size, clip["no_speech_prob"], avg,
                                            float("nan") if lp_f is None else lp_f, float("nan") if ns_f is None else ns_f)
            if not skip:
                for s0, s1, toks in clip["segments"]:
                    out[r]["segments"].append((seek[r] * 0.01 + s0, seek[r] * 0.01 + s1, toks))
            prev[r], reset[r] = R.long_prompt_next(prev[r], reset[r], clip["tokens"], skip, clip["temperature"], condition,
                                                   reset_temperature, ts0)
            win = dict(clip, avg_logprob=avg, seek=seek[r], size=size, advance=advance, skipped=bool(skip), prompt_len=k)
            win.pop("segments"), win.pop("seek_frames")
            out[r]["windows"].append(win)
            seek[r] += advance
            w[r] += 1
    for r in range(S):
        out[r]["truncated"] = seek[r] < C[r]
    return out


def same(got, want, prompt_len=True):
    assert len(got) == len(want)
    for r, (g, x) in enumerate(zip(got, want)):
        assert g["truncated"] == x["truncated"], r
        assert len(g["windows"]) == len(x["windows"]), (r, len(g["windows"]), len(x["windows"]))
        for i, (a, b) in enumerate(zip(g["windows"], x["windows"])):
            for k in ("seek", "size", "advance", "skipped", "rung", "tokens", "lang_token", "temperature") + \
                    (("prompt_len",) if prompt_len else ()):
                assert a[k] == b[k], (r, i, k, a[k], b[k])
            assert np.array_equal(a["logprob_slots"].view(np.uint32), b["logprob_slots"].view(np.uint32)), (r, i)
            for k in ("no_speech_prob", "lang_prob", "avg_logprob"):
                assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (r, i, k, a[k], b[k])
        assert g["segments"] == x["segments"], (r, g["segments"], x["segments"])


def test_prompted_driver_equals_its_composition(wa, torch, model, audio):
    """One initial prompt, conditioning on.  Run 0 (ladder off) records the mean
    log-probabilities that run 1's threshold is chosen from; run 1 makes some
    windows fall back, so hot rungs move the reset mark."""
    go = lambda lp, ns, cond: model.transcribe_long(audio, seed=REC_SEEDS, temperatures=LADDER, logprob_threshold=lp,
                                                    no_speech_threshold=ns, max_tokens=TOKENS, max_windows=WINDOWS,
                                                    initial_prompts=INITIAL, condition_on_previous_text=cond)
    want0 = restate(wa, torch, model, audio, REC_SEEDS, None, None, INITIAL, True)
    same(go(None, None, True), want0)
    ks = [[w["prompt_len"] for w in x["windows"]] for x in want0]
    print("prompt_len", ks)
    assert ks[1][0] == len(INITIAL[1]) and ks[0][0] == 0
    assert any(k > 0 for k in ks[0][1:] + ks[2][1:]), "no window was conditioned on previous text"
    avgs = np.sort([w["avg_logprob"] for x in want0 for w in x["windows"]])
    i = int(np.argmax(np.diff(avgs)))
    lp1 = float(f32((avgs[i] + avgs[i + 1]) / 2))
    want1 = restate(wa, torch, model, audio, REC_SEEDS, lp1, None, INITIAL, True)
    same(go(lp1, None, True), want1)
    rungs = {w["rung"] for x in want1 for w in x["windows"]}
    assert 0 in rungs and len(rungs) > 1, rungs
    # conditioning off: only the initial prompt, and only in window 0
    want2 = restate(wa, torch, model, audio, REC_SEEDS, None, None, INITIAL, False)
    same(go(None, None, False), want2)
    assert [[w["prompt_len"] for w in x["windows"]][1:] for x in want2] == [[0] * (len(x["windows"]) - 1) for x in want2]


def test_no_prompt_is_transcribe_long(model, audio):
    """No initial tokens and conditioning off: the existing path, bit for bit."""
    args = dict(seed=REC_SEEDS, temperatures=LADDER, logprob_threshold=None, no_speech_threshold=None, max_tokens=TOKENS,
                max_windows=WINDOWS)
    want = model.transcribe_long(audio, **args)
    got = model.transcribe_long(audio, initial_prompts=[[], [], []], condition_on_previous_text=False, **args)
    same(got, want, prompt_len=False)
    assert all(w["prompt_len"] == 0 for x in got for w in x["windows"])
