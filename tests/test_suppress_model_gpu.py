"""Suppress-token lists end to end (WhisperModel.set_suppress_tokens): every
transcribe entry inherits the lists through its pick kernels.

The reference needs no new rule code: the numpy drivers around
whisper_oracle.SynthWhisper (the scored driver below, built as
test_timestamps_gpu.oracle_timestamps is; that driver itself; beam_ref.
oracle_beam) run over a model whose decoder_pass results are pre-masked
(suppress_ref.premask) -- the prompt pass with both lists, the steps with
`always`, the SOT pass (scores, language detection) not at all.

Comparison: test_timestamps_gpu.check_against_driver's rule -- tokens and
log-probabilities up to a clip's first pick whose margin is below 2 * 2e-3 *
max|finite logit|, at least min(8, picks) picks per clip and half of all
(clip, pick) pairs.  TINY_TEST, seed 1234, Q4_0, language 50259, 24 tokens.  The
clips were found on the CPU (the driver alone keeps the cap: 24 of 24 picks on
the scored clips, 24 / 23 / 20 on the timestamp clips).
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import beam_ref
import suppress_ref as sr
import test_longform_gpu as tl
import test_timestamps_gpu as tg
import ts_rules as tr
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

EOT = 50257
SEED = 1234
LANG = 50259
TOKENS = 24
GREEDY_CLIPS, GREEDY_ALWAYS, GREEDY_FIRST = [9, 10, 11], [46097, 48993] + sr.SPECIALS, [43675, 9576, 220, EOT]
TS_CLIPS, TS_ALWAYS, TS_FIRST = [12, 7, 1], [39553, 43675] + sr.SPECIALS, [220, EOT]


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


class Suppressed:
    """A SynthWhisper whose decoder_pass returns pre-masked logits: the prompt
    pass (fresh, more than the lone SOT) under both lists, a decode step under
    `always`; the SOT pass -- no_speech_prob, language -- unmasked."""

    def __init__(self, om, always, first):
        self.om, self.always, self.both = om, list(always), sr.union(always, first)

    def __getattr__(self, name):
        return getattr(self.om, name)

    def decoder_pass(self, tokens, positions, cache, fresh):
        z = self.om.decoder_pass(tokens, positions, cache, fresh)
        if fresh and tokens.shape[1] == 1 and (np.asarray(tokens) == wo.SOT).all():
            return z
        return sr.premask(z, self.both if fresh else self.always)


def mels(clips):
    return np.stack([wo.synthetic_mel(c, 80) for c in clips]).astype(np.float32)


def top_gap(z):
    top = np.unique(z[np.isfinite(z)])[-2:]
    return float(top[1] - top[0]) if top.size == 2 else np.inf


def oracle_scored(om, mel, lang, max_tokens):
    """test_timestamps_gpu.oracle_timestamps for the greedy scored decode: the
    prompt [SOT, lang, TRANSCRIBE, NO_TIMESTAMPS], EOT masked at the prompt's
    pick and while step + 1 < 3, the last maximum.  Per clip the picks (token,
    float64 log-probability, tolerance, margin)."""
    c = om.cfg
    B = mel.shape[0]
    tt = 50260 + c["n_lang"]
    cache = om.init_cache(om.encode(mel))
    z0 = om.decoder_pass(np.full((B, 1), wo.SOT), np.arange(1), cache, fresh=True).astype(np.float64)
    lo, hi = 50259, 50259 + c["n_lang"]
    logits = om.decoder_pass(np.array([[wo.SOT, lang, tt, tt + 4]] * B), np.arange(4), cache, fresh=True)
    position = 4
    picks = [[] for _ in range(B)]
    done = [False] * B

    def pick_all(logits, suppress):
        nxt = []
        for b in range(B):
            z = logits[b].astype(np.float64)
            if suppress:
                z[EOT] = -np.inf
            t = tr.pick(z)
            if not done[b]:
                picks[b].append((t, z[t] - tr.lse(z), 2 * 2e-3 * np.abs(z[np.isfinite(z)]).max(), top_gap(z)))
            nxt.append(t)
        return nxt

    nxt = pick_all(logits, True)
    for step in range(max_tokens):
        for b in range(B):
            done[b] = done[b] or nxt[b] == EOT
        if all(done):
            break
        logits = om.decoder_pass(np.array(nxt)[:, None], np.array([position]), cache, fresh=False)
        position += 1
        nxt = pick_all(logits, step + 1 < wo.MIN_TOKENS)
    for b in range(B):
        picks[b] = picks[b][:max_tokens]
    return {"picks": picks, "lang_tok": [lang] * B, "z0tol": 2 * 2e-3 * np.abs(z0).max(axis=1),
            "no_speech": np.exp(z0[:, tt + 3] - tg.lse_rows(z0)),
            "lang_prob": np.exp(z0[np.arange(B), [lang] * B] - tg.lse_rows(z0[:, lo:hi]))}


def check_scored(got, want, max_tokens):
    """check_against_driver without the segments."""
    total = compared = 0
    for b, g in enumerate(got):
        picks = want["picks"][b]
        k = tg.compared_steps(picks)
        total += len(picks)
        compared += k
        assert k >= min(8, len(picks)), (b, k)
        seq = tg.got_sequence(g, max_tokens)
        assert seq[:k] == [p[0] for p in picks[:k]], (b, k, seq, [p[0] for p in picks])
        err = np.abs(g["logprob_slots"][:k].astype(np.float64) - np.array([p[1] for p in picks[:k]]))
        assert (err <= np.array([p[2] for p in picks[:k]])).all(), (b, err)
        for key in ("no_speech", "lang_prob"):
            p, q = g[key if key == "lang_prob" else "no_speech_prob"], want[key][b]
            assert abs(p - q) <= q * math.expm1(want["z0tol"][b]) + 1e-12, (key, b, p, q)
        assert g["lang_token"] == want["lang_tok"][b]
    assert 2 * compared >= total, (compared, total)
    print(f"compared {compared} of {total} picks")


@pytest.fixture(scope="module")
def oracle_model():
    return wo.SynthWhisper("tiny_test", SEED)


@pytest.fixture()
def model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=12)
    yield m
    m.close()


def clean(clips, always, first):
    for c in clips:
        assert not set(c["tokens"]) & set(always), c["tokens"]
        assert c["tokens"][0] not in first, c["tokens"]


def test_scored_matches_driver(torch, oracle_model, model):
    """The three clips emit 46097 .. 48993 .. without lists and start 43675 /
    9576 / 43675 under `always` alone; with both lists pick 0 moves on and a
    `first` id returns at a later pick: `first` holds at pick 0 only."""
    mel = mels(GREEDY_CLIPS)
    x = torch.from_numpy(mel).cuda()
    free = model.transcribe_scored(x, LANG, max_tokens=TOKENS)
    assert all(set(c["tokens"]) & {46097, 48993} for c in free)
    model.set_suppress_tokens(GREEDY_ALWAYS)
    only_always = model.transcribe_scored(x, LANG, max_tokens=TOKENS)
    assert [c["tokens"][0] for c in only_always] == [43675, 9576, 43675]
    model.set_suppress_tokens(GREEDY_ALWAYS, GREEDY_FIRST)
    assert model.suppress_tokens == (tuple(GREEDY_ALWAYS), tuple(GREEDY_FIRST))
    got = model.transcribe_scored(x, LANG, max_tokens=TOKENS)
    want = oracle_scored(Suppressed(oracle_model, GREEDY_ALWAYS, GREEDY_FIRST), mel, LANG, TOKENS)
    assert all(tg.compared_steps(p) == TOKENS for p in want["picks"])  # the CPU search's figure: 24 of 24
    check_scored(got, want, TOKENS)
    clean(got, GREEDY_ALWAYS, GREEDY_FIRST)
    assert all(set(c["tokens"][1:]) & set(GREEDY_FIRST) for c in got)
    assert model.transcribe(x, LANG, max_tokens=TOKENS) == [c["tokens"] for c in got]  # the plain entry


def test_timestamps_match_driver(torch, oracle_model, model):
    mel = mels(TS_CLIPS)
    x = torch.from_numpy(mel).cuda()
    free = model.transcribe_timestamps(x, LANG, max_tokens=TOKENS)
    model.set_suppress_tokens(TS_ALWAYS, TS_FIRST)
    got = model.transcribe_timestamps(x, LANG, max_tokens=TOKENS)
    want = tg.oracle_timestamps(Suppressed(oracle_model, TS_ALWAYS, TS_FIRST), mel, LANG, TOKENS)
    assert [tg.compared_steps(p) for p in want["picks"]] == [24, 23, 20]  # the CPU search's figures
    tg.check_against_driver(got, want, TOKENS)
    clean(got, TS_ALWAYS, TS_FIRST)
    for a, b in zip(got, free):  # the same first pick, different from pick 1 on
        assert a["tokens"][0] == b["tokens"][0] and a["tokens"][1] != b["tokens"][1]
        assert b["tokens"][1] in TS_ALWAYS


def slots_bytes(c):
    return np.asarray(c["logprob_slots"]).tobytes()


def same_slots(a, b):
    """Equal values (test_sampling_gpu.same_clip: the row pick's -log S and the
    scored pick's (z - m) - log s may differ in the sign of a zero)."""
    return np.array_equal(a["logprob_slots"], b["logprob_slots"], equal_nan=True)


def test_set_then_clear(torch, model):
    import whisper_amd
    import wq4

    x = torch.from_numpy(mels(GREEDY_CLIPS)).cuda()
    fresh = model.transcribe_scored(x, None, max_tokens=TOKENS)
    fresh_ts = model.transcribe_timestamps(x, LANG, max_tokens=TOKENS)
    b0 = model.device_bytes()
    assert model.suppress_tokens == ((), ())
    assert all(49974 in c["tokens"] for c in fresh)  # what these clips emit after auto-detect
    always = GREEDY_ALWAYS + [49974]
    model.set_suppress_tokens(always, GREEDY_FIRST)
    assert model.device_bytes() > b0  # the two masks are counted
    b1 = model.device_bytes()
    listed = model.transcribe_scored(x, None, max_tokens=TOKENS)
    clean(listed, always, GREEDY_FIRST)
    for a, b in zip(listed, fresh):  # read from the unmasked SOT row: the same bits
        assert a["lang_token"] == b["lang_token"]
        for k in ("no_speech_prob", "lang_prob"):
            assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), k
    with pytest.raises(wq4.WQ4Error):  # invalid: nothing is set
        model.set_suppress_tokens([EOT], [])
    with pytest.raises(wq4.WQ4Error):
        model.set_suppress_tokens([], [model.timestamp_begin])
    assert model.suppress_tokens == (tuple(always), tuple(GREEDY_FIRST))
    again = model.transcribe_scored(x, None, max_tokens=TOKENS)
    assert [c["tokens"] for c in again] == [c["tokens"] for c in listed]
    model.set_suppress_tokens((), ())
    assert model.suppress_tokens == ((), ()) and model.device_bytes() == b1
    for run, ref in ((model.transcribe_scored(x, None, max_tokens=TOKENS), fresh),
                     (model.transcribe_timestamps(x, LANG, max_tokens=TOKENS), fresh_ts)):
        for a, b in zip(run, ref):
            assert a["tokens"] == b["tokens"] and slots_bytes(a) == slots_bytes(b)
            assert a["lang_token"] == b["lang_token"]
            for k in ("no_speech_prob", "lang_prob"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), k
    # a model that never held a list returns the same bytes
    other = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=12)
    for a, b in zip(other.transcribe_scored(x, None, max_tokens=TOKENS), fresh):
        assert a["tokens"] == b["tokens"] and slots_bytes(a) == slots_bytes(b)
    other.close()


def test_entries_agree_under_a_list(torch, model):
    """The equalities the suite asserts without a list, with lists set."""
    x = torch.from_numpy(mels(GREEDY_CLIPS)).cuda()
    model.set_suppress_tokens(GREEDY_ALWAYS, GREEDY_FIRST)
    scored = model.transcribe_scored(x, LANG, max_tokens=TOKENS)
    toks = [c["tokens"] for c in scored]
    clean(scored, GREEDY_ALWAYS, GREEDY_FIRST)
    cold = model.transcribe_sampled(x, 0.0, 7, LANG, max_tokens=TOKENS)
    for a, b in zip(cold, scored):
        assert a["tokens"] == b["tokens"] and same_slots(a, b)
    hot = model.transcribe_sampled(x, 1.0, 7, LANG, max_tokens=TOKENS)
    clean(hot, GREEDY_ALWAYS, GREEDY_FIRST)
    assert model.transcribe_beam(x, 1, 1.0, None, LANG, TOKENS) == toks
    both = torch.stack([x, x.flip(0)]).contiguous()
    for nb in (2, 3):  # units of two and of three batches
        xs = both if nb == 2 else torch.cat([both, x[None]]).contiguous()
        out = model.transcribe_batches_scored(xs, LANG, max_tokens=TOKENS)
        assert [c["tokens"] for c in out[0]] == toks and [c["tokens"] for c in out[1]] == toks[::-1]
        assert [c["tokens"] for c in out[-1]] == (toks if nb == 3 else toks[::-1])
    prompt = [wo.SOT, LANG, 50360, 50364]  # the default prompt
    assert [c["tokens"] for c in model.transcribe_prompted(x, [prompt] * 3, max_tokens=TOKENS)] == toks
    fb = model.transcribe_fallback(x, 7, (0.0,), None, None, LANG, max_tokens=TOKENS)
    for a, b in zip(fb, scored):
        assert a["tokens"] == b["tokens"] and same_slots(a, b)
    fbp = model.fallback_prompted(x, [prompt] * 3, 7, (0.0,), None, None, max_tokens=TOKENS)
    assert [c["tokens"] for c in fbp] == toks
    # the timestamp entries
    model.set_suppress_tokens(TS_ALWAYS, TS_FIRST)
    xt = torch.from_numpy(mels(TS_CLIPS)).cuda()
    ts = model.transcribe_timestamps(xt, LANG, max_tokens=TOKENS)
    clean(ts, TS_ALWAYS, TS_FIRST)
    beam1 = model.transcribe_beam(xt, 1, 1.0, None, LANG, TOKENS, timestamps=True)
    assert [c["tokens"] for c in beam1] == [c["tokens"] for c in ts]
    cold = model.transcribe_sampled(xt, 0.0, 3, LANG, max_tokens=TOKENS, timestamps=True)
    for a, b in zip(cold, ts):
        assert a["tokens"] == b["tokens"] and same_slots(a, b)


def test_wide_groups_take_the_stored_logits_kernels(torch):
    """66 clips: two groups of 33 rows, every step through the stored-logits
    kernels.  The clips are the three scored clips, repeated: every margin of
    theirs is above the tolerance, so each gets the tokens of the 3-clip call."""
    import whisper_amd

    B = 66
    assert whisper_amd.decode_group_rows(B) > 32 >= whisper_amd.decode_group_rows(3)
    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=B)
    m.set_suppress_tokens(GREEDY_ALWAYS, GREEDY_FIRST)
    x3 = torch.from_numpy(mels(GREEDY_CLIPS)).cuda()
    x = x3.repeat(B // 3, 1, 1).contiguous()
    narrow = m.transcribe_scored(x3, LANG, max_tokens=TOKENS)
    wide = m.transcribe_scored(x, LANG, max_tokens=TOKENS)
    clean(wide, GREEDY_ALWAYS, GREEDY_FIRST)
    for c, g in enumerate(wide):
        assert g["tokens"] == narrow[c % 3]["tokens"], c
    mt = torch.from_numpy(mels(TS_CLIPS)).cuda()
    m.set_suppress_tokens(TS_ALWAYS, TS_FIRST)
    narrow = m.transcribe_timestamps(mt[:1].contiguous(), LANG, max_tokens=TOKENS)
    wide = m.transcribe_timestamps(mt[:1].repeat(B, 1, 1).contiguous(), LANG, max_tokens=TOKENS)
    clean(wide, TS_ALWAYS, TS_FIRST)
    assert all(g["tokens"] == narrow[0]["tokens"] for g in wide)
    m.close()


BEAM_PICKS = 12  # test_beam_model_gpu.py's


def test_beam_matches_oracle_under_a_list(torch, oracle_model, model):
    """beam_size 3 on clips 9, 10 under the greedy lists, compared as
    test_beam_model_gpu.py compares: every candidate's tokens, the sums within
    2 * 2e-3 * max|picked logit|, no clip cut short -- a flipped decision
    anywhere fails it (the reference's smallest kept-set margins on these
    clips, printed below: 0.86 and 0.008 of the tolerance)."""
    K = 3
    mel = mels(GREEDY_CLIPS[:2])
    ref, amax, _ = beam_ref.oracle_beam(Suppressed(oracle_model, GREEDY_ALWAYS, GREEDY_FIRST), mel, K, K, LANG,
                                        BEAM_PICKS, True)
    tol = 2 * 2e-3 * amax
    model.set_suppress_tokens(GREEDY_ALWAYS, GREEDY_FIRST)
    got = model.transcribe_beam(torch.from_numpy(mel).cuda(), K, 1.0, None, LANG, BEAM_PICKS, True,
                                return_candidates=True)
    for c, (r, g) in enumerate(zip(ref, got)):
        print(f"clip {c}: margin {r['margin'] / tol:.4f} of the tolerance")
        want = sorted((tuple(t), float(s)) for t, s in r["candidates"])
        have = sorted((tuple(x["tokens"]), x["sum_logprob"]) for x in g["candidates"])
        assert [t for t, _ in have] == [t for t, _ in want], (c, have, want)
        assert len(have) == K and all(len(t) == BEAM_PICKS for t, _ in have)
        assert max(abs(a[1] - b[1]) for a, b in zip(have, want)) <= tol
        assert g["tokens"] == list(r["candidates"][r["best"]][0])
        for t, _ in have:
            assert not set(t) & set(GREEDY_ALWAYS) and t[0] not in GREEDY_FIRST, t


def test_long_form_under_a_list(torch):
    """One 70-s recording with the timestamp lists set: the driver still
    equals its composition from public pieces (transcribe_fallback on the same
    windows, bit for bit), and no window holds an `always` id."""
    import mel_oracle as mo
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=2)
    m.set_suppress_tokens(TS_ALWAYS, TS_FIRST)
    audio = [torch.from_numpy(mo.synthetic_audio(1, 70 * 16000, seed=31)[0].copy()).cuda()]
    want, rounds = tl.restate(whisper_amd, torch, m, audio, (77,), None, None)
    got = m.transcribe_long(audio, seed=(77,), temperatures=tl.LADDER, logprob_threshold=None,
                            no_speech_threshold=None, max_tokens=tl.TOKENS, max_windows=tl.WINDOWS)
    tl.same(got, want)
    assert len(got[0]["windows"]) >= 2
    for w in got[0]["windows"]:
        assert not set(w["tokens"]) & set(TS_ALWAYS), w["tokens"]
    # the same with the text ids these windows emit listed as well: the invariant holds where the list bites
    emitted = sorted({t for w in got[0]["windows"] for t in w["tokens"] if t < EOT})
    assert emitted
    m.set_suppress_tokens(TS_ALWAYS + emitted, TS_FIRST)
    want2, _ = tl.restate(whisper_amd, torch, m, audio, (77,), None, None)
    got2 = m.transcribe_long(audio, seed=(77,), temperatures=tl.LADDER, logprob_threshold=None,
                             no_speech_threshold=None, max_tokens=tl.TOKENS, max_windows=tl.WINDOWS)
    tl.same(got2, want2)
    for w in got2[0]["windows"]:
        assert not set(w["tokens"]) & set(TS_ALWAYS + emitted), w["tokens"]
    m.close()
