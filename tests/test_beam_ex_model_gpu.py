"""wa_transcribe_beam_ex end to end on TINY_TEST: beam search under the
timestamp rules and after caller prompts against the numpy oracle
(beam_ts_ref.oracle_beam_ex: whisper_oracle.SynthWhisper.decoder_pass, the
rows' logits masked by ts_rules from each row's gathered history, the per-beam
caches gathered physically), and the equalities the header states.

Every clip is compared over all 12 picks: candidates (tokens, lengths) and the
best index exact, the sums within the module's model-level tolerance 2 * 2e-3 *
max|logit a pick saw| (test_model_gpu.py; no new number).  The clips' decision
margins -- kept set, rank, and rule f of every live row -- are asserted on the
CPU (test_beam_ex_ref.py): the whole tolerance at K = 1 with an explicit
language, a share >= 0.15 elsewhere, as in test_beam_ref.py; each test prints
the worst |sum - oracle| / tolerance it met.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_beam_ex_ref as ter
import test_beam_ref as tbr
import wq4

pytestmark = pytest.mark.gpu

PICKS = ter.MODEL_PICKS
TS0 = 50365


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", ter.MODEL_SEED, max_batch=16)
    yield m
    m.close()


def mel_dev(torch, clips=ter.MODEL_CLIPS, order=(0, 1, 2)):
    _, _, mel = ter._oracle(clips)
    return torch.from_numpy(mel[list(order)]).cuda()


def compare(ref, got, tol, K, timestamps=True):
    """Candidates exact, sums within tol, the best index, the segments; returns the worst sum error."""
    import whisper_amd

    worst = 0.0
    for c, (r, g) in enumerate(zip(ref, got)):
        want = sorted((tuple(t), float(s)) for t, s in r["candidates"])
        have = sorted((tuple(x["tokens"]), x["sum_logprob"]) for x in g["candidates"])
        assert [t for t, _ in have] == [t for t, _ in want], (c, have, want)
        assert len(have) == K and all(len(t) == PICKS for t, _ in have)
        err = max(abs(a[1] - b[1]) for a, b in zip(have, want))
        worst = max(worst, err)
        assert err <= tol, (c, err, tol)
        assert g["tokens"] == list(r["candidates"][r["best"]][0])
        assert g["candidates"][g["best"]]["tokens"] == g["tokens"]
        sums = [x["sum_logprob"] for x in g["candidates"]]
        assert sums == sorted(sums, reverse=True)  # the live beams finalize added, by their sums
        if timestamps:
            for x in [g] + g["candidates"]:
                segs, seek = whisper_amd.segments_from_tokens(x["tokens"], TS0)
                assert x["segments"] == segs and x["seek_frames"] == seek
            assert g["tokens"][0] >= TS0  # rule e: every sequence starts with a timestamp
        assert 0.0 <= g["no_speech_prob"] <= 1.0 and 0.0 < g["lang_prob"] <= 1.0
    return worst


# -------------------------------------------------------------- timestamps --
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("lang", [50259, None])
@pytest.mark.parametrize("eot_stop", [True, False])
def test_beam_timestamps_matches_oracle(torch, gpu_model, K, lang, eot_stop):
    ref, tol, n_finished = ter.oracle_case(K, lang, eot_stop)
    got = gpu_model.transcribe_beam(mel_dev(torch), K, 1.0, None, lang, PICKS, eot_stop, return_candidates=True,
                                    timestamps=True)
    worst = compare(ref, got, tol, K)
    for g in got:
        assert g["lang_token"] == (lang if lang is not None else g["lang_token"])
    print(f"K {K} lang {lang} eot_stop {eot_stop}: finished {n_finished}; worst |sum - oracle| {worst:.3g} = "
          f"{worst / tol:.4f} of the tolerance {tol:.4g}; margins / tolerance "
          f"{[round(ter.clip_margin(r) / tol, 2) for r in ref]}")


def test_beam_size_one_is_transcribe_timestamps(torch, gpu_model):
    import test_timestamps_gpu as ttg
    import whisper_oracle as wo

    mel = np.stack([wo.synthetic_mel(c, 80) for c in ttg.MODEL_CLIPS[50259]]).astype(np.float32)
    mel = torch.from_numpy(mel).cuda()
    greedy = gpu_model.transcribe_timestamps(mel, 50259, max_tokens=ttg.MODEL_TOKENS)
    beam = gpu_model.transcribe_beam(mel, 1, 1.0, None, 50259, ttg.MODEL_TOKENS, timestamps=True)
    n_ts = 0
    for g, b in zip(greedy, beam):
        assert b["tokens"] == g["tokens"]
        assert b["segments"] == g["segments"] and b["seek_frames"] == g["seek_frames"]
        assert len(b["candidates"]) == 1
        n_ts += sum(t >= TS0 for t in b["tokens"])
    assert n_ts >= 2 * len(beam)


def test_timestamp_clip_position_does_not_matter(torch, gpu_model):
    base = gpu_model.transcribe_beam(mel_dev(torch), 3, 1.0, None, 50259, PICKS, return_candidates=True,
                                     timestamps=True)
    perm = (2, 0, 1)
    moved = gpu_model.transcribe_beam(mel_dev(torch, order=perm), 3, 1.0, None, 50259, PICKS, return_candidates=True,
                                      timestamps=True)
    for i, c in enumerate(perm):
        assert moved[i]["candidates"] == base[c]["candidates"] and moved[i]["best"] == base[c]["best"]


def test_max_initial_bounds_the_first_timestamp(torch, gpu_model):
    out = gpu_model.transcribe_beam(mel_dev(torch), 3, 1.0, None, 50259, 4, return_candidates=True, timestamps=True,
                                    max_initial=0)
    for g in out:  # <|0.00|> alone at pick 0: one live beam offers it, the others are dead until pick 1
        assert all(x["tokens"][0] == TS0 for x in g["candidates"]) and len(g["candidates"]) == 3
        assert all(np.isfinite(x["sum_logprob"]) for x in g["candidates"])


def test_neighbours_and_device_bytes(torch):
    """Plain transcribe_beam, transcribe and transcribe_scored give the same
    bytes before and after timestamp and prompted beam calls; device_bytes
    grows on the first such call only."""
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", ter.MODEL_SEED, max_batch=16)
    mel = mel_dev(torch)

    def snapshot():
        t = m.transcribe(mel, 50259, PICKS)
        s = m.transcribe_scored(mel, 50259, PICKS)
        b = m.transcribe_beam(mel, 3, 1.0, None, 50259, PICKS, return_candidates=True)
        a = m.transcribe_beam(mel, 5, 1.0, None, None, PICKS, return_candidates=True)
        return t, s, b, a

    def same(x, y):
        assert x[0] == y[0]
        for a, b in zip(x[1], y[1]):
            assert a["tokens"] == b["tokens"] and a["lang_token"] == b["lang_token"]
            for k in ("no_speech_prob", "lang_prob"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes()
            assert np.asarray(a["logprob_slots"]).tobytes() == np.asarray(b["logprob_slots"]).tobytes()
        for u, v in ((x[2], y[2]), (x[3], y[3])):
            for a, b in zip(u, v):
                assert a["candidates"] == b["candidates"] and a["best"] == b["best"]
                for k in ("no_speech_prob", "lang_prob", "sum_logprob"):
                    assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes()

    before = snapshot()
    b0 = m.device_bytes()
    m.transcribe_beam(mel, 3, 1.0, None, 50259, PICKS, timestamps=True)
    b1 = m.device_bytes()
    assert b1 > b0
    m.transcribe_beam(mel, 5, 1.0, None, None, PICKS, timestamps=True)
    assert m.device_bytes() == b1
    same(before, snapshot())
    prompts = [ter.make_prompt(n, 100 + n) for n in ter.PROMPT_LENGTHS]
    m.transcribe_beam(mel, 3, 1.0, None, None, PICKS, timestamps=True, prompts=prompts)
    b2 = m.device_bytes()
    assert b2 > b1
    m.transcribe_beam(mel, 3, 1.0, None, None, PICKS, prompts=[ter.make_prompt(4, 0, False)] * 3)
    assert m.device_bytes() == b2
    same(before, snapshot())
    assert m.device_bytes() == b2
    m.close()


# ----------------------------------------------------------------- prompts --
def test_default_prompt_given_by_the_caller(torch, gpu_model):
    """(i) [SOT, lang, TRANSCRIBE, NO_TIMESTAMPS] as a caller prompt: the
    candidates of the lang_token call (the prompt runs through the prefill
    instead of the fixed-prompt pass: the sums agree within the tolerance)."""
    _, tol, _ = tbr.oracle_case(3, 50259, True)
    mel = mel_dev(torch, tbr.MODEL_CLIPS)
    want = gpu_model.transcribe_beam(mel, 3, 1.0, None, 50259, PICKS, return_candidates=True)
    got = gpu_model.transcribe_beam(mel, 3, 1.0, None, None, PICKS, return_candidates=True,
                                    prompts=[ter.make_prompt(4, 0, False)] * 3)
    worst = 0.0
    for w, g in zip(want, got):
        assert [x["tokens"] for x in g["candidates"]] == [x["tokens"] for x in w["candidates"]]
        assert g["best"] == w["best"] and g["lang_token"] == 50259
        worst = max([worst] + [abs(a["sum_logprob"] - b["sum_logprob"]) for a, b in zip(g["candidates"], w["candidates"])])
    assert worst <= tol
    print(f"caller default prompt: worst |sum - lang_token call| {worst:.3g} = {worst / tol:.4f} of the tolerance")


def test_prompted_beam_size_one_is_transcribe_prompted(torch, gpu_model):
    """(ii) K = 1 under prompts of 4, 5, 37 and 130 tokens: transcribe_prompted's greedy tokens."""
    import prompt_ref

    mel = torch.from_numpy(prompt_ref.mels(len(prompt_ref.LENGTHS))).cuda()
    prompts, _ = prompt_ref.prompts()
    greedy = gpu_model.transcribe_prompted(mel, prompts, PICKS)
    beam = gpu_model.transcribe_beam(mel, 1, 1.0, None, None, PICKS, prompts=prompts)
    assert beam == [g["tokens"] for g in greedy]
    assert all(len(t) > 0 for t in beam)


def ragged(lengths, salt=0):
    return [ter.make_prompt(n, 100 + n + salt) for n in lengths]


def test_ragged_prompts_do_not_leak_between_clips(torch, gpu_model):
    """(iii) prompts of 3, 7 and 12 tokens (<|startofprev|> + text), K = 3, with
    timestamps: a clip's candidates and sums are the same bits when the other
    clips' prompts change length and content and when the clips are permuted.
    A beam self-attention that ignores pad reads the other-length garbage in
    front of a short prompt and fails this."""
    def run(prompts, order=(0, 1, 2)):
        return gpu_model.transcribe_beam(mel_dev(torch, ter.PROMPT_CLIPS, order), 3, 1.0, None, None, PICKS,
                                         return_candidates=True, timestamps=True, prompts=prompts)

    def same(a, b):
        assert a["candidates"] == b["candidates"] and a["best"] == b["best"]
        for x, y in zip(a["candidates"], b["candidates"]):
            assert np.float32(x["sum_logprob"]).tobytes() == np.float32(y["sum_logprob"]).tobytes()
        for k in ("no_speech_prob", "lang_prob"):
            assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes()

    base_p = ragged(ter.PROMPT_LENGTHS)
    base = run(base_p)
    for keep, other in ((0, (3, 12, 7)), (1, (12, 7, 3)), (2, (7, 3, 12))):
        p = ragged(other, salt=50)
        p[keep] = base_p[keep]
        same(run(p)[keep], base[keep])
    perm = (2, 0, 1)
    moved = run([base_p[c] for c in perm], perm)
    for i, c in enumerate(perm):
        same(moved[i], base[c])
    # the prompts matter at all: clip 2 under the short prompt decodes differently
    assert run(ragged((3, 7, 3)))[2]["candidates"] != base[2]["candidates"]


def test_ragged_prompted_timestamps_match_oracle(torch, gpu_model):
    """(iv) ragged prompts, K = 3, timestamps, against the oracle (the prompt through decoder_pass)."""
    ref, tol, n_finished, prompts = ter.oracle_prompted_case()
    got = gpu_model.transcribe_beam(mel_dev(torch, ter.PROMPT_CLIPS), 3, 1.0, None, None, PICKS,
                                    return_candidates=True, timestamps=True, prompts=prompts)
    worst = compare(ref, got, tol, 3)
    for g in got:
        assert g["lang_token"] == 50259
    print(f"ragged prompts: finished {n_finished}; worst |sum - oracle| {worst:.3g} = {worst / tol:.4f} of the "
          f"tolerance {tol:.4g}; margins / tolerance {[round(ter.clip_margin(r) / tol, 2) for r in ref]}")


# ------------------------------------------------- errors and range tiers --
def test_rejects_bad_arguments(torch, gpu_model):
    mel = mel_dev(torch)
    ok = ragged(ter.PROMPT_LENGTHS)
    ctx = gpu_model.config["n_text_ctx"]
    b0 = gpu_model.device_bytes()
    bad = [dict(prompts=[ok[0], ok[1], [50258] * (ctx - PICKS + 1)]),  # longest prompt + max_tokens > n_text_ctx
           dict(prompts=[ok[0], ok[1], [50258, 51866]]),  # an id outside the vocabulary
           dict(prompts=[ok[0], ok[1], []]),  # an empty prompt
           dict(prompts=ok, beam_size=9), dict(prompts=ok, beam_size=6),  # 6 beams x 3 clips > max_batch 16
           dict(timestamps=True, beam_size=0), dict(timestamps=True, patience=0.5)]
    for kw in bad:
        kw = dict({"beam_size": 3, "patience": 1.0}, **kw)
        with pytest.raises(wq4.WQ4Error):
            gpu_model.transcribe_beam(mel, kw.pop("beam_size"), kw.pop("patience"), None, 50259, PICKS, **kw)
    assert gpu_model.device_bytes() == b0  # refused before any device work


def test_timestamp_beam_call_climbs_the_range_tiers(torch, tmp_path):
    """The attention-output stress fixture of test_range_guard.py under the
    timestamp rules: the call comes back with finite sums at range tier 3."""
    import test_range_guard as rg
    import whisper_amd

    n = len(rg.CLIPS)
    m = whisper_amd.WhisperModel.from_gguf(rg._write("value", tmp_path), "tiny_test", max_batch=2 * n)
    mel = torch.from_numpy(rg._mels(m.config["n_mels"])).cuda()
    out = m.transcribe_beam(mel, 2, 1.0, None, 50259, rg.STEPS, eot_stop=False, return_candidates=True,
                            timestamps=True)
    assert m.range_tier == 3
    for c in out:
        assert len(c["candidates"]) == 2
        assert all(np.isfinite(x["sum_logprob"]) and len(x["tokens"]) == rg.STEPS for x in c["candidates"])
        assert all(x["tokens"][0] >= TS0 for x in c["candidates"])
    m.close()
