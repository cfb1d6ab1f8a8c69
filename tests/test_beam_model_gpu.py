"""wa_transcribe_beam end to end on TINY_TEST against the numpy oracle
(beam_ref.oracle_beam: whisper_oracle.SynthWhisper.decoder_pass with the
per-beam caches gathered physically).

Every clip is compared over all 12 picks -- candidates (tokens, lengths), the
best index, and the sums within the module's model-level tolerance 2 * 2e-3 *
max|picked logit| (test_model_gpu.py; no new number).  No clip is cut short.

Decision margins.  The synthetic weights give nearly flat logits (max about
3.7 over 51866 ids), so the candidates of a beam step lie closer together than
that tolerance: of 80 clip seeds searched on the CPU none keeps every kept-set
margin of a K = 3 or K = 5 decode above it for 12 picks (the best reach 0.2 -
0.35 of it; K = 1 keeps 2.7 x and more).  test_beam_ref.py asserts what the
chosen clips (the best three of the search) do keep: the full margin at K = 1,
and at K = 3, 5 a margin >= 0.15 of the tolerance, far above the measured
error of the runtime against the oracle, which this test prints.  The
comparison here is therefore stricter than "compare up to the first low
margin": a flipped decision anywhere fails it.

The synthetic weights never emit EOT inside 12 picks (EOT sits about 3 below
the leaders): no sequence finishes in these decodes, eot_stop = 1 and 0 agree,
and finishing is covered by the merge kernel's own test
(test_beam_pick_gpu.py) and, on the host side, by test_beam_ref.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_beam_ref as tbr
import wq4

pytestmark = pytest.mark.gpu

PICKS = tbr.MODEL_PICKS


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", tbr.MODEL_SEED, max_batch=16)
    yield m
    m.close()


def mel_dev(torch, order=(0, 1, 2)):
    _, _, mel = tbr._oracle()
    return torch.from_numpy(mel[list(order)]).cuda()


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("lang", [50259, None])
@pytest.mark.parametrize("eot_stop", [True, False])
def test_beam_matches_oracle(torch, gpu_model, K, lang, eot_stop):
    ref, tol, n_finished = tbr.oracle_case(K, lang, eot_stop)
    got = gpu_model.transcribe_beam(mel_dev(torch), K, 1.0, None, lang, PICKS, eot_stop, return_candidates=True)
    print(f"K {K} lang {lang} eot_stop {eot_stop}: the reference finished {n_finished} sequences; tolerance {tol:.4g}")
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
        # list order: the live beams finalize added, by their sums
        sums = [x["sum_logprob"] for x in g["candidates"]]
        assert sums == sorted(sums, reverse=True)
        assert 0.0 <= g["no_speech_prob"] <= 1.0 and 0.0 < g["lang_prob"] <= 1.0
        assert g["lang_token"] == (lang if lang is not None else g["lang_token"])
    print(f"  worst |sum - oracle| {worst:.3g} = {worst / tol:.4f} of the tolerance; margins / tolerance "
          f"{[round(r['margin'] / tol, 2) for r in ref]}")


def test_beam_size_one_is_greedy(torch, gpu_model):
    mel = mel_dev(torch)
    for lang in (50259, None):
        greedy = gpu_model.transcribe(mel, lang, PICKS)
        assert gpu_model.transcribe_beam(mel, 1, 1.0, None, lang, PICKS) == greedy


def test_clip_position_does_not_matter(torch, gpu_model):
    base = gpu_model.transcribe_beam(mel_dev(torch), 3, 1.0, None, 50259, PICKS, return_candidates=True)
    perm = (2, 0, 1)
    moved = gpu_model.transcribe_beam(mel_dev(torch, perm), 3, 1.0, None, 50259, PICKS, return_candidates=True)
    for i, c in enumerate(perm):
        assert moved[i]["candidates"] == base[c]["candidates"] and moved[i]["best"] == base[c]["best"]


def test_patience_and_length_penalty_are_accepted(torch, gpu_model):
    out = gpu_model.transcribe_beam(mel_dev(torch), 3, 2.0, 1.0, 50259, PICKS, return_candidates=True)
    ref = gpu_model.transcribe_beam(mel_dev(torch), 3, 1.0, None, 50259, PICKS, return_candidates=True)
    for a, b in zip(out, ref):  # nothing finishes: the same live beams, every length equal, the same winner
        assert a["candidates"] == b["candidates"] and a["best"] == b["best"]


def test_neighbours_and_device_bytes(torch):
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", tbr.MODEL_SEED, max_batch=16)
    mel = mel_dev(torch)
    t0 = m.transcribe(mel, 50259, PICKS)
    s0 = m.transcribe_scored(mel, 50259, PICKS)
    b0 = m.device_bytes()
    m.transcribe_beam(mel, 5, 1.0, None, 50259, PICKS)
    b1 = m.device_bytes()
    assert b1 > b0
    m.transcribe_beam(mel, 3, 1.0, None, None, PICKS)
    assert m.device_bytes() == b1  # the first beam call only
    assert m.transcribe(mel, 50259, PICKS) == t0
    s1 = m.transcribe_scored(mel, 50259, PICKS)
    for a, b in zip(s0, s1):
        assert a["tokens"] == b["tokens"] and a["lang_token"] == b["lang_token"]
        for k in ("no_speech_prob", "lang_prob"):
            assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes()
        assert np.asarray(a["logprob_slots"]).tobytes() == np.asarray(b["logprob_slots"]).tobytes()
    m.close()


def test_rejects_bad_arguments(torch, gpu_model):
    mel = mel_dev(torch)
    for K, patience in ((0, 1.0), (9, 1.0), (3, 0.5), (3, 6.0), (6, 1.0)):  # 6 beams x 3 clips > max_batch 16
        with pytest.raises(wq4.WQ4Error):
            gpu_model.transcribe_beam(mel, K, patience, None, 50259, PICKS)


def test_beam_call_climbs_the_range_tiers(torch, tmp_path):
    """The attention-output stress fixture of test_range_guard.py: a beam call
    comes back with finite sums at range tier 3 (the f32 form of the beam
    self-attention), and beam_size 1 gives the f32 oracle's greedy tokens."""
    import test_range_guard as rg
    import whisper_amd

    t32, _, _, _, _ = rg.oracle_run("value")
    n = len(rg.CLIPS)
    m = whisper_amd.WhisperModel.from_gguf(rg._write("value", tmp_path), "tiny_test", max_batch=2 * n)
    mel = torch.from_numpy(rg._mels(m.config["n_mels"])).cuda()
    out = m.transcribe_beam(mel, 2, 1.0, None, 50259, rg.STEPS, eot_stop=False, return_candidates=True)
    assert m.range_tier == 3
    for c in out:
        assert len(c["candidates"]) == 2
        assert all(np.isfinite(x["sum_logprob"]) and len(x["tokens"]) == rg.STEPS for x in c["candidates"])
    assert m.transcribe_beam(mel, 1, 1.0, None, 50259, rg.STEPS, eot_stop=False) == t32
    m.close()
