"""Caller prompts of any length through the model (wa_transcribe_prompted,
wa_transcribe_fallback_prompted, wa_prompt_logits_ragged) on tiny_test.

Oracle: the unmodified float32 oracle composed by prompt_ref.py (decoder_pass
over the whole prompt, then the step loop), on a fixture whose float32 and
float64 runs emit the same tokens (test_prompted.py).  Tolerances are those of
test_model_gpu.py (logits: 2e-3 * max|oracle|; tokens identical) and of
test_scores_gpu.py (a log-probability: 2 * 2e-3 * max|row|)."""
from __future__ import annotations

import math

import numpy as np
import pytest

import prompt_ref as R
import sample_rules as sr
import ts_rules as tr
import whisper_oracle as wo

SEED = R.SEED
EOT = R.EOT


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    yield m
    m.close()


@pytest.fixture(scope="module")
def mel(torch):
    return torch.from_numpy(R.mels(len(R.LENGTHS))).cuda()


@pytest.fixture(scope="module")
def batch_run(gpu_model, mel):
    """transcribe_prompted of the four clips under prompts of 4, 5, 37 and 130 tokens, greedy, 32 steps."""
    return gpu_model.transcribe_prompted(mel, R.prompts()[0], max_tokens=R.STEPS)


def lse64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]


def same_clip(a, b):
    """Two clips' tokens and scores, bit for bit."""
    assert a["tokens"] == b["tokens"]
    assert a["logprob_slots"].tobytes() == b["logprob_slots"].tobytes()
    for key in ("no_speech_prob", "lang_prob"):
        assert np.float32(a[key]).tobytes() == np.float32(b[key]).tobytes(), key
    assert a["lang_token"] == b["lang_token"]


def check_clip(got, want):
    """Tokens identical; every stored log-probability and the SOT scores within the score tolerance."""
    assert got["tokens"] == want["tokens"]
    seq = list(want["tokens"]) + ([EOT] if len(want["tokens"]) < R.STEPS else [])
    slots = got["logprob_slots"]
    assert np.isnan(slots[len(seq):]).all() and not np.isnan(slots[:len(seq)]).any()
    for s, t in enumerate(seq):
        row = want["picked"][s].astype(np.float64)
        lp = row[t] - lse64(row)
        tol = 2 * 2e-3 * np.abs(row[np.isfinite(row)]).max()
        assert abs(float(slots[s]) - lp) <= tol, (s, slots[s], lp, tol)
    z0 = want["z0"].astype(np.float64)
    z0tol = 2 * 2e-3 * np.abs(z0).max()
    lo, hi = 50259, 50259 + 100
    q = math.exp(z0[R.NO_TIMESTAMPS - 1] - lse64(z0))
    assert abs(got["no_speech_prob"] - q) <= q * math.expm1(z0tol) + 1e-12
    q = math.exp(z0[R.LANG] - lse64(z0[lo:hi]))
    assert got["lang_token"] == R.LANG and abs(got["lang_prob"] - q) <= q * math.expm1(z0tol) + 1e-12


# ------------------------------------------------------------------ parity --
@pytest.mark.gpu
def test_prompt_logits_ragged_match_oracle(torch, gpu_model, mel):
    """Lengths (4, 5, 37, 130) in one batch, and 227 alone."""
    ref = R.reference("float32")
    batch, long = R.prompts()
    gpu_model.encode(mel)
    out = gpu_model.prompt_logits_ragged(batch).cpu().numpy()
    gpu_model.encode(mel[:1])
    out = np.concatenate([out, gpu_model.prompt_logits_ragged([long]).cpu().numpy()])
    for got, want in zip(out, [c["first"] for c in ref["batch"]] + [ref["long"]["first"]]):
        err = np.max(np.abs(got - want))
        print(f"prompt logits: max error {err:.3e}, max |oracle| {np.max(np.abs(want)):.3e}")
        assert err <= 2e-3 * np.max(np.abs(want)), (err, np.max(np.abs(want)))
        assert wo.SynthWhisper.argmax_last(got) == wo.SynthWhisper.argmax_last(want)


@pytest.mark.gpu
def test_prompted_tokens_and_scores_match_oracle(gpu_model, mel, batch_run):
    ref = R.reference("float32")
    for got, want in zip(batch_run, ref["batch"]):
        check_clip(got, want)
    alone = gpu_model.transcribe_prompted(mel[:1], [R.prompts()[1]], max_tokens=R.STEPS)
    check_clip(alone[0], ref["long"])


@pytest.mark.gpu
def test_default_prompt_is_transcribe(gpu_model, mel, batch_run):
    """[SOT, lang, TRANSCRIBE, NO_TIMESTAMPS] through the prefill gives transcribe's tokens."""
    default = [[R.SOT, R.LANG, R.TRANSCRIBE, R.NO_TIMESTAMPS]] * 4
    got = gpu_model.transcribe_prompted(mel, default, max_tokens=R.STEPS)
    assert [c["tokens"] for c in got] == gpu_model.transcribe(mel, R.LANG, max_tokens=R.STEPS)
    assert got[0]["tokens"] == batch_run[0]["tokens"]


# ------------------------------------------------------------ independence --
@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [None, 0.7])
def test_clip_is_independent_of_the_batch(gpu_model, mel, batch_run, temperature):
    """Each clip alone and inside the mixed batch: the same tokens and scores,
    bit for bit, greedy and sampled; and at another place in the batch."""
    batch = R.prompts()[0]
    seeds = np.array([5, 6, 7, 8], np.uint64)
    if temperature is None:
        mixed = batch_run
    else:
        mixed = gpu_model.transcribe_prompted(mel, batch, max_tokens=R.STEPS, temperature=temperature, seed=seeds)
        assert [c["tokens"] for c in mixed] != [c["tokens"] for c in batch_run]
    for b in range(4):
        alone = gpu_model.transcribe_prompted(mel[b:b + 1], [batch[b]], max_tokens=R.STEPS, temperature=temperature,
                                              seed=seeds[b:b + 1])
        same_clip(alone[0], mixed[b])
    order = [3, 0, 2, 1]
    moved = gpu_model.transcribe_prompted(mel[order].contiguous(), [batch[i] for i in order], max_tokens=R.STEPS,
                                          temperature=temperature, seed=seeds[order])
    for i, b in enumerate(order):
        same_clip(moved[i], mixed[b])


@pytest.mark.gpu
def test_scores_follow_the_last_sot(gpu_model, mel):
    """No SOT: NaN no_speech_prob, lang_token -1, NaN lang_prob; SOT followed by a
    non-language id: the no-speech score stands, the language scores do not."""
    text = [100, 200, 300]
    got = gpu_model.transcribe_prompted(mel[:3], [text, text + [R.SOT, R.TRANSCRIBE], text + [R.SOT]], max_tokens=4)
    assert math.isnan(got[0]["no_speech_prob"]) and got[0]["lang_token"] == -1 and math.isnan(got[0]["lang_prob"])
    for c in got[1:]:
        assert 0.0 <= c["no_speech_prob"] <= 1.0 and c["lang_token"] == -1 and math.isnan(c["lang_prob"])


# ----------------------------------------------- unprompted calls unchanged --
@pytest.mark.gpu
def test_unprompted_calls_are_unchanged(torch):
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    x = torch.from_numpy(R.mels(3, first=11)).cuda()
    before = m.transcribe_scored(x, R.LANG, max_tokens=12)
    key = m.decode_graph_key(0)
    n0 = m.device_bytes()
    prompted = m.transcribe_prompted(x, [R.make_prompt(n, n) for n in (9, 4, 40)], max_tokens=12)
    assert m.device_bytes() > n0  # the prefill's arrays (and, past the few-clip caches, its K / V) are counted
    n1 = m.device_bytes()
    assert m.decode_graph_key(0) == key  # the same layout and mode: kept apart beside the key
    after = m.transcribe_scored(x, R.LANG, max_tokens=12)
    assert m.decode_graph_key(0) == key
    for a, b in zip(after, before):
        same_clip(a, b)
    again = m.transcribe_prompted(x, [R.make_prompt(n, n) for n in (9, 4, 40)], max_tokens=12)
    assert m.device_bytes() == n1  # allocated once
    for a, b in zip(again, prompted):
        same_clip(a, b)
    with pytest.raises(whisper_amd.wq4.WQ4Error):
        m.transcribe_prompted(x, [[R.SOT] * 225] * 3, max_tokens=224)
    with pytest.raises(whisper_amd.wq4.WQ4Error):
        m.transcribe_prompted(x, [[R.SOT], [], [R.SOT]], max_tokens=4)
    with pytest.raises(whisper_amd.wq4.WQ4Error):
        m.transcribe_prompted(x, [[R.SOT], [51866], [R.SOT]], max_tokens=4)
    m.close()


# -------------------------------------------------- timestamps and the ladder --
@pytest.mark.gpu
def test_timestamps_under_a_prompt_obey_the_rules(gpu_model, mel):
    """timestamps = 1 under prompts that end at TRANSCRIBE: every emitted id is
    one the rule record of its history allows (ts_rules.py)."""
    V, ts0 = gpu_model.config["n_vocab"], gpu_model.timestamp_begin
    batch = [p[:-1] for p in R.prompts()[0]]  # without NO_TIMESTAMPS
    got = gpu_model.transcribe_prompted(mel, batch, max_tokens=24, temperature=0.0, seed=1, timestamps=True)
    for c in got:
        toks = c["tokens"]
        assert toks and toks[0] >= ts0
        for s, t in enumerate(toks):
            ok = tr.allowed_from_record(tr.record(toks[:s], ts0, V), ts0, V, s < wo.MIN_TOKENS)
            assert ok[t], (s, t, toks)
        assert "segments" in c


@pytest.mark.gpu
def test_fallback_prompted_composes_the_rungs(gpu_model, mel):
    """Rungs (0, 0.4, 0.8): every clip's result is that of transcribe_prompted at
    the rung the ladder's rule keeps, seeds seed + r."""
    n, ladder = 12, (0.0, 0.4, 0.8)
    batch = R.prompts()[0]
    seeds = np.array([11, 22, 33, 44], np.uint64)
    rungs = [gpu_model.transcribe_prompted(mel, batch, max_tokens=n, temperature=t, seed=seeds + np.uint64(r))
             for r, t in enumerate(ladder)]
    means = np.sort([sr.mean_logprob(c["logprob_slots"]) for c in rungs[0]])
    i = int(np.argmax(np.diff(means)))
    thr = float((means[i] + means[i + 1]) / 2)
    res = [[(sr.mean_logprob(c["logprob_slots"]), c["no_speech_prob"]) for c in rung] for rung in rungs]
    for lp_thr, want in ((thr, sr.ladder(res, thr, float("nan"))), (math.inf, [2, 2, 2, 2]), (None, [0, 0, 0, 0])):
        got = gpu_model.fallback_prompted(mel, batch, seeds, ladder, lp_thr, None, max_tokens=n)
        assert [c["rung"] for c in got] == want
        for c, g in enumerate(got):
            same_clip(g, rungs[g["rung"]][c])
    assert 0 in sr.ladder(res, thr, float("nan")) and any(r > 0 for r in sr.ladder(res, thr, float("nan")))


# -------------------------------------------------------------- range tiers --
PROMPT40 = R.make_prompt(40, 40)


def _stress_reference(dtype):
    import test_range_guard as rg

    om = rg.stress_oracle("value", dtype)
    enc = om.encode(rg._mels(om.cfg["n_mels"]).astype(om.dt))
    return [c["tokens"] for c in R.prompted_transcribe(om, enc, [PROMPT40] * len(rg.CLIPS), rg.STEPS, eot_stop=False)]


_STRESS: dict = {}


def stress_tokens(dtype):
    if dtype not in _STRESS:
        _STRESS[dtype] = _stress_reference(dtype)
    return _STRESS[dtype]


def test_value_fixture_has_no_near_ties_under_the_prompt():
    """CPU: on the `value` fixture of test_range_guard.py under the 40-token prompt, float32 and float64 agree."""
    assert stress_tokens(np.float32) == stress_tokens(np.float64)


@pytest.mark.gpu
def test_prompted_call_climbs_the_range_tiers(torch, tmp_path):
    """A flagged prompted call climbs the tiers as any call does: the `value`
    fixture ends at tier 3 with the float32 oracle's tokens, sticky."""
    import test_range_guard as rg
    import whisper_amd

    m = whisper_amd.WhisperModel.from_gguf(rg._write("value", tmp_path), "tiny_test", max_batch=len(rg.CLIPS))
    x = torch.from_numpy(rg._mels(m.config["n_mels"])).cuda()
    got = m.transcribe_prompted(x, [PROMPT40] * len(rg.CLIPS), max_tokens=rg.STEPS, eot_stop=False)
    assert m.range_tier == 3
    assert [c["tokens"] for c in got] == stress_tokens(np.float32)
    again = m.transcribe_prompted(x, [PROMPT40] * len(rg.CLIPS), max_tokens=rg.STEPS, eot_stop=False)
    assert m.range_tier == 3 and [c["tokens"] for c in again] == stress_tokens(np.float32)
    m.close()
