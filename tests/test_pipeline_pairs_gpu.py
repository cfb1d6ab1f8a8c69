"""Paired decode of pipelined transcribes (wa_transcribe_batches,
include/whisper_amd.h): batches of 16 .. 32 clips decode two at a time, one
decode group per batch, the second on the model's second lane of encoder
planes and self-attention caches (allocated by the first paired call); an odd
last batch decodes alone on today's groups.  Every kernel computes per row
what it computes in wa_transcribe, so the tokens must EQUAL those of one
wa_transcribe per batch -- for even and odd batch counts, at every overlap
depth, explicit and auto language, EOT stop and fixed length -- and the model
must be left as a plain wa_transcribe expects it."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import whisper_oracle as wo

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, B, STEPS = 300, 16, 24  # tests/pairs_child.py decodes the same clips


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def model():
    import whisper_amd

    return whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)


@pytest.fixture(scope="module")
def x5(torch):
    """Five batches of 16 clips, on the device."""
    m = np.stack([np.stack([wo.synthetic_mel(FIRST + i * B + c, 80) for c in range(B)]) for i in range(5)])
    return torch.from_numpy(m).cuda()


@pytest.fixture(scope="module")
def sequential(model, x5):
    """One transcribe per batch of x5, computed once per (language, EOT mode)."""
    memo = {}

    def get(lang, eot):
        if (lang, eot) not in memo:
            memo[(lang, eot)] = [model.transcribe(x5[i], lang, max_tokens=STEPS, eot_stop=eot) for i in range(5)]
        return memo[(lang, eot)]

    return get


@pytest.mark.parametrize("NB,overlap,lang,eot", [
    (2, None, 50259, True),    # one pair, no masked part at all
    (3, None, None, True),     # pair + odd tail, auto language
    (4, "0", 50259, False),    # two pairs, only the conv stem beside the first, fixed length
    (5, "2", None, False),     # two pairs + tail, the whole tiny encoder beside each decode
    (3, "2", 50259, True),
    (4, None, None, True),
    (5, "0", 50259, True),
    (2, "2", None, False),
])
def test_paired_tokens_equal_sequential(model, x5, sequential, monkeypatch, NB, overlap, lang, eot):
    if overlap is None:
        monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("WA_ENC_OVERLAP", overlap)
    got = model.transcribe_batches(x5[:NB], lang, max_tokens=STEPS, eot_stop=eot)
    assert got == sequential(lang, eot)[:NB]
    assert model.pipeline_pairs() == NB // 2
    st = model.pipeline_stats()
    assert st["batches"] == NB and st["masked_cus"] == 32
    if overlap is not None and NB > 2:  # NB = 2 is one pair: nothing runs masked
        assert st["overlap_layers"] == int(overlap)
    t = model.last_timings()
    assert t["decode_ms"] > 0
    if not eot:
        assert t["steps"] == STEPS


def test_knob_off_equals_default(model, x5, monkeypatch):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    want = model.transcribe_batches(x5[:4], 50259, max_tokens=STEPS, eot_stop=False)
    assert model.pipeline_pairs() == 2
    env = dict(os.environ)
    env.pop("WA_ENC_OVERLAP", None)
    env["WA_PAIR_BATCHES"] = "0"
    r = subprocess.run([sys.executable, os.path.join(HERE, "pairs_child.py")], env=env, capture_output=True,
                       text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    off = json.loads(r.stdout.strip().splitlines()[-1])
    assert off["pairs"] == 0
    assert off["tokens"] == want


def test_below_threshold_is_unpaired(model, x5, monkeypatch):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    x = x5[:2, :15].contiguous()
    seq = [model.transcribe(x[i], 50259, max_tokens=STEPS) for i in range(2)]
    assert model.transcribe_batches(x, 50259, max_tokens=STEPS) == seq
    assert model.pipeline_pairs() == 0
    assert model.pipeline_stats()["batches"] == 2


def test_plain_transcribe_after_paired_call(model, x5, sequential, monkeypatch):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    before = sequential(50259, True)
    few = x5[0, :5].contiguous()
    before_few = model.transcribe(few, 50259, max_tokens=STEPS)
    model.transcribe_batches(x5[1:5], 50259, max_tokens=STEPS)
    assert model.pipeline_pairs() == 2
    # 16 clips (two groups of 8 on the first lane), then 5 (one group over the K/V caches)
    assert model.transcribe(x5[0], 50259, max_tokens=STEPS) == before[0]
    assert model.transcribe(few, 50259, max_tokens=STEPS) == before_few


def test_second_lane_allocated_once(torch, x5, monkeypatch):
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
    try:
        n0 = m.device_bytes()
        m.transcribe(x5[0], 50259, max_tokens=4)
        m.transcribe_batches(x5[:2, :15].contiguous(), 50259, max_tokens=4)
        assert m.device_bytes() == n0  # unpaired users never hold the lane
        m.transcribe_batches(x5[:2], 50259, max_tokens=4)
        n1 = m.device_bytes()
        cfg = m.config
        lane = B * (cfg["n_audio_ctx"] * 2 * cfg["n_audio_state"] * 2
                    + cfg["n_text_layer"] * 2 * cfg["n_text_ctx"] * cfg["n_text_state"] * 4)
        assert n1 - n0 == lane  # f16 hi / lo planes + f32 K and V caches per layer, max_batch clips
        m.transcribe_batches(x5[:3], 50259, max_tokens=4)
        assert m.device_bytes() == n1
    finally:
        m.close()
