"""Units of up to three batches in pipelined transcribes
(wa_transcribe_batches, include/whisper_amd.h): batches of 17 .. 32 clips
decode up to three at a time, one decode group per batch, batch j of a unit
on lane j of encoder planes and self-attention caches (each allocated by the
first call that forms so wide a unit).  A call is cut into units widest first
with no lone last batch where two units of two serve (4 -> 2 + 2, 7 -> 3 + 2
+ 2); batches of exactly 16 clips keep pairs.  Every kernel computes per row
what it computes in wa_transcribe, so the tokens must EQUAL those of one
wa_transcribe per batch -- for a triple, 2 + 2, 3 + 2 and 3 + 2 + 2, at every
overlap depth, explicit and auto language, EOT stop and fixed length -- and
the model must be left as a plain wa_transcribe expects it.

The masked stream stops after the first batch of the next unit (its L
layers): WA_ENC_OVERLAP beyond L is the depth L, which the cases at "4" pin
for the tiny encoder's L = 2."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import whisper_oracle as wo

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, B, STEPS = 500, 17, 24  # tests/lanes_child.py decodes the same clips
UNITS = {3: [3], 4: [2, 2], 5: [3, 2], 7: [3, 2, 2]}  # the units of a call over NB batches


def test_unit_sizes_table():
    import whisper_amd

    for width in (1, 2, 3):
        for nb in range(1, 22):
            sizes = whisper_amd.pipeline_unit_sizes(nb, width)
            assert sum(sizes) == nb, (nb, width, sizes)
            assert all(1 <= s <= width for s in sizes), (nb, width, sizes)
            if nb > 1 and width > 1:
                # an odd count at width 2 cannot avoid its lone last batch; nothing else leaves one
                assert sizes.count(1) == (1 if width == 2 and nb % 2 else 0), (nb, width, sizes)
            assert sizes == sorted(sizes, reverse=True), (nb, width, sizes)  # widest first
    for nb, want in UNITS.items():
        assert whisper_amd.pipeline_unit_sizes(nb, 3) == want
    assert whisper_amd.pipeline_unit_sizes(10, 3) == [3, 3, 2, 2]
    assert whisper_amd.pipeline_unit_sizes(20, 3) == [3] * 6 + [2]
    assert whisper_amd.pipeline_unit_sizes(5, 2) == [2, 2, 1]  # today's pairs
    assert whisper_amd.pipeline_unit_sizes(1, 3) == [1]
    for bad in ((0, 3), (3, 0), (3, 4)):
        with pytest.raises(Exception):
            whisper_amd.pipeline_unit_sizes(*bad)


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
def x7(torch):
    """Seven batches of 17 clips, on the device."""
    m = np.stack([np.stack([wo.synthetic_mel(FIRST + i * B + c, 80) for c in range(B)]) for i in range(7)])
    return torch.from_numpy(m).cuda()


@pytest.fixture(scope="module")
def sequential(model, x7):
    """One transcribe per batch of x7, computed once per (language, EOT mode)."""
    memo = {}

    def get(lang, eot):
        if (lang, eot) not in memo:
            memo[(lang, eot)] = [model.transcribe(x7[i], lang, max_tokens=STEPS, eot_stop=eot) for i in range(7)]
        return memo[(lang, eot)]

    return get


def lane_bytes(cfg, clips):
    """f16 hi / lo planes + f32 K and V caches per decoder layer, `clips` clips."""
    return clips * (cfg["n_audio_ctx"] * 2 * cfg["n_audio_state"] * 2
                    + cfg["n_text_layer"] * 2 * cfg["n_text_ctx"] * cfg["n_text_state"] * 4)


@gpu
@pytest.mark.parametrize("NB,overlap,lang,eot", [
    (3, None, 50259, True),    # one triple, no masked part at all
    (4, None, None, True),     # 2 + 2 and not 3 + 1, auto language
    (5, "0", 50259, False),    # 3 + 2, only the conv stem beside the triple, fixed length
    (7, "2", None, False),     # 3 + 2 + 2, the whole tiny encoder of each next unit's first batch beside a decode
    (5, "4", None, True),      # a depth past the first batch's layers
    (7, None, 50259, True),
    (4, "4", 50259, False),
    (3, "2", None, False),
    (7, "0", None, True),
])
def test_lane_tokens_equal_sequential(model, x7, sequential, monkeypatch, NB, overlap, lang, eot):
    if overlap is None:
        monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("WA_ENC_OVERLAP", overlap)
    got = model.transcribe_batches(x7[:NB], lang, max_tokens=STEPS, eot_stop=eot)
    assert got == sequential(lang, eot)[:NB]
    assert model.pipeline_units3() == UNITS[NB].count(3)
    assert model.pipeline_pairs() == UNITS[NB].count(2)  # so no unit of one
    st = model.pipeline_stats()
    assert st["batches"] == NB and st["masked_cus"] == 32
    assert (st["pairs"], st["units3"]) == (UNITS[NB].count(2), UNITS[NB].count(3))
    if overlap is not None and len(UNITS[NB]) > 1:  # one unit: nothing runs masked
        assert st["overlap_layers"] == min(int(overlap), model.config["n_audio_layer"])
    t = model.last_timings()
    assert t["decode_ms"] > 0
    if not eot:
        assert t["steps"] == STEPS


@gpu
@pytest.mark.parametrize("lanes,pairs,units3", [("2", 2, 0), ("1", 0, 0)])
def test_lanes_knob_equals_default(model, x7, monkeypatch, lanes, pairs, units3):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    want = model.transcribe_batches(x7[:5], 50259, max_tokens=STEPS, eot_stop=False)
    assert (model.pipeline_pairs(), model.pipeline_units3()) == (1, 1)
    env = dict(os.environ)
    env.pop("WA_ENC_OVERLAP", None)
    env["WA_LANES"] = lanes
    r = subprocess.run([sys.executable, os.path.join(HERE, "lanes_child.py")], env=env, capture_output=True,
                       text=True, timeout=100)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert (got["pairs"], got["units3"]) == (pairs, units3)  # today's pairs (2 + 2 + 1) / every batch on its own
    assert got["lanes"] == int(lanes) - 1  # a capped call never allocates the lanes it does not use
    assert got["tokens"] == want


@gpu
def test_sixteen_clip_batches_keep_pairs(torch, x7, monkeypatch):
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
    try:
        x = x7[:3, :16].contiguous()
        seq = [m.transcribe(x[i], 50259, max_tokens=STEPS) for i in range(3)]
        n0 = m.device_bytes()
        assert m.transcribe_batches(x, 50259, max_tokens=STEPS) == seq
        assert (m.pipeline_pairs(), m.pipeline_units3()) == (1, 0)  # one pair plus a tail
        assert m.device_bytes() - n0 == lane_bytes(m.config, B)  # no third lane
    finally:
        m.close()


@gpu
def test_lanes_allocated_once_each(torch, x7, monkeypatch):
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
    try:
        lane = lane_bytes(m.config, B)
        n0 = m.device_bytes()
        m.transcribe(x7[0], 50259, max_tokens=4)
        assert m.device_bytes() == n0
        m.transcribe_batches(x7[:2], 50259, max_tokens=4)
        assert m.device_bytes() - n0 == lane
        m.transcribe_batches(x7[:4], 50259, max_tokens=4)  # 2 + 2: still two lanes
        assert (m.pipeline_pairs(), m.pipeline_units3()) == (2, 0)
        assert m.device_bytes() - n0 == lane
        m.transcribe_batches(x7[:3], 50259, max_tokens=4)
        assert m.pipeline_units3() == 1
        assert m.device_bytes() - n0 == 2 * lane
        # narrower and equally wide calls afterwards release nothing and allocate nothing
        for nb in (2, 1, 5, 7):
            m.transcribe_batches(x7[:nb], 50259, max_tokens=4)
            assert m.device_bytes() - n0 == 2 * lane
        m.transcribe(x7[0], 50259, max_tokens=4)
        assert m.device_bytes() - n0 == 2 * lane
    finally:
        m.close()


@gpu
def test_plain_transcribe_after_three_lane_call(model, x7, sequential, monkeypatch):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    before = sequential(50259, True)
    few = x7[0, :5].contiguous()
    before_few = model.transcribe(few, 50259, max_tokens=STEPS)
    model.transcribe_batches(x7[1:4], 50259, max_tokens=STEPS)
    assert model.pipeline_units3() == 1
    # 17 clips (two groups on the first lane), then 5 (one group over the K/V caches)
    assert model.transcribe(x7[0], 50259, max_tokens=STEPS) == before[0]
    assert model.transcribe(few, 50259, max_tokens=STEPS) == before_few
