"""GPU parity tests of the Whisper model around the Q4 path (run on an MI355X).

Oracle: oracle/whisper_oracle.py, a float32 numpy restatement of
src/model/*.rs on bit-identical synthetic weights (tests/test_synth.py).
Tolerances (stated here, DESIGN.md "Numerics"):
  encoder_out:        max|gpu - oracle| <= 2e-3 * max|oracle|
  prompt logits:      max|gpu - oracle| <= 2e-3 * max|oracle| (absolute ~1e-3)
  emitted token ids:  identical (greedy decode, 32 steps, 2 clips, both the
                      explicit-language and the auto-language prompt)
Model-level parity is "unpinned" w.r.t. the reference binary (it has no
golden tokens) and pinned to this restatement.
"""
from __future__ import annotations

import numpy as np
import pytest

import whisper_oracle as wo
import wq4

pytestmark = pytest.mark.gpu

SEED = 1234


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.fixture(scope="module")
def oracle_model():
    return wo.SynthWhisper("tiny_test", SEED)


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    return whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)


def mels(n, n_mels=80, first=0):
    return np.stack([wo.synthetic_mel(first + c, n_mels) for c in range(n)]).astype(np.float32)


def test_encoder_matches_oracle(torch, oracle_model, gpu_model):
    mel = mels(2)
    ref = oracle_model.encode(mel)
    out = gpu_model.encode(torch.from_numpy(mel).cuda()).cpu().numpy()
    err = np.max(np.abs(out - ref))
    assert err <= 2e-3 * np.max(np.abs(ref)), (err, np.max(np.abs(ref)))


def test_prompt_logits_match_oracle(torch, oracle_model, gpu_model):
    mel = mels(2)
    enc = oracle_model.encode(mel)
    cache = oracle_model.init_cache(enc)
    prompt = np.array([[50258, 50259, 50360, 50364]] * 2)
    ref = oracle_model.decoder_pass(prompt, np.arange(4), cache, fresh=True)
    gpu_model.encode(torch.from_numpy(mel).cuda())
    out = gpu_model.prompt_logits(torch.from_numpy(prompt.astype(np.int32)).cuda()).cpu().numpy()
    err = np.max(np.abs(out - ref))
    assert err <= 2e-3 * np.max(np.abs(ref)), (err, np.max(np.abs(ref)))
    assert [wo.SynthWhisper.argmax_last(r) for r in out] == [wo.SynthWhisper.argmax_last(r) for r in ref]


@pytest.mark.parametrize("lang", [50259, None])
def test_transcribe_tokens_match_oracle(torch, oracle_model, gpu_model, lang):
    mel = mels(2)
    ref = oracle_model.transcribe(mel, lang, max_tokens=32)
    got = gpu_model.transcribe(torch.from_numpy(mel).cuda(), lang, max_tokens=32)
    assert got == ref


def test_batch_invariance_of_tokens(torch, gpu_model):
    mel = torch.from_numpy(mels(3, first=5)).cuda()
    batch = gpu_model.transcribe(mel, 50259, max_tokens=24)
    for i in range(3):
        assert gpu_model.transcribe(mel[i:i + 1], 50259, max_tokens=24)[0] == batch[i]


def test_fixed_length_decode_and_timings(torch, gpu_model):
    mel = torch.from_numpy(mels(1)).cuda()
    out = gpu_model.transcribe(mel, 50259, max_tokens=16, eot_stop=False)
    assert len(out[0]) == 16
    t = gpu_model.last_timings()
    assert t["steps"] == 16 and t["encoder_ms"] > 0 and t["decode_ms"] > 0


def test_rejects_bad_arguments(torch, gpu_model):
    mel = torch.from_numpy(mels(1)).cuda()
    with pytest.raises(wq4.WQ4Error):
        gpu_model.transcribe(mel, 50259, max_tokens=225)
    with pytest.raises(wq4.WQ4Error):
        gpu_model.transcribe(torch.from_numpy(mels(5)).cuda(), 50259, max_tokens=4)


# ------------------------------------------------- GGUF loader (§8(f) rank 2) --
def test_gguf_model_equals_synthetic(torch, gpu_model, tmp_path):
    """load_whisper_from_gguf on a checkpoint written by tools/write_gguf.py
    (the converter's format) gives the synthetic model bit for bit."""
    import whisper_amd
    import write_gguf

    p = tmp_path / "tiny.gguf"
    write_gguf.write_synthetic_gguf(str(p), "tiny_test", SEED)
    g = whisper_amd.WhisperModel.from_gguf(str(p), "tiny_test", max_batch=4)
    mel = torch.from_numpy(mels(2, first=7)).cuda()
    assert torch.equal(g.encode(mel), gpu_model.encode(mel))
    assert g.transcribe(mel, 50259, max_tokens=24) == gpu_model.transcribe(mel, 50259, max_tokens=24)
    g.close()


def test_gguf_loader_errors(torch, tmp_path, monkeypatch):
    import whisper_amd
    import write_gguf

    tensors = write_gguf.synthetic_tensors("tiny_test", SEED)
    p = tmp_path / "t.gguf"
    write_gguf.write_gguf(str(p), tensors, "t")
    with pytest.raises(wq4.WQ4Error, match="elements, expected|wrong shape"):
        whisper_amd.WhisperModel.from_gguf(str(p), "medium", max_batch=1)  # D = 1024 expected
    # an F32 linear weight is refused like loader.rs:131-134
    real = write_gguf.should_quantize
    monkeypatch.setattr(write_gguf, "should_quantize",
                        lambda n, s: False if n == "encoder.blocks.0.attn.query.weight" else real(n, s))
    q = tmp_path / "f32.gguf"
    write_gguf.write_gguf(str(q), tensors, "t")
    with pytest.raises(wq4.WQ4Error, match="Expected Q4_0 for weight 'encoder.blocks.0.attn.query.weight'"):
        whisper_amd.WhisperModel.from_gguf(str(q), "tiny_test", max_batch=1)
    monkeypatch.undo()
    del tensors["decoder.ln.bias"]
    r = tmp_path / "missing.gguf"
    write_gguf.write_gguf(str(r), tensors, "t")
    with pytest.raises(wq4.WQ4Error, match="Tensor 'decoder.ln.bias' not found"):
        whisper_amd.WhisperModel.from_gguf(str(r), "tiny_test", max_batch=1)


# ------------------------------------------- f16 weights (BASELINE config 5) --
def test_f16_weight_model_matches_oracle(torch):
    """Config 5's unquantized path: linear weights f16 (the synthetic values
    rounded to f16), same kernels; tokens equal to the oracle run on the same
    f16 weights, and a GGUF F16 checkpoint loads to the same model."""
    import whisper_amd

    ref = wo.SynthWhisper("tiny_test", SEED, weights="f16")
    gm = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=2, weights="f16")
    assert gm.weights == "f16"
    mel = mels(2, first=3)
    enc = gm.encode(torch.from_numpy(mel).cuda()).cpu().numpy()
    want = ref.encode(mel)
    assert np.max(np.abs(enc - want)) <= 2e-3 * np.max(np.abs(want))
    got = gm.transcribe(torch.from_numpy(mel).cuda(), 50259, max_tokens=16)
    assert got == ref.transcribe(mel, 50259, max_tokens=16)
    gm.close()


def test_f16_gguf_checkpoint(torch, tmp_path):
    import whisper_amd
    import write_gguf

    p = tmp_path / "f16.gguf"
    write_gguf.write_synthetic_gguf(str(p), "tiny_test", SEED, linear="f16")
    g = whisper_amd.WhisperModel.from_gguf(str(p), "tiny_test", max_batch=2)
    s = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=2, weights="f16")
    assert g.weights == "f16"
    mel = torch.from_numpy(mels(2, first=9)).cuda()
    assert torch.equal(g.encode(mel), s.encode(mel))


def test_two_decode_groups_match_oracle(torch, oracle_model, gpu_model):
    """16 clips take the two-stream decode path (two groups of 8, each its own
    graph and KV cache, wa_forward.cpp decode_groups); their tokens must equal
    the single-group path's (batches of 4) and the oracle's for a sample."""
    import whisper_amd

    m16 = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=16)
    mel = mels(16, first=20)
    got = m16.transcribe(torch.from_numpy(mel).cuda(), 50259, max_tokens=24)
    assert len(got) == 16
    for c0 in range(0, 16, 4):
        assert gpu_model.transcribe(torch.from_numpy(mel[c0:c0 + 4]).cuda(), 50259, max_tokens=24) == got[c0:c0 + 4]
    sample = [0, 7, 8, 15]  # first and last clip of each group
    assert oracle_model.transcribe(mel[sample], 50259, max_tokens=24) == [got[i] for i in sample]
    m16.close()


@pytest.mark.parametrize("eot_scale", [10.0, 12.0])
def test_ragged_eot_stop_matches_oracle(torch, tmp_path, eot_scale):
    """Ragged end of transcript (whisper.rs:104-125): the EOT row of the token
    embedding is scaled so that some clips emit EOT after the 3 forced tokens
    and others run to max_tokens (oracle lengths at 10x: one clip of six stops
    at 7 tokens; at 12x most stop at 3). Finished clips keep running masked in
    their decode group, a group whose clips are all done stops replaying, and
    every clip's tokens must equal the oracle's, through both decode groups."""
    import whisper_amd
    import write_gguf

    tensors = write_gguf.synthetic_tensors("tiny_test", SEED)
    tensors["decoder.token_embedding.weight"][wo.EOT] *= eot_scale
    p = tmp_path / "eot.gguf"
    write_gguf.write_gguf(str(p), tensors, "eot")
    g = whisper_amd.WhisperModel.from_gguf(str(p), "tiny_test", max_batch=16)
    ref = wo.SynthWhisper("tiny_test", SEED)
    ref.w["decoder.token_embedding.weight"][wo.EOT] *= eot_scale
    mel = mels(16, first=30)
    want = ref.transcribe(mel, 50259, max_tokens=24)
    assert len({len(t) for t in want}) > 1  # the case is ragged
    got = g.transcribe(torch.from_numpy(mel).cuda(), 50259, max_tokens=24)
    assert got == want
    # a decode group whose clips have all emitted EOT stops replaying (the
    # host's lag-4 poll of n_done, wa_transcribe.cpp run_decode): when every clip of one
    # group of 8 stops early, fewer than max_tokens steps run
    longest = [max(len(t) for t in want[i:i + 8]) for i in (0, 8)]
    steps = g.last_timings()["steps"]
    if max(longest) < 24 - 5:
        assert steps <= max(longest) + 1 + 4 + 1, (steps, longest)  # + EOT step + poll lag + slack
    else:
        assert steps == 24
    g.close()


# ------------------------------------- full-size models (BASELINE configs) --
@pytest.mark.parametrize("variant,n_mels,batch", [("large_v3", 128, 32), ("medium", 80, 16)])
def test_full_size_batch_invariance(torch, variant, n_mels, batch):
    """At the bench's full sizes the numpy oracle is too slow, so parity rests
    on a size-independent property: a clip's encoder output and tokens are the
    same alone (B = 1: one decode group, M = 1 GEMV plans, 1500-row encoder
    GEMMs) as inside a full batch (two decode groups, 48000-row encoder GEMMs
    at Large-V3) -- bit for bit, since every kernel's per-row arithmetic is
    batch-independent by construction."""
    import whisper_amd

    m = whisper_amd.WhisperModel(variant, SEED, max_batch=batch)
    mel = torch.from_numpy(mels(batch, n_mels=n_mels, first=40)).cuda()
    enc = m.encode(mel)
    got = m.transcribe(mel, 50259, max_tokens=32)
    assert len(got) == batch
    for i in (0, batch // 2 - 1, batch // 2, batch - 1):  # first and last clip of each decode group
        assert torch.equal(m.encode(mel[i:i + 1])[0], enc[i])
        assert m.transcribe(mel[i:i + 1], 50259, max_tokens=32)[0] == got[i]
    m.close()
