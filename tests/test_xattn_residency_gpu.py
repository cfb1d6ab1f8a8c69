"""The cache policy of the cross-attention's encoder-plane loads (wa_xattn.hip:
resident sub-chunks load with the default policy, the others nontemporal)
changes no value: for every share -- everything streamed, a partial share
whose workgroups walk a mix of both, everything resident -- the output of
wa_xattn_check equals the default call's bit for bit and stays within the
float64 bound of tests/test_xattn_gpu.py (2e-5 of max|ref| for f16x2, 5e-3
for f16), through the fused kernel (decode and prompt rows) and the
split-phase kernels of few rows; a paired transcribe under a forced partial
share returns the tokens of one transcribe per batch, and the share is part of
a decode group's graph key."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import whisper_oracle as wo
import wq4

pytestmark = pytest.mark.gpu

ENV = "WA_XATTN_RESIDENT_MB"


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def reference(q, wk, wv, bv, enc, Tq, H):
    """softmax(q K^T / 8) V per head in float64 (attention.rs:204-298, key bias absent)."""
    B, T, D = enc.shape
    q = q.astype(np.float64).reshape(B, Tq, H, 64)
    K = (enc.astype(np.float64) @ wk.astype(np.float64).T).reshape(B, T, H, 64)
    V = (enc.astype(np.float64) @ wv.astype(np.float64).T + bv).reshape(B, T, H, 64)
    s = np.einsum("bqhd,bthd->bhqt", q, K) / 8.0
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return np.einsum("bhqt,bthd->bqhd", p, V).reshape(B * Tq, H * 64)


# B, Tq, T, H, precision, WA_XATTN_SMALL_ROWS (0: the fused kernel, 8: the split phases)
CASES = [
    (3, 1, 100, 6, wq4.PREC_F16X2, "0"),   # ragged last sub-chunk, 7 sub-chunks: fewer than 8 splits
    (3, 1, 100, 6, wq4.PREC_F16, "0"),
    (2, 1, 200, 20, wq4.PREC_F16X2, "0"),  # second head tile; 2 sub-chunks per workgroup
    (2, 3, 200, 6, wq4.PREC_F16X2, "0"),   # prompt rows (Tq = 3)
    (2, 1, 200, 6, wq4.PREC_F16X2, "8"),   # xattn_scores_kernel / xattn_z_kernel
    (3, 1, 200, 20, wq4.PREC_F16X2, "8"),
]


@pytest.mark.parametrize("B,Tq,T,H,prec,small", CASES)
def test_share_changes_no_bit(torch, monkeypatch, B, Tq, T, H, prec, small):
    import whisper_amd

    D, ns = 64 * H, 1 if prec == wq4.PREC_F16 else 2
    rng = np.random.default_rng(100 * B + 10 * Tq + H)
    enc = rng.standard_normal((B, T, D)).astype(np.float32)
    q = (2.0 * rng.standard_normal((B * Tq, D))).astype(np.float32)
    wk = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
    wv = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
    bv = rng.uniform(-0.02, 0.02, D).astype(np.float32)
    rk, rv = wq4.quantize_q4_0(wk), wq4.quantize_q4_0(wv)
    ref = reference(q, oracle.dequantize_np(rk, D * D).reshape(D, D), oracle.dequantize_np(rv, D * D).reshape(D, D),
                    bv, enc, Tq, H)
    args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, rk, rv, bv, enc)]
    monkeypatch.setenv("WA_XATTN_SMALL_ROWS", small)
    monkeypatch.delenv(ENV, raising=False)
    assert whisper_amd.xattn_resident_share(B, T, ns, D) == whisper_amd.XATTN_SHARE_DEN  # these planes fit
    base = whisper_amd.xattn_check(*args, Tq, H, 0, prec)
    err = np.abs(base.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"B={B} Tq={Tq} T={T} H={H} prec={prec} small={small}: err {err:.3e}")
    assert err <= (5e-3 if prec == wq4.PREC_F16 else 2e-5), err
    live_mb = B * T * ns * D * 2 / 1e6
    splits, ch = whisper_amd.xattn_plan(T)
    for budget, lo, hi in (("0", 0, 0), (repr(0.42 * live_mb), 1, 63), ("1000000", 64, 64)):
        monkeypatch.setenv(ENV, budget)
        share = whisper_amd.xattn_resident_share(B, T, ns, D)
        assert lo <= share <= hi, (budget, share)
        if lo == 1:  # both policies among the sub-chunks, and inside one workgroup's walk where it has more than one
            res = [whisper_amd.xattn_chunk_resident(c, share) for c in range((T + 15) // 16)]
            assert any(res) and not all(res)
            if ch > 1:
                assert any(0 < sum(res[s * ch:(s + 1) * ch]) < len(res[s * ch:(s + 1) * ch]) for s in range(splits))
        got = whisper_amd.xattn_check(*args, Tq, H, 0, prec)
        assert torch.equal(got, base), (budget, (got - base).abs().max().item())


FIRST, NB_CLIPS, STEPS = 300, 16, 12


@pytest.fixture(scope="module")
def model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=NB_CLIPS)
    yield m
    m.close()


@pytest.fixture(scope="module")
def x2(torch):
    m = np.stack([np.stack([wo.synthetic_mel(FIRST + i * NB_CLIPS + c, 80) for c in range(NB_CLIPS)])
                  for i in range(2)])
    return torch.from_numpy(m).cuda()


def pair_live_mb(model):
    cfg = model.config
    return 2 * NB_CLIPS * cfg["n_audio_ctx"] * 2 * cfg["n_audio_state"] * 2 / 1e6


def test_pair_under_partial_share_equals_sequential(model, x2, monkeypatch):
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    monkeypatch.delenv(ENV, raising=False)
    seq = [model.transcribe(x2[i], 50259, max_tokens=STEPS, eot_stop=False) for i in range(2)]
    monkeypatch.setenv(ENV, repr(0.4 * pair_live_mb(model)))
    got = model.transcribe_batches(x2, 50259, max_tokens=STEPS, eot_stop=False)
    assert model.pipeline_pairs() == 1
    assert got == seq


def test_share_is_part_of_the_graph_key(model, x2, monkeypatch):
    """The share is baked into the captured step graph.  With a budget of 0.6
    of the pair's planes one batch alone (half the pair's bytes live) keeps
    everything resident and the pair 38 / 64: the pair counts the clips of both
    lanes, and the same pair at another share captures a new graph."""
    import whisper_amd

    den = whisper_amd.XATTN_SHARE_DEN
    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    monkeypatch.setenv(ENV, repr(0.6 * pair_live_mb(model)))
    model.transcribe(x2[0], 50259, max_tokens=4)
    alone = model.decode_graph_key(0)
    assert alone >= 0 and alone % (den + 1) == den
    model.transcribe_batches(x2, 50259, max_tokens=4)
    assert model.pipeline_pairs() == 1
    pair = model.decode_graph_key(0)
    assert pair != alone and pair % (den + 1) == 38
    assert model.decode_graph_key(1) % (den + 1) == 38
    monkeypatch.setenv(ENV, "1000000")
    model.transcribe_batches(x2, 50259, max_tokens=4)
    full = model.decode_graph_key(0)
    assert full != pair and full % (den + 1) == den and full // (den + 1) == pair // (den + 1)
