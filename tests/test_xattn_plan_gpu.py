"""The cross-attention under every frame split a decode may be given
(wa_xattn.hip xattn_plan: 1 .. 8 splits, chosen per decode unit from the CUs
it has; WA_XATTN_SPLITS_RT forces the count in wa_xattn_check and where a
decode's plan is decided).  One launch at S = 1 .. 8 against the float64
reference of tests/test_xattn_gpu.py, within the project's own bounds (2e-5 of
max|ref| for f16x2, 5e-3 for f16); S = 8 is the default plan bit for bit; under
a fixed plan a row's bits do not depend on the rows it is batched with; the
plan is part of a decode group's graph key; paired pipelined transcribes under
a forced plan return the sequential run's tokens (tests/plan_child.py)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import whisper_oracle as wo
import wq4

pytestmark = pytest.mark.gpu

ENV = "WA_XATTN_SPLITS_RT"
HERE = os.path.dirname(os.path.abspath(__file__))


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


# (B, Tq, T, H): Large-V3 rows; 9 rows (the fused kernel) over 13 sub-chunks --
# S = 6 normalises to 5 splits, S = 7 to 7 splits of 2 with a short last one;
# 3 sub-chunks -- every S >= 3 clamps
SHAPES = [(3, 1, 1500, 20), (9, 1, 200, 6), (1, 1, 37, 20)]
_cases = {}


def case(torch, shape):
    """Inputs on the device and the float64 reference, computed once per shape."""
    if shape not in _cases:
        B, Tq, T, H = shape
        D = 64 * H
        rng = np.random.default_rng(1000 * B + T + H)
        enc = rng.standard_normal((B, T, D)).astype(np.float32)
        q = (2.0 * rng.standard_normal((B * Tq, D))).astype(np.float32)
        wk = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
        wv = rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32)
        bv = rng.uniform(-0.02, 0.02, D).astype(np.float32)
        rk, rv = wq4.quantize_q4_0(wk), wq4.quantize_q4_0(wv)
        ref = reference(q, oracle.dequantize_np(rk, D * D).reshape(D, D),
                        oracle.dequantize_np(rv, D * D).reshape(D, D), bv, enc, Tq, H)
        args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, rk, rv, bv, enc)]
        _cases[shape] = (args, ref)
    return _cases[shape]


@pytest.mark.parametrize("prec", [wq4.PREC_F16X2, wq4.PREC_F16])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_split_matches_reference(torch, monkeypatch, shape, prec):
    import whisper_amd

    B, Tq, T, H = shape
    args, ref = case(torch, shape)
    tol = 5e-3 if prec == wq4.PREC_F16 else 2e-5
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv("WA_XATTN_SMALL_ROWS", raising=False)
    base = whisper_amd.xattn_check(*args, Tq, H, 0, prec)
    for S in range(1, 9):
        monkeypatch.setenv(ENV, str(S))
        got = whisper_amd.xattn_check(*args, Tq, H, 0, prec)
        err = np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max()
        print(f"B={B} Tq={Tq} T={T} H={H} prec={prec} S={S}: err {err:.3e}")
        assert err <= tol, (S, err)
        if S == 8:
            assert torch.equal(got, base)


def test_rows_independent_under_a_fixed_plan(torch, monkeypatch):
    """tests/test_xattn_gpu.py test_xattn_rows_independent at S = 7 with 9 rows
    (the fused kernel): the same 9 rows in another order give every row the
    same bits."""
    import whisper_amd

    H, D, T, R = 20, 1280, 1500, 9
    rng = np.random.default_rng(9)
    enc = torch.from_numpy(rng.standard_normal((R, T, D)).astype(np.float32)).cuda()
    q = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).cuda()
    rk = torch.from_numpy(wq4.quantize_q4_0(rng.uniform(-0.05, 0.05, (D, D)).astype(np.float32))).cuda()
    bv = torch.zeros(D, device="cuda")
    monkeypatch.setenv(ENV, "7")
    full = whisper_amd.xattn_check(q, rk, rk, bv, enc, 1, H)
    perm = torch.tensor([4, 8, 0, 6, 2, 7, 1, 5, 3], device="cuda")
    again = whisper_amd.xattn_check(q[perm].contiguous(), rk, rk, bv, enc[perm].contiguous(), 1, H)
    assert torch.equal(again[4:5], full[2:3])  # row 2, now fifth of the nine
    assert torch.equal(again, full[perm])


FIRST, NB_CLIPS = 300, 16


def key_splits(key):
    import whisper_amd

    return key // (whisper_amd.XATTN_SHARE_DEN + 1) % 16


def test_plan_is_part_of_the_graph_key(torch, monkeypatch):
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    monkeypatch.delenv("WA_XATTN_RESIDENT_MB", raising=False)
    monkeypatch.delenv(ENV, raising=False)
    mel = np.stack([np.stack([wo.synthetic_mel(FIRST + i * NB_CLIPS + c, 80) for c in range(NB_CLIPS)])
                    for i in range(2)])
    x2 = torch.from_numpy(mel).cuda()
    m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=NB_CLIPS)
    try:
        m.transcribe_batches(x2, 50259, max_tokens=4)
        assert m.pipeline_pairs() == 1
        k8 = [m.decode_graph_key(g) for g in (0, 1)]
        assert [key_splits(k) for k in k8] == [8, 8]
        monkeypatch.setenv(ENV, "5")
        m.transcribe_batches(x2, 50259, max_tokens=4)
        k5 = [m.decode_graph_key(g) for g in (0, 1)]
        assert [key_splits(k) for k in k5] == [5, 5] and k5[0] != k8[0] and k5[1] != k8[1]
        m.transcribe_batches(x2, 50259, max_tokens=4)  # an equal plan: the same graphs
        assert [m.decode_graph_key(g) for g in (0, 1)] == k5
        monkeypatch.delenv(ENV)
        m.transcribe_batches(x2, 50259, max_tokens=4)
        assert [m.decode_graph_key(g) for g in (0, 1)] == k8
    finally:
        m.close()


def test_pipeline_under_forced_plans_equals_sequential():
    env = dict(os.environ)
    for k in ("WA_ENC_OVERLAP", "WA_XATTN_RESIDENT_MB", "WA_PAIR_BATCHES", ENV):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "plan_child.py")], env=env, capture_output=True, text=True,
                       timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["sequential_splits"] == [8, 8]
    for run in out["runs"]:
        assert run["pairs"] == run["batches"] // 2, run
        assert run["splits"] == [run["forced"]] * 2, run
        assert run["equal"], run
        assert run["plain_after_splits"] == [8, 8], run
        assert run["plain_after_equal"], run
