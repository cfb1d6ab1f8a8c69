"""The argument combinations the unified check entries newly accept or reject
(include/whisper_amd_checks.h).  Every call gets real tensors, sized so that
even a wrongly accepted call stays in bounds."""
from __future__ import annotations

import numpy as np
import pytest

import wq4

pytestmark = pytest.mark.gpu

V, EOT, TS0 = 51866, 50257, 50365


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def test_self_attention_modes(torch):
    import whisper_amd

    R, H, ctx, kv_len = 3, 2, 8, 5
    g = torch.Generator(device="cuda:0").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda:0")
    qkv, qkv2 = rnd(R, 3 * 64 * H), rnd(2 * R, 3 * 64 * H)
    ck, cv = rnd(R, H, ctx, 64), rnd(R, H, ctx, 64)
    anc = torch.arange(R, dtype=torch.int32, device="cuda:0").repeat_interleave(ctx).reshape(R, ctx).contiguous()
    with pytest.raises(wq4.WQ4Error):  # the reindexed kernel has no Tq
        whisper_amd.self_attention_check(qkv2, ck.clone(), cv.clone(), 2, H, kv_len, anc=anc)
    with pytest.raises(wq4.WQ4Error):  # pad past kv_len
        whisper_amd.self_attention_check(qkv, ck.clone(), cv.clone(), 1, H, kv_len, pad=[6, 0, 0])
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.self_attention_check(qkv, ck.clone(), cv.clone(), 1, H, kv_len, anc=anc, pad=[6, 0, 0])
    k1, v1, k2, v2 = ck.clone(), cv.clone(), ck.clone(), cv.clone()
    want = whisper_amd.self_attention_check(qkv, k1, v1, 1, H, kv_len)
    got = whisper_amd.self_attention_check(qkv, k2, v2, 1, H, kv_len, wq4.PREC_F16X2, anc=None, pad=None,
                                           f32_out=False)
    assert torch.equal(got, want) and torch.equal(k1, k2) and torch.equal(v1, v2)
    assert not torch.equal(k1, ck)  # the row's key went into the cache


def test_embed_without_pad(torch):
    import whisper_amd

    B, Tq, D, Vs, ctx = 2, 1, 128, 64, 8
    g = torch.Generator(device="cuda:0").manual_seed(12)
    te = torch.randn(Vs, D, generator=g, device="cuda:0")
    pe = torch.randn(ctx + 2, D, generator=g, device="cuda:0")[2:]  # rows to spare before position 0
    assert pe.is_contiguous()
    want = whisper_amd.embed_check([5, 63], te, pe, B, Tq, 3)[0]
    got = whisper_amd.embed_check([5, 63], te, pe, B, Tq, 3, pad=None)[0]
    assert torch.equal(got, want)
    assert torch.equal(want, te[[5, 63]] + pe[3])
    with pytest.raises(wq4.WQ4Error):  # pad past pos0
        whisper_amd.embed_check([5, 63], te, pe, B, Tq, 3, pad=[4, 0])


@pytest.fixture(scope="module")
def rows(torch):
    g = torch.Generator(device="cuda:0").manual_seed(13)
    z = torch.randn(2, V, generator=g, device="cuda:0")
    z[0, EOT] = 9.0  # row 0 picks EOT unless it is masked
    return z


def test_beam_topk_without_rules(torch, rows):
    import whisper_amd

    kp = 3
    rec = np.stack([whisper_amd.timestamp_rule([], TS0, V)] * 2)
    mass = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    with pytest.raises(wq4.WQ4Error):  # records need a ts0
        whisper_amd.beam_topk_check(rows, kp, records=rec, ts0=0, mass=mass)
    with pytest.raises(wq4.WQ4Error):  # and so does a list
        whisper_amd.beam_topk_check(rows, kp, ids=[7], ts0=0)
    tok, lp, flag = whisper_amd.beam_topk_check(rows, kp)
    tok2, lp2, flag2 = whisper_amd.beam_topk_check(rows, kp, ids=(), ts0=0, records=None, mass=None)
    assert torch.equal(tok, tok2) and torch.equal(lp, lp2) and flag == flag2 == 0
    assert int(tok[0, 0]) == EOT


@pytest.mark.parametrize("suppress_eot", [False, True])
def test_row_pick_greedy_is_argmax_and_row_logprob(torch, rows, suppress_eot):
    import whisper_amd

    buf = torch.full((2,), 7.5, device="cuda:0")
    tok, lp, mass = whisper_amd.row_pick_check(rows, suppress_eot=suppress_eot, logprob=buf)
    assert lp is buf and mass is None
    masked = rows.clone()
    if suppress_eot:
        masked[:, EOT] = float("-inf")
    assert torch.equal(tok.long(), masked.argmax(1))
    assert (int(tok[0]) == EOT) != suppress_eot
    want = whisper_amd.row_logprob_check(rows, 0, V, mask_eot=suppress_eot, idx=tok)
    assert torch.equal(lp, want)
    tok0, lp0, _ = whisper_amd.row_pick_check(rows, suppress_eot=suppress_eot, scored=False)
    assert lp0 is None and torch.equal(tok0, tok)
