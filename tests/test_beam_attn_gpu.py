"""The beam step's self-attention over a reindexed K/V cache
(wa_self_attention_beam_check) against the kernel it mirrors
(wa_self_attention_check): the order of operations is the same, so every
comparison is bit for bit.

  (a) an identity table on the same caches;
  (b) random tables, drawn within each clip's rows, against the existing kernel
      on caches gathered by torch according to the table (a kernel that ignores
      the table fails here);
  (c) the caches whole, before and after: exactly slot (r, kv_len) of every row
      changed, to the row's new key / value;
  (d) the f32-row form of range tier 3, against the existing kernel's.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import wq4

pytestmark = pytest.mark.gpu

CTX = 448
PREC = {1: wq4.PREC_F16, 2: wq4.PREC_F16X2}
KV_LENS = [0, 1, 3, 4, 37, 223, 447]


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@functools.lru_cache(maxsize=None)
def case(H, rows, K):
    """qkv rows, full caches and a random table per (H, rows): on the device
    once, never modified (the tests clone the caches)."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(H * 1000 + rows)
    qkv = torch.randn((rows, 3 * 64 * H), generator=g).cuda()
    ck = torch.randn((rows, H, CTX, 64), generator=g).cuda()
    cv = torch.randn((rows, H, CTX, 64), generator=g).cuda()
    # anc[r, j]: a row of r's clip, drawn per slot
    clip0 = (torch.arange(rows) // K * K)[:, None]
    anc = (clip0 + torch.randint(0, K, (rows, CTX), generator=g)).to(torch.int32).cuda()
    ident = torch.arange(rows, dtype=torch.int32)[:, None].repeat(1, CTX).contiguous().cuda()
    return qkv, ck, cv, anc, ident


def gathered(torch, cache, anc):
    """cache[r, h, j] <- cache[anc[r, j], h, j]: what OpenAI's rearrange_kv_cache leaves."""
    rows, H, ctx, _ = cache.shape
    j = torch.arange(ctx, device=cache.device)[None, :].expand(rows, ctx)
    return cache[anc.long(), :, j].permute(0, 2, 1, 3).contiguous()


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("H,rows,K", [(6, 6, 3), (20, 10, 5)])
@pytest.mark.parametrize("kv_len", KV_LENS)
def test_beam_self_attention_bits(torch, H, rows, K, kv_len, ns):
    import whisper_amd

    qkv, ck, cv, anc, ident = case(H, rows, K)
    D = 64 * H
    # (a) identity table
    k0, v0 = ck.clone(), cv.clone()
    want = whisper_amd.self_attention_check(qkv, k0, v0, 1, H, kv_len, PREC[ns])
    k1, v1 = ck.clone(), cv.clone()
    got = whisper_amd.self_attention_beam_check(qkv, k1, v1, ident, H, kv_len, PREC[ns])
    assert torch.equal(got, want)
    assert torch.equal(k1, k0) and torch.equal(v1, v0)
    # (b) a random table against the existing kernel on gathered caches
    kg, vg = gathered(torch, ck, anc), gathered(torch, cv, anc)
    want = whisper_amd.self_attention_check(qkv, kg, vg, 1, H, kv_len, PREC[ns])
    k2, v2 = ck.clone(), cv.clone()
    got = whisper_amd.self_attention_beam_check(qkv, k2, v2, anc, H, kv_len, PREC[ns])
    assert torch.equal(got, want)
    if kv_len >= 3:  # the table matters: the identity's result differs
        assert not torch.equal(got, whisper_amd.self_attention_beam_check(qkv, ck.clone(), cv.clone(), ident, H,
                                                                          kv_len, PREC[ns]))
    # (c) exactly slot (r, kv_len) of every row changed, to the row's new key / value
    for new, old, part in ((k2, ck, 1), (v2, cv, 2)):
        exp = old.clone()
        exp[:, :, kv_len, :] = qkv[:, part * D:(part + 1) * D].reshape(rows, H, 64)
        assert torch.equal(new, exp)
    # (d) the f32-row form
    want32 = whisper_amd.self_attention_beam_check(qkv, kg.clone(), vg.clone(), None, H, kv_len, PREC[ns], f32_out=True)
    got32 = whisper_amd.self_attention_beam_check(qkv, ck.clone(), cv.clone(), anc, H, kv_len, PREC[ns], f32_out=True)
    assert torch.equal(got32, want32)
    assert torch.isfinite(got32).all()


def test_beam_self_attention_rejects_bad_tables(torch):
    import whisper_amd

    qkv, ck, cv, anc, _ = case(6, 6, 3)
    bad = anc.clone()
    bad[2, 1] = 6
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.self_attention_beam_check(qkv, ck.clone(), cv.clone(), bad, 6, 5)
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.self_attention_beam_check(qkv, ck.clone(), cv.clone(), anc, 6, CTX)
