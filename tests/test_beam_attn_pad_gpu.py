"""The beam step's self-attention in the pad form of a prompted beam call
(wa_self_attention_beam_pad_check): row r attends slots [pad[r], kv_len] through
its ancestor table, the waves splitting the keys from pad[r].  The order of
operations is that of the pad kernel of a prompted greedy step
(wa_self_attention_pad_check), so every comparison is bit for bit:

  (a) the operand form against wa_self_attention_pad_check on caches gathered
      by torch through random in-clip tables (a kernel that ignores the table,
      or the pad, fails here);
  (b) the f32-row form of range tier 3 (wa_self_attention_pad_check has no such
      form): against this kernel with an identity table on the gathered caches
      -- (a) ties that to the pad kernel in the operand form -- and, on rows
      with pad 0, against the f32 form of the unpadded kernel on the gathered
      caches;
  (c) the caches whole, before and after: exactly slot (r, kv_len) changed.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_beam_attn_gpu as tba
import wq4

pytestmark = pytest.mark.gpu

ROWS, K = 6, 3


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("H", [6, 20])
@pytest.mark.parametrize("kv_len", [4, 37, 447])
def test_beam_pad_self_attention_bits(torch, H, kv_len, ns):
    import whisper_amd

    qkv, ck, cv, anc, ident = tba.case(H, ROWS, K)
    D = 64 * H
    prec = tba.PREC[ns]
    kg, vg = tba.gathered(torch, ck, anc), tba.gathered(torch, cv, anc)
    plain = whisper_amd.self_attention_beam_check(qkv, ck.clone(), cv.clone(), anc, H, kv_len, prec)
    for p0, p1 in ((0, 3), (4, 4), (kv_len, 0)):
        pad = np.repeat(np.array([p0, p1], np.int32), K)  # the rows of a clip share its prompt
        # (a) the operand form
        want = whisper_amd.self_attention_pad_check(qkv, kg.clone(), vg.clone(), H, kv_len, pad, prec)
        k2, v2 = ck.clone(), cv.clone()
        got = whisper_amd.self_attention_beam_pad_check(qkv, k2, v2, anc, pad, H, kv_len, prec)
        assert torch.equal(got, want), (p0, p1)
        zero = torch.from_numpy(pad == 0).cuda()
        assert torch.equal(got[zero], plain[zero])  # pad 0: the unpadded beam kernel's bits
        assert not torch.equal(got[~zero], plain[~zero])  # the pad matters
        # (c) exactly slot (r, kv_len) of every row changed, to the row's new key / value
        for new, old, part in ((k2, ck, 1), (v2, cv, 2)):
            exp = old.clone()
            exp[:, :, kv_len, :] = qkv[:, part * D:(part + 1) * D].reshape(ROWS, H, 64)
            assert torch.equal(new, exp)
        # (b) the f32-row form
        got32 = whisper_amd.self_attention_beam_pad_check(qkv, ck.clone(), cv.clone(), anc, pad, H, kv_len, prec,
                                                          f32_out=True)
        want32 = whisper_amd.self_attention_beam_pad_check(qkv, kg.clone(), vg.clone(), ident, pad, H, kv_len, prec,
                                                           f32_out=True)
        assert torch.equal(got32, want32) and torch.isfinite(got32).all()
        flat32 = whisper_amd.self_attention_beam_check(qkv, kg.clone(), vg.clone(), None, H, kv_len, prec, f32_out=True)
        assert torch.equal(got32[zero], flat32[zero])
        assert not torch.equal(got32[~zero], flat32[~zero])
    if kv_len >= 37:  # the table matters: the identity's result differs
        pad = np.repeat(np.array([0, 3], np.int32), K)
        a = whisper_amd.self_attention_beam_pad_check(qkv, ck.clone(), cv.clone(), anc, pad, H, kv_len, prec)
        b = whisper_amd.self_attention_beam_pad_check(qkv, ck.clone(), cv.clone(), ident, pad, H, kv_len, prec)
        assert not torch.equal(a, b)


def test_beam_pad_self_attention_rejects_bad_arguments(torch):
    import whisper_amd

    qkv, ck, cv, anc, _ = tba.case(6, ROWS, K)
    for pad in ([0, 0, 0, 6, 6, 6], [-1, 0, 0, 0, 0, 0]):  # pad outside [0, kv_len]
        with pytest.raises(wq4.WQ4Error):
            whisper_amd.self_attention_beam_pad_check(qkv, ck.clone(), cv.clone(), anc, pad, 6, 5)
    bad = anc.clone()
    bad[2, 3] = ROWS
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.self_attention_beam_pad_check(qkv, ck.clone(), cv.clone(), bad, [0] * ROWS, 6, 5)
