"""The prefill's two attention kernels (wa_transcribe_prompted) against float64
on planted softmax patterns, and the pad forms of the decode step's
self-attention and embedding against the unpadded kernels, bit for bit.

The prefill kernel runs encoder_attention_f16_kernel's arithmetic (f16-pair
MFMA operands at the same scales, 64-key tiles in two 32-key sub-tiles, the
lazy reference maximum), so the per-element bound is the one attn_ref.py
derives for the encoder self-attention: sdpa_ref(..., pair=True), with the
causal / pad visibility as its `vis` (the kernel differs from the encoder's in
adding the sub-tiles' parts with compensated sums, which only lowers the error;
test_prefill_ref.py shows on the CPU that the bound has teeth for this use:
DESIGN.md "Numerics").  Every block of 16 queries of a (clip,
head) shares a direction with its own score family planted in that head's
keys, as attn_ref.encoder_case does; a causal query then sees the family's
first keys.
"""
from __future__ import annotations

import numpy as np
import pytest

import attn_ref as A
import wq4

pytestmark = pytest.mark.gpu

PREC = {"f16x2": wq4.PREC_F16X2, "f16": wq4.PREC_F16}
SCORE_FAMILIES = ("spike_first", "spike_last", "ramp_up", "flat", "wide", "gauss", "just_over", "ramp_down")
H = 6
CTX = 448
# P -> the clips' prompt lengths n_b (n_b in {1, 4, 5, P}; 130 at P = 227: a
# padded clip of more than one key tile)
SELF_CASES = {5: (5, 1, 4), 17: (17, 4, 5), 64: (64, 1, 5), 65: (65, 5, 4), 227: (227, 4, 130)}


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def planted(n_q, n_k, seed, shift):
    """q [n_q, 64], k, v [n_k, 64] of one (clip, head) and the families' names."""
    rng = np.random.default_rng(seed)
    nb = -(-n_q // A.ENC_BLOCK)
    blk = np.arange(n_q) // A.ENC_BLOCK
    fams = [A.rotate(shift + j, SCORE_FAMILIES) for j in range(nb)]
    vf = A.rotate(shift, A.VALUE_FAMILIES)
    G = 2.0 * rng.standard_normal((nb, 64))
    G[[f == "flat" for f in fams]] = 0.0
    S = np.array([A.family_scores(f, n_k, A.ENC_SUB, 2 * A.ENC_SUB, rng) for f in fams])
    a = np.array([1.0 if fams[j] in A.THRESHOLD_FAMILIES else 1.0 - (t % A.ENC_BLOCK) / 160.0 for t, j in enumerate(blk)])
    k0 = rng.standard_normal((n_k, 64)) * (2.0**-10 if vf == "tiny" else 1.0)
    f = np.float32
    return (a[:, None] * G[blk]).astype(f), A.plant(G, S, k0).astype(f), A.values(vf, n_k, rng).astype(f), (vf, fams)


def hold(label, prec, got, ref, bound):
    bad, worst = A.violations(got, ref, bound)
    print(f"ATTN_WORST prefill {prec} {worst:.3f}  {label}")
    assert not bad.any(), f"{label}: {int(bad.sum())} elements outside the bound, worst error / bound {worst:.3g}"


def self_case(P, ns, seed, prec):
    """qkv [B P, 3 D] with clip b's n_b rows right-aligned (the pad rows hold
    large junk no real row may see), and per clip the float64 reference and
    bound of its own rows."""
    B, D = len(ns), 64 * H
    rng = np.random.default_rng(seed)
    qkv = (1000.0 * rng.standard_normal((B, P, 3, H, 64))).astype(np.float32)
    refs = []
    for b, n in enumerate(ns):
        ref, bound = np.zeros((n, H, 64)), np.zeros((n, H, 64))
        vis = np.tril(np.ones((n, n), bool))
        for h in range(H):
            q, k, v, _ = planted(n, n, seed * 1000 + b * H + h, b * H + h)
            qkv[b, P - n:, 0, h], qkv[b, P - n:, 1, h], qkv[b, P - n:, 2, h] = q, k, v
            ref[:, h], bound[:, h] = A.sdpa_ref(q, k, v, prec, True, vis)
        refs.append((ref.reshape(n, D), bound.reshape(n, D)))
    return qkv.reshape(B * P, 3 * D), refs


def run_self(torch, qkv, P, ns, prec, sentinel=None):
    import whisper_amd

    B = len(ns)
    pad = [P - n for n in ns]
    shape = (B, H, CTX, 64)
    ck = torch.full(shape, 7.0 if sentinel is None else sentinel, device="cuda", dtype=torch.float32)
    cv = torch.full(shape, -7.0 if sentinel is None else -sentinel, device="cuda", dtype=torch.float32)
    out = whisper_amd.self_attention_prefill_check(cu(torch, qkv), ck, cv, P, pad, H, PREC[prec])
    return out.cpu().numpy(), ck.cpu().numpy(), cv.cpu().numpy()


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("P", sorted(SELF_CASES))
def test_prefill_self_attention_planted(torch, P, prec):
    """Causal, ragged: every real row within the encoder kernel's bound, pad
    rows zero, K / V of the real rows in the caches bit for bit, every other
    cache slot untouched."""
    ns = SELF_CASES[P]
    qkv, refs = self_case(P, ns, 7 + P, prec)
    out, ck, cv = run_self(torch, qkv, P, ns, prec)
    D = 64 * H
    x = qkv.reshape(len(ns), P, 3, H, 64)
    for b, n in enumerate(ns):
        rows = out[b * P:(b + 1) * P]
        hold(f"self P{P} clip{b} n{n}", prec, rows[P - n:], *refs[b])
        assert not rows[:P - n].any(), "pad rows are written as zeros"
        assert np.array_equal(ck[b, :, P - n:P], x[b, P - n:, 1].transpose(1, 0, 2))
        assert np.array_equal(cv[b, :, P - n:P], x[b, P - n:, 2].transpose(1, 0, 2))
        for c, s in ((ck, 7.0), (cv, -7.0)):
            assert (c[b, :, :P - n] == s).all() and (c[b, :, P:] == s).all(), "slots outside [pad, P) survive"
    assert out.shape == (len(ns) * P, D)


@pytest.mark.parametrize("prec", A.PRECS)
def test_prefill_self_attention_clip_is_independent_of_its_padding(torch, prec):
    """A clip of 130 rows right-aligned in P = 227 beside other clips, and the
    same clip alone and unpadded: the same bits."""
    P, ns = 227, SELF_CASES[227]
    qkv, _ = self_case(P, ns, 7 + P, prec)
    out, _, _ = run_self(torch, qkv, P, ns, prec)
    D = 64 * H
    for b, n in enumerate(ns):
        alone = qkv.reshape(len(ns), P, 3 * D)[b, P - n:]
        got, ck, _ = run_self(torch, alone, n, (n,), prec)
        assert np.array_equal(got, out[b * P + P - n:(b + 1) * P]), f"clip {b} (n = {n})"


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("P,T", [(5, 1500), (17, 37), (64, 1500), (65, 37), (227, 1500), (227, 37)])
def test_prefill_cross_attention_planted(torch, P, T, prec):
    """Non-causal over T encoder frames (1500, and 37: no multiple of the key tile)."""
    import whisper_amd

    B, D = 3, 64 * H
    q, k, v = np.zeros((B, P, H, 64), np.float32), np.zeros((B, H, T, 64), np.float32), np.zeros((B, H, T, 64), np.float32)
    ref, bound = np.zeros((B, P, H, 64)), np.zeros((B, P, H, 64))
    for b in range(B):
        for h in range(H):
            q[b, :, h], k[b, h], v[b, h], _ = planted(P, T, 31 * P + T + b * H + h, b * H + h)
            ref[b, :, h], bound[b, :, h] = A.sdpa_ref(q[b, :, h], k[b, h], v[b, h], prec, True)
    got = whisper_amd.cross_attention_prefill_check(cu(torch, q.reshape(B * P, D)), cu(torch, k), cu(torch, v), P,
                                                    PREC[prec]).cpu().numpy()
    hold(f"cross P{P} T{T}", prec, got, ref.reshape(B * P, D), bound.reshape(B * P, D))
    # a clip alone: the same bits
    one = whisper_amd.cross_attention_prefill_check(cu(torch, q[1].reshape(P, D)), cu(torch, k[1:2]), cu(torch, v[1:2]), P,
                                                    PREC[prec]).cpu().numpy()
    assert np.array_equal(one, got[P:2 * P])


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("kv_len", [17, 40, 223])
def test_decode_step_pad_form_equals_the_shifted_clip(torch, kv_len, prec):
    """wa_self_attention_pad_check with pad = (0, 3, 17) equals, per clip,
    wa_self_attention_check on the clip's cache shifted down by pad_b with
    kv_len - pad_b entries."""
    import whisper_amd

    pad = (0, 3, 17)
    B, D = len(pad), 64 * H
    qkv, ck, cv, _, _, _ = A.self_case(B, 1, kv_len, H, 5 + kv_len)
    got = whisper_amd.self_attention_pad_check(cu(torch, qkv), cu(torch, ck), cu(torch, cv), H, kv_len, pad,
                                               PREC[prec]).cpu().numpy()
    for b, p in enumerate(pad):
        sk, sv = np.zeros((1, H, CTX, 64), np.float32), np.zeros((1, H, CTX, 64), np.float32)
        sk[0, :, :kv_len - p], sv[0, :, :kv_len - p] = ck[b, :, p:kv_len], cv[b, :, p:kv_len]
        tk, tv = cu(torch, sk), cu(torch, sv)
        want = whisper_amd.self_attention_check(cu(torch, qkv[b:b + 1]), tk, tv, 1, H, kv_len - p, PREC[prec]).cpu().numpy()
        assert np.array_equal(got[b:b + 1], want), f"clip {b}, pad {p}"
        # the appended key lands at the unshifted slot
        assert np.array_equal(tk.cpu().numpy()[0, :, kv_len - p], qkv[b, D:2 * D].reshape(H, 64))
    assert got.shape == (B, D)


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("use_state", [False, True])
def test_embedding_pad_form_equals_the_shifted_position(torch, use_state, fold):
    """The embedding's pad form against wa_embed_check at position pos0 - pad_b, per clip."""
    import whisper_amd

    rng = np.random.default_rng(3)
    V, D, pos0, pad = 300, 384, 40, (0, 3, 17)
    B = len(pad)
    te, pe = cu(torch, rng.standard_normal((V, D)).astype(np.float32)), cu(torch, rng.standard_normal((CTX, D)).astype(np.float32))
    gamma = cu(torch, rng.uniform(0.9, 1.1, D).astype(np.float32)) if fold else None
    tokens = rng.integers(0, V, B).astype(np.int32)
    x, tiled, stats = whisper_amd.embed_pad_check(tokens, te, pe, B, 1, pos0, pad, use_state, gamma)
    for b, p in enumerate(pad):
        wx, wt, ws = whisper_amd.embed_check(tokens[b:b + 1], te, pe, 1, 1, pos0 - p, use_state, gamma)
        assert torch.equal(x[b:b + 1], wx), f"clip {b}"
        if fold:
            assert torch.equal(stats[b:b + 1], ws)
    if fold:  # the operand of all rows at once, against the unpadded kernel fed the rows' own positions
        one = [whisper_amd.embed_check(tokens[b:b + 1], te, pe, 1, 1, pos0 - p, use_state, gamma)[0] for b, p in enumerate(pad)]
        assert torch.equal(x, torch.cat(one))
