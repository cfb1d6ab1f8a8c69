"""The four attention kernels against float64 on planted softmax patterns
(attn_ref.py: the score and value families, the per-element bounds and their
derivation; test_attn_ref.py: the bounds' teeth on the CPU), through the
check entries, at the smallest shapes at which each path still runs.  Every
output element is compared with its own bound; every test prints its worst
error / bound.

The axes are covered as a covering set, not as their full product:
every (H, T) pair of the cache-free form and every (T, Tq) pair of the K / V
form is a case, the other axes (rows, weight format, precision, split count,
small-rows path) rotate over the cases so that each value meets each kernel
shape several times, and the families rotate over heads and rows inside
every case.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest

import attn_ref as A
import oracle
import wq4

pytestmark = pytest.mark.gpu

PREC = {"f16x2": wq4.PREC_F16X2, "f16": wq4.PREC_F16}


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hold(kernel, prec, label, got, ref, bound, names):
    """Every element within its bound; prints the worst error / bound and, on
    failure, names the (row, head, family) of the worst element."""
    bad, worst = A.violations(got, ref, bound)
    print(f"ATTN_WORST {kernel} {prec} {worst:.3f}  {label}")
    if bad.any():
        r = np.abs(np.asarray(got, np.float64) - ref) / bound
        r = np.where(np.isfinite(r), r, np.inf)
        row, col = np.unravel_index(np.argmax(r), r.shape)
        raise AssertionError(f"{label}: {int(bad.sum())} elements outside the bound, worst error / bound {worst:.3g} at "
                             f"row {row}, head {col // 64}, dim {col % 64} ({names(row, col // 64)}): got {got[row, col]!r}, "
                             f"reference {ref[row, col]!r}, bound {bound[row, col]:.3g}")


# ------------------------------------------- cache-free cross-attention --
@functools.lru_cache(maxsize=None)
def weights(H, wtype):
    return A.xattn_weights(H, wtype, 3 + H, wq4.quantize_q4_0, oracle.dequantize_np)


def _xattn_cases():
    cases = []
    for i, (H, T) in enumerate(itertools.product((20, 16, 12, 8, 6), (1, 15, 16, 17, 37, 203))):
        R = (1, 3, 5, 33)[i % 4]
        if R == 33 and T > 37 and H > 6:
            R = 5  # 33 rows at T = 203 only at the narrow model: the reference stays quick
        cases.append((R, 1, T, H, 1 if i % 5 == 4 else 0, "f16" if i % 3 == 2 else "f16x2", (1, 3, 7, 8)[(i // 4 + i) % 4], "unit"))
    cases += [
        (1, 4, 203, 20, 0, "f16x2", 7, "unit"),    # the prompt's Tq = 4, both head tiles
        (2, 4, 17, 6, 1, "f16x2", 8, "unit"),
        (33, 1, 37, 20, 0, "f16x2", 3, "unit"),    # the second 32-row group of xattn_q at two head tiles
        (1, 1, 1500, 20, 0, "f16x2", 8, "unit"),   # the whole clip, once: ramp_up and creep over 94 sub-chunks
        (1, 1, 203, 20, 0, "f16x2", 8, "tiny"),    # |enc| about 2^-10: every lo half under the flush threshold
        (1, 1, 203, 20, 0, "f16x2", 8, "large"),   # max |enc| = 2000, inside the planes' |x| < 2047
        (5, 1, 37, 6, 0, "f16x2", 3, "tiny"),
        (5, 1, 37, 6, 0, "f16", 3, "large"),
    ]
    return cases


XATTN_CASES = _xattn_cases()


def _xattn_id(c):
    B, Tq, T, H, wtype, prec, S, scale = c
    return f"B{B}-Tq{Tq}-T{T}-H{H}-{'f16w' if wtype else 'q4'}-{prec}-S{S}-{scale}"


def xattn_inputs(B, Tq, T, H, wtype, prec, S, scale, shift=0):
    import whisper_amd

    w = weights(H, wtype)
    sp = A.xattn_splits(T, S, whisper_amd.xattn_plan_splits)
    q, enc, names = A.xattn_case(B, Tq, T, H, w, 100 * H + T + B, sp[1][0] if len(sp) > 1 else A.XATTN_TC, shift + T + H, scale)
    ref, bound = A.xattn_ref(q, w["wk"], w["wv"], w["bv"], enc, Tq, H, prec)
    return w, q, enc, names, ref, bound, sp


def xattn_call(torch, w, q, enc, Tq, H, wtype, prec):
    import whisper_amd

    return whisper_amd.xattn_check(cu(torch, q), cu(torch, w["rk"]), cu(torch, w["rv"]), cu(torch, w["bv"]), cu(torch, enc),
                                   Tq, H, wtype, PREC[prec]).cpu().numpy()


@pytest.mark.parametrize("case", XATTN_CASES, ids=[_xattn_id(c) for c in XATTN_CASES])
def test_xattn_planted(torch, monkeypatch, case):
    """xattn_q / xattn_main / xattn_out and, for up to 8 rows, xattn_scores +
    xattn_z: each path within the bound, and the two bit-identical."""
    B, Tq, T, H, wtype, prec, S, scale = case
    w, q, enc, names, ref, bound, sp = xattn_inputs(*case)
    monkeypatch.setenv("WA_XATTN_SPLITS_RT", str(S))
    label = _xattn_id(case)
    monkeypatch.setenv("WA_XATTN_SMALL_ROWS", "0")
    fused = xattn_call(torch, w, q, enc, Tq, H, wtype, prec)
    hold("xattn", prec, label + " fused", fused, ref, bound, lambda row, h: names[row][h])
    if B * Tq <= 8:
        monkeypatch.setenv("WA_XATTN_SMALL_ROWS", "8")
        split = xattn_call(torch, w, q, enc, Tq, H, wtype, prec)
        hold("xattn", prec, label + " split-phase", split, ref, bound, lambda row, h: names[row][h])
        assert np.array_equal(fused, split), np.abs(fused - split).max()


@pytest.mark.parametrize("prec", A.PRECS)
def test_xattn_planted_residency_bit_identical(torch, monkeypatch, prec):
    """WA_XATTN_RESIDENT_MB = 0 (all nontemporal), a partial share and large
    (all default) load the same values: bit-identical on planted inputs, on
    both paths."""
    import whisper_amd

    B, Tq, T, H = 3, 1, 203, 20
    w, q, enc, names, ref, bound, _ = xattn_inputs(B, Tq, T, H, 0, prec, 8, "unit", shift=5)
    ns = 1 if prec == "f16" else 2
    live_mb = B * T * ns * 64 * H * 2 / 1e6
    partial = 0.45 * live_mb
    share = whisper_amd.xattn_resident_share(B, T, ns, 64 * H, partial)
    assert 0 < share < whisper_amd.XATTN_SHARE_DEN
    for small in ("0", "8"):
        monkeypatch.setenv("WA_XATTN_SMALL_ROWS", small)
        outs = []
        for mb in ("0", f"{partial:.4f}", "100000"):
            monkeypatch.setenv("WA_XATTN_RESIDENT_MB", mb)
            outs.append(xattn_call(torch, w, q, enc, Tq, H, 0, prec))
        hold("xattn", prec, f"residency small_rows={small}", outs[0], ref, bound, lambda row, h: names[row][h])
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_xattn_marker_names_the_frame(torch, monkeypatch):
    """enc column 0 carries the frame index and Wv's first row picks it out, so
    a spike's output names the frame that was picked -- at the first and last
    frame of every split of the 8-way plan."""
    import whisper_amd

    H, T, D = 6, 203, 384
    w = dict(weights(H, 1))
    wv = np.zeros((D, D), np.float16)
    wv[np.arange(D), np.arange(D)] = 1.0  # V = enc + bv
    w["rv"], w["wv"] = wv.view(np.uint8).ravel(), wv.astype(np.float32)
    sp = A.xattn_splits(T, 8, whisper_amd.xattn_plan_splits)
    frames = sorted({t for a, b in sp for t in (a, b - 1)})
    rng = np.random.default_rng(7)
    B = len(frames)
    q = (2.0 * rng.standard_normal((B, H, 64)))
    enc = np.zeros((B, T, D))
    wk = w["wk"].astype(np.float64)
    for b, f in enumerate(frames):
        S = np.zeros((H, T))
        S[:, f] = A.SPIKE
        e0 = rng.standard_normal((T, D))
        G = np.array([wk[h * 64:(h + 1) * 64].T @ q[b, h] for h in range(H)])
        # the marker column is fixed first; the planting then works in the other columns
        G0 = G.copy()
        G0[:, 0] = 0.0
        e0[:, 0] = 0.0
        e = A.plant(G0, S - np.outer(G[:, 0], np.arange(T)) / 8.0, e0)
        e[:, 0] = np.arange(T)
        enc[b] = e
    q32, enc32 = q.reshape(B, D).astype(np.float32), enc.astype(np.float32)
    monkeypatch.setenv("WA_XATTN_SPLITS_RT", "8")
    got = xattn_call(torch, w, q32, enc32, 1, H, 1, "f16x2")
    ref, bound = A.xattn_ref(q32, w["wk"], w["wv"], w["bv"], enc32, 1, H)
    hold("xattn", "f16x2", "marker", got, ref, bound, lambda row, h: f"spike at frame {frames[row]}")
    picked = got[:, 0] - w["bv"][0]
    assert np.allclose(picked, frames, atol=1e-3), (picked, frames)


# ------------------------------------ cross-attention over cached K / V --
KV_CASES = [(T, Tq, (20, 6)[i % 2], ("f16x2", "f16")[(i // 2) % 2])
            for i, (T, Tq) in enumerate(itertools.product((1, 187, 188, 189, 376, 377, 1500), (1, 3, 4)))]
KV_CASES += [(189, 4, 20, "f16"), (377, 1, 6, "f16x2"), (1500, 4, 20, "f16x2"), (1, 1, 6, "f16")]


@pytest.mark.parametrize("T,Tq,H,prec", KV_CASES)
def test_xattn_kv_planted(torch, T, Tq, H, prec):
    import whisper_amd

    B = 1 if H == 20 else 3
    q, k, v, names = A.kv_case(B, Tq, T, H, 7 * T + Tq, shift=T + Tq)
    ref, bound = A.f32_ref(q, k, v, Tq, prec)
    got = whisper_amd.xattn_kv_check(cu(torch, q), cu(torch, k), cu(torch, v), Tq, PREC[prec]).cpu().numpy()
    hold("xattn_kv", prec, f"T{T} Tq{Tq} H{H}", got, ref, bound, lambda row, h: names[row // Tq][h][1][row % Tq] + "/" + names[row // Tq][h][0])
    # constant-1 value dimensions come out as 1, the marker dimension of a spike names its key
    for b in range(B):
        for h in range(H):
            vf, fams = names[b][h]
            for t in range(Tq):
                o = got[b * Tq + t, h * 64:(h + 1) * 64]
                if vf == "ones":
                    assert np.abs(o[32:] - 1.0).max() <= 1e-6, (b, h, t, o[32:])
                if vf == "marker" and fams[t].startswith("spike_") and prec == "f16x2":
                    key = int(np.argmax(A.family_scores(fams[t], T, *_kv_geometry(T), None)))
                    assert abs(o[0] - key) <= 1e-3 * max(1, key), (fams[t], o[0], key)


def _kv_geometry(T):
    rg = A.xkv_ranges(T)
    return rg[0][1], (rg[1][1] if len(rg) > 2 else rg[0][1])


# ----------------------------------------------------- encoder attention --
ENC_CASES = [(2, 6, T, prec) for T in (1, 31, 32, 33, 63, 64, 65, 100, 257) for prec in A.PRECS]
ENC_CASES += [(1, 6, 100, "f16x2"), (13, 20, 100, "f16x2"), (13, 20, 100, "f16")]  # the 4-wave and the 8-wave (260 workgroups) launcher


@pytest.mark.parametrize("B,H,T,prec", ENC_CASES)
def test_encoder_attention_planted(torch, B, H, T, prec):
    """A family per block of 16 queries: the two halves of every wave, and the
    waves of a workgroup, need different rescales (the wave-uniform skip)."""
    import whisper_amd

    qkv, names = A.encoder_case(B, T, H, 3 * T + B, shift=T)
    ref, bound = A.encoder_ref(qkv, B, T, H, prec)
    got = whisper_amd.encoder_attention_check(cu(torch, qkv), T, H, PREC[prec]).cpu().numpy()
    hold("encoder", prec, f"B{B} H{H} T{T}", got, ref, bound,
         lambda row, h: names[row // T][h][1][(row % T) // A.ENC_BLOCK] + "/" + names[row // T][h][0])


# ------------------------------------------------ decoder self-attention --
SELF_CASES = [(1, kv, (20, 6)[i % 2], prec) for i, kv in enumerate((0, 1, 15, 16, 17, 63, 64, 227)) for prec in A.PRECS]
SELF_CASES += [(Tq, kv, (20, 6)[i % 2], prec) for i, (Tq, kv) in enumerate(((4, 0), (3, 1), (4, 200), (2, 446))) for prec in A.PRECS]


@pytest.mark.parametrize("Tq,kv,H,prec", SELF_CASES)
def test_decoder_self_attention_planted(torch, Tq, kv, H, prec):
    """Families planted over the cached keys and the appended ones (spike_last:
    the spike on the key the query itself appends); the prompt's causal form
    on empty and non-empty caches; the cache append."""
    import whisper_amd

    B, D = 2, 64 * H
    qkv, ck, cv, k, v, names = A.self_case(B, Tq, kv, H, 11 * kv + Tq, shift=kv + Tq)
    q = qkv.reshape(B * Tq, 3, D)[:, 0]
    ref, bound = A.f32_ref(q, k, v, Tq, prec, kv)
    ck_dev, cv_dev = cu(torch, ck), cu(torch, cv)
    got = whisper_amd.self_attention_check(cu(torch, qkv), ck_dev, cv_dev, Tq, H, kv, PREC[prec]).cpu().numpy()
    hold("self", prec, f"Tq{Tq} kv{kv} H{H}", got, ref, bound, lambda row, h: names[row // Tq][h][1][row % Tq] + "/" + names[row // Tq][h][0])
    kc, vc = ck_dev.cpu().numpy(), cv_dev.cpu().numpy()
    # the new keys / values appended at kv .. kv + Tq - 1, nothing else touched
    assert np.array_equal(kc[:, :, :kv + Tq], k) and np.array_equal(vc[:, :, :kv + Tq], v)
    assert np.array_equal(kc[:, :, kv + Tq:], ck[:, :, kv + Tq:]) and np.array_equal(vc[:, :, kv + Tq:], cv[:, :, kv + Tq:])
