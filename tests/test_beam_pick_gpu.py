"""The beam search's per-row top-(K + 1) kernel (wa_beam_topk_check) and its
per-clip merge kernel (wa_beam_select_check) on planted data.

Top-k bound.  u = 2^-24.  The kernel's log-probability against float64 numpy
on its OWN f32 row: |lp - lp64| <= (R + 24) u max(1, |lp|), with R the longest
chain of f32 roundings in the sum as built (beam_topk_kernel): a thread takes
at most n = 4 ceil(V / 1024) + 2 elements (groups of four 256 groups apart,
then one of the up to 3 left over: 4 ceil(V / 1024) + 1) and each costs at most two
roundings (the rescale by a new maximum, the addition); then 6 shuffle joins
and 3 joins over the waves of at most three roundings each:
    R = 2 (4 ceil(V / 1024) + 2) + 27       (439 at V = 51866, 35 at V = 1000).
The 24 covers the rounding of v - m, expf, logf and the two final subtractions
(relative to |lp|, hence the max(1, |lp|)), as in test_scores_gpu.py.  The
leaders are planted 0.5 apart, >= 100 x the bound, so every row is compared
in full; exact ties are planted inside the top K + 1 and across its boundary.

Select: pairs and sums are multiples of 1/8, so both sides do the same exact
f32 additions and comparisons and everything the kernel writes -- guard bands
included -- equals the reference (beam_ref.select) bit for bit.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import beam_ref
import wq4

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def r_topk(V):
    return 2 * (4 * math.ceil(V / 1024) + 2) + 27


# ------------------------------------------------------------------ top-k --
@functools.lru_cache(maxsize=None)
def planted(V):
    """32 logit rows with 12 planted leaders each, 0.5 apart above the crowd
    (on the device once).  Row 0: leaders 2 and 3 tie exactly; row 1: for every
    kp of the tests the leaders kp and kp + 1 tie (all of 2 .. 10 equal in
    pairs is impossible, so row 1 ties leaders (2, 3), (6, 7), (9, 10)); row 2
    (V > EOT): EOT is the raw maximum; the others plain."""
    import torch

    rng = np.random.default_rng(V)
    z = (rng.standard_normal((32, V)) * 1.5).astype(np.float32)
    lead = np.stack([rng.choice(V - 1, 12, replace=False) for _ in range(32)])
    if V > EOT:
        lead[lead == EOT] = 17  # EOT is planted on purpose only
        lead[2, 0] = EOT
    for r in range(32):
        assert len(set(lead[r])) == 12
        z[r, lead[r]] = np.float32(20.0) - np.float32(0.5) * np.arange(12, dtype=np.float32)
    z[0, lead[0, 2]] = z[0, lead[0, 1]]
    for a in (1, 5, 8):  # 0-based leader a and a + 1 equal: ranks (2,3), (6,7), (9,10)
        z[1, lead[1, a + 1]] = z[1, lead[1, a]]
    return z, torch.from_numpy(z).cuda()


def expected(zrow, masked, kp):
    z = zrow.astype(np.float64)
    if masked and z.size > EOT:
        z[EOT] = -np.inf
    lp = beam_ref.log_softmax(z)
    ids, _ = beam_ref.topk_row(z, kp + 1)
    return ids, lp


@pytest.mark.parametrize("V", [51866, 1000])
@pytest.mark.parametrize("rows", [1, 5, 30, 32])
@pytest.mark.parametrize("kp", [2, 6, 9])
def test_topk_planted(torch, V, rows, kp):
    import whisper_amd

    z, z_dev = planted(V)
    bound_u = (r_topk(V) + 24) * U
    # (step, suppress_eot, eot_stop) -> is EOT masked
    modes = [((-1, True, True), True), ((-1, False, True), False), ((0, False, True), True),
             ((1, False, True), True), ((2, False, True), False), ((2, False, False), True)]
    for (step, sup, stop), masked in modes if V > EOT else modes[1:2]:
        tok = torch.full((rows * kp + GUARD,), -7, dtype=torch.int32, device="cuda")
        lp = torch.full((rows * kp + GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        _, _, flag = whisper_amd.beam_topk_check(z_dev[:rows], kp, step, sup, stop, tok, lp)
        assert flag == 0
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
        assert (tok[rows * kp:] == -7).all() and (lp[rows * kp:] == 12345.0).all()  # guard bands intact
        tok, lp = tok[:rows * kp].reshape(rows, kp), lp[:rows * kp].reshape(rows, kp).astype(np.float64)
        worst = 0.0
        for r in range(rows):
            ids, lp64 = expected(z[r], masked, kp)
            b = bound_u * np.maximum(1.0, np.abs(lp64[ids[:kp]]))
            # the gap behind the compared ranks: >= 100 x the bound (an exact tie across the boundary is
            # decided by the id rule: then the gap behind the tied pair)
            gap = lp64[ids[kp - 1]] - lp64[ids[kp]]
            if gap == 0.0:
                ids2, _ = beam_ref.topk_row(np.where(np.arange(V) == ids[kp], -np.inf, lp64), kp + 1)
                gap = lp64[ids2[kp - 1]] - lp64[ids2[kp]]
                assert ids[kp - 1] > ids[kp]  # the larger id is the one inside
            assert gap >= 100 * b.max(), (r, gap, b.max())
            assert list(tok[r]) == list(ids[:kp]), (r, step, tok[r], ids)
            err = np.abs(lp[r] - lp64[ids[:kp]])
            worst = max(worst, float((err / b).max()))
            assert (err <= b).all(), (r, err / U, b / U)
        print(f"V {V} rows {rows} kp {kp} step {step} sup {sup} stop {stop}: worst {worst:.3f} of the bound "
              f"({r_topk(V) + 24} u)")
        # planted rows
        a, b2 = sorted(np.flatnonzero(z[0] == z[0].max() - np.float32(0.5)))
        if kp >= 3:
            assert list(tok[0][1:3]) == [b2, a]  # a tie inside the top kp: the larger id first
        if rows > 2 and V > EOT:
            assert (tok[2][0] == EOT) == (not masked) and (masked == (EOT not in tok[2]))


def test_topk_row_bits_do_not_depend_on_position(torch):
    """At V = 51866 consecutive rows alternate between 16- and 8-byte alignment
    (and a view one float in has neither): a row's pairs are the same bits."""
    import whisper_amd

    _, z_dev = planted(51866)
    tok, lp, _ = whisper_amd.beam_topk_check(z_dev[:5], 6, 2)
    for r in range(5):
        t1, l1, _ = whisper_amd.beam_topk_check(z_dev[r:r + 1].clone(), 6, 2)
        assert torch.equal(t1[0], tok[r]) and torch.equal(l1[0], lp[r])
    flat = torch.empty(51866 + 1, device="cuda")
    flat[1:] = z_dev[3]
    t2, l2, _ = whisper_amd.beam_topk_check(flat[1:][None, :], 6, 2)
    assert torch.equal(t2[0], tok[3]) and torch.equal(l2[0], lp[3])


def test_topk_flags_non_finite_logits(torch):
    import whisper_amd

    z, z_dev = planted(1000)
    for bad in (np.inf, -np.inf, np.nan):
        x = z_dev[:5].clone()
        assert whisper_amd.beam_topk_check(x, 6)[2] == 0
        x[3, 777] = bad
        tok, lp, flag = whisper_amd.beam_topk_check(x, 6)
        assert flag == 1
        assert (tok.cpu().numpy() >= 0).all() and (tok.cpu().numpy() < 1000).all()
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.beam_topk_check(z_dev[:5], 10)
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.beam_topk_check(z_dev[:5, :12].contiguous(), 6)


# ----------------------------------------------------------------- select --
CTX = 24
KV0 = 3


def planted_pairs(rng, n_clips, K, step):
    """[rows][K + 1] distinct tokens and non-increasing log-probabilities in
    multiples of 1/8.  Clip 0 sees EOT often and at any rank (above, between and
    below the kept beams); the others rarely."""
    rows = n_clips * K
    tok = np.zeros((rows, K + 1), np.int32)
    lp = np.zeros((rows, K + 1), np.float32)
    for r in range(rows):
        tok[r] = rng.choice(np.arange(100, 140), K + 1, replace=False)
        lp[r] = -np.sort(rng.integers(0, 24, K + 1)) / 8.0
        if step > 0 and rng.random() < 0.12:
            tok[r, rng.integers(0, K + 1)] = EOT
    if step == 1:  # clip 0: EOT in front of everything, and as the weakest candidate of the last beam
        tok[0, 0], lp[0, 0] = EOT, 0.0
        if K > 1:
            tok[K - 1, K], lp[K - 1, K] = EOT, -3.0
    if step in (2, 3):  # clip 0: every beam's EOT far ahead of its other candidates -- K finish at once, twice
        tok[:K, 0], lp[:K, 0] = EOT, 0.0
        lp[:K, 1:] -= 64.0
        tok[:K, 1:] = np.where(tok[:K, 1:] == EOT, 99, tok[:K, 1:])
    return tok, lp


@pytest.mark.parametrize("K", [1, 3, 5, 8])
@pytest.mark.parametrize("n_clips", [1, 2, 4])
@pytest.mark.parametrize("extra", [0, 2])
def test_select_matches_reference(torch, K, n_clips, extra):
    import whisper_amd

    C = min(16, K + extra)
    rows = n_clips * K
    rng = np.random.default_rng(K * 100 + n_clips * 10 + extra)
    shapes = {"top_tok": (rows * (K + 1), np.int32), "top_lp": (rows * (K + 1), np.float32), "S": (rows, np.float32),
              "next_tok": (rows, np.int32), "parent": (rows, np.int32), "anc": (2 * rows * CTX, np.int32),
              "fed": (CTX * rows, np.int32), "fin_sum": (n_clips * C, np.float32), "fin_len": (n_clips * C, np.int32),
              "fin_anc": (n_clips * C * CTX, np.int32), "fin_n": (n_clips, np.int32),
              "complete": (n_clips, np.int32), "state": (4, np.int32)}
    ref = {k: np.full(n + GUARD, -3, dt) for k, (n, dt) in shapes.items()}
    ref["S"][:rows] = -np.inf
    ref["S"][:rows:K] = 0.0
    ref["anc"][:2 * rows * CTX] = np.tile(np.repeat(np.arange(rows), CTX), 2)
    ref["fin_n"][:n_clips] = 0
    ref["complete"][:n_clips] = 0
    ref["state"][:4] = [KV0 + 1, KV0, -1, 0]  # position one ahead (the auto-detect quirk), kv_len, step, n_done
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in ref.items()}
    seen = {"above": 0, "between": 0, "below": 0, "overflow": 0, "lonely": 0}
    for step in range(8):
        tok, lp = planted_pairs(rng, n_clips, K, step)
        ref["top_tok"][:tok.size], ref["top_lp"][:lp.size] = tok.ravel(), lp.ravel()
        dev["top_tok"][:tok.size] = torch.from_numpy(tok.ravel()).cuda()
        dev["top_lp"][:lp.size] = torch.from_numpy(lp.ravel()).cuda()
        whisper_amd.beam_select_check(dev, n_clips, K, C, CTX)
        # the reference step
        pos, kv, st, _ = (int(x) for x in ref["state"][:4])
        anc = ref["anc"][:2 * rows * CTX].reshape(2, rows, CTX)
        cur, nxt = anc[(st + 1) & 1], anc[st & 1]
        fed = ref["fed"][:CTX * rows].reshape(CTX, rows)
        fin_anc = ref["fin_anc"][:n_clips * C * CTX].reshape(n_clips, C, CTX)
        for c in range(n_clips):
            r0 = c * K
            f0, was = int(ref["fin_n"][c]), bool(ref["complete"][c])
            sel = beam_ref.select(ref["S"][r0:r0 + K], tok[r0:r0 + K], lp[r0:r0 + K], K, C, f0, was, EOT)
            live_eot = int(((tok[r0:r0 + K] == EOT) & (ref["S"][r0:r0 + K, None] + lp[r0:r0 + K] > -np.inf)).sum())
            for e, (j, s) in enumerate(sel["filed"]):
                ref["fin_sum"][c * C + f0 + e], ref["fin_len"][c * C + f0 + e] = s, st + 1
                fin_anc[c, f0 + e, :kv + 1] = cur[r0 + j, :kv + 1]
            new_rows = np.stack([cur[r0 + p, :kv + 1] for p in sel["parent"]])
            nxt[r0:r0 + K, :kv + 1] = new_rows
            nxt[r0:r0 + K, kv + 1] = np.arange(r0, r0 + K)
            fed[kv + 1, r0:r0 + K] = sel["next_tok"]
            ref["S"][r0:r0 + K] = sel["S"]
            ref["next_tok"][r0:r0 + K] = sel["next_tok"]
            ref["parent"][r0:r0 + K] = [r0 + p for p in sel["parent"]]
            ref["fin_n"][c], ref["complete"][c] = sel["fin_n"], int(sel["complete"])
            # what the planted data exercised
            kinds = [x[3] == EOT for x in sel["order"]]
            if kinds and kinds[0]:
                seen["above"] += 1
            if any(kinds[1:]):
                seen["between"] += 1
            if live_eot > sum(kinds):  # an EOT candidate behind the walk: not met
                seen["below"] += 1
            if not was and f0 + sum(kinds) > C:
                seen["overflow"] += 1
        ref["state"][:4] = [pos + 1, kv + 1, st + 1, int(ref["complete"][:n_clips].sum())]
        if n_clips > 1 and 0 < ref["complete"][:n_clips].sum() < n_clips:
            seen["lonely"] += 1
        for k in shapes:
            got = dev[k].cpu().numpy()
            assert np.array_equal(got, ref[k], equal_nan=True), (step, k, np.flatnonzero(got != ref[k])[:8])
    print(f"K {K} clips {n_clips} C {C}: {seen}, finished {ref['fin_n'][:n_clips].tolist()}")
    if K >= 3:
        assert seen["above"] and seen["between"] and seen["below"]
        assert seen["overflow"] or extra  # C = K: 1 + K finish by step 2; a wider list may fill exactly
    if K >= 3 and n_clips > 1:
        assert seen["lonely"]  # a clip completed while a neighbour went on
