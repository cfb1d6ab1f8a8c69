"""The beam search's kernels under the timestamp rules on planted data: the
per-row top-(K + 1) (wa_beam_topk_rules_check) and the per-clip merge with the
rows' rule records (wa_beam_select_rules_check).  The rules' reference is
ts_rules.py, the merge's beam_ref.select.

Top-k bound.  u = 2^-24.  The rules kernel walks the row twice; the second walk
is the plain kernel's (beam_topk_kernel) over the finally masked row, and the
log-probabilities come from it alone, so the chain of f32 roundings is the one
counted in test_beam_pick_gpu.py for the kernel as built:
    R = 2 (4 ceil(V / 1024) + 2) + 27          (439 at V = 51866 and 51865)
and |lp - lp64| <= (R + 24) u max(1, |lp|) against float64 numpy on the kernel's
OWN f32 row.  The first walk only decides rule f, logsumexp(timestamps) against
max(text, EOT); its sum has the same walk and the same joins, so the same
(R + 24) u max(1, |lse|) bounds its error, and every row's rule-f margin on the
float64 reference is asserted >= 100 x that: no row is left out.  The leaders
are planted 0.5 apart (>= 100 x the bound); exact ties sit inside the top K + 1
and across its boundary.

Rows: one per record kind -- first pick with max_initial 50, 0 and -1, text
last, timestamp + timestamp, text + timestamp, text + timestamp with t_last =
V - 1 (allowed set {EOT, V - 1}) -- rule f planted not to fire (rows 0 .. 6) and
to fire (rows 7 .. 13) where the row has two sides, then the same again.

Merge: pairs and sums are multiples of 1/8, so everything the kernel writes --
guard bands included -- equals the reference bit for bit; the records equal
ts_rules.record of the reindexed histories.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import beam_ref
import beam_ts_ref as btr
import ts_rules as tr
import wq4

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
GUARD = 64
A = 1000  # a text id
KINDS = 7


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def r_topk(V):
    return 2 * (4 * math.ceil(V / 1024) + 2) + 27


def ts0_of(V):
    return {51866: 50365, 51865: 50364}[V]


def kind_of(r, V):
    """(history, max_initial) of row r."""
    ts0 = ts0_of(V)
    t = lambda k: ts0 + k  # noqa: E731
    return [([], 50), ([], 0), ([], -1), ([t(10), A], 50), ([t(10), A, t(20), t(20)], 50), ([t(10), A, t(20)], 50),
            ([t(10), A, V - 1], 50)][r % KINDS]


# ------------------------------------------------------------------ top-k --
@functools.lru_cache(maxsize=None)
def planted(V):
    """32 logit rows (on the device once), their histories and max_initial.  Per
    row 12 leaders 0.5 apart from 20 down on ids the row's rules allow (fewer
    where the allowed set is smaller), on the text side where rule f is planted
    not to fire and on the timestamp side where it is planted to fire; the
    other side's best id sits at 12.  After text + timestamp the text side is
    EOT alone: it sits at 24 (not to fire) or at 12.  Ties: rows of kind 3
    tie leaders (1, 2); rows of kinds 2 and 4 tie (1, 2), (5, 6), (8, 9), a
    pair across the boundary of every kp of the tests."""
    import torch

    ts0 = ts0_of(V)
    rng = np.random.default_rng(V)
    z = (rng.standard_normal((32, V)) * 1.5).astype(np.float32)
    hist, mi = [], []
    for r in range(32):
        h, m = kind_of(r, V)
        hist.append(h)
        mi.append(m)
        fire = (r // KINDS) % 2 == 1
        rec = tr.record(h, ts0, V, m)
        ok = tr.allowed_from_record(rec, ts0, V, False)
        text = np.flatnonzero(ok[:EOT])
        ts = ts0 + np.flatnonzero(ok[ts0:])
        kind = r % KINDS
        if kind in (5, 6):  # the text side is EOT alone
            lead = rng.choice(ts, min(12, ts.size), replace=False)
            z[r, EOT] = 12.0 if fire else 24.0
        elif text.size and ts.size:  # kind 3
            main, other = (ts, text) if fire else (text, ts)
            lead = rng.choice(main, 12, replace=False)
            z[r, rng.choice(other)] = 12.0
        else:
            lead = rng.choice(ts if ts.size else text, min(12, max(ts.size, text.size)), replace=False)
        assert len(set(lead)) == lead.size
        z[r, lead] = np.float32(20.0) - np.float32(0.5) * np.arange(lead.size, dtype=np.float32)
        if kind == 3:
            z[r, lead[2]] = z[r, lead[1]]
        if kind in (2, 4):
            for a in (1, 5, 8):
                z[r, lead[a + 1]] = z[r, lead[a]]
    return z, torch.from_numpy(z).cuda(), hist, mi


@functools.lru_cache(maxsize=None)
def expected(V, r, masked):
    """(ids in the kernel's order, float64 log-probabilities of the finally
    masked row, allowed ids, rule f fired, its margin, the logsumexp it compares)."""
    z, _, hist, mi = planted(V)
    ts0 = ts0_of(V)
    z64 = z[r].astype(np.float64)
    ae = tr.masks_ae(z64, hist[r], ts0, masked, mi[r])
    zz, fired, _ = tr.apply_rules(z64, hist[r], ts0, masked, mi[r])
    lp = beam_ref.log_softmax(zz)
    ids, _ = beam_ref.topk_row(zz, 11)
    return ids, lp, int(np.isfinite(zz).sum()), fired, btr.rule_f_margin(ae, ts0), tr.lse(ae[ts0:])


@pytest.mark.parametrize("V", [51866, 51865])
@pytest.mark.parametrize("rows", [1, 5, 32])
@pytest.mark.parametrize("kp", [2, 6, 9])
def test_topk_rules_planted(torch, V, rows, kp):
    import whisper_amd

    z, z_dev, hist, mi = planted(V)
    ts0 = ts0_of(V)
    bound_u = (r_topk(V) + 24) * U
    rec = np.array([tr.record(hist[r], ts0, V, mi[r]) for r in range(rows)], np.int32)
    # (step, suppress_eot, eot_stop) -> mask a
    modes = [((-1, True, True), True), ((-1, False, True), False), ((1, False, True), True),
             ((2, False, True), False), ((2, False, False), True)]
    fired_seen = set()
    for (step, sup, stop), masked in modes:
        tok = torch.full((rows * kp + GUARD,), -7, dtype=torch.int32, device="cuda")
        lp = torch.full((rows * kp + GUARD,), 12345.0, dtype=torch.float32, device="cuda")
        mass = torch.full((rows + GUARD,), -7, dtype=torch.int32, device="cuda")
        _, _, _, flag = whisper_amd.beam_topk_rules_check(z_dev[:rows], kp, rec, ts0, step, sup, stop, tok, lp, mass)
        assert flag == 0
        tok, lp, mass = tok.cpu().numpy(), lp.cpu().numpy(), mass.cpu().numpy()
        assert (tok[rows * kp:] == -7).all() and (lp[rows * kp:] == 12345.0).all() and (mass[rows:] == -7).all()
        tok, lp = tok[:rows * kp].reshape(rows, kp), lp[:rows * kp].reshape(rows, kp).astype(np.float64)
        worst = 0.0
        for r in range(rows):
            ids, lp64, n_ok, fired, m_f, lse_ts = expected(V, r, masked)
            # rule f decides with room on every row
            assert m_f >= 100 * bound_u * max(1.0, abs(lse_ts)), (r, m_f)
            assert mass[r] == int(fired), (r, step, mass[r], fired)
            if r % KINDS in (3, 5, 6) and not masked:
                fired_seen.add((r % KINDS, fired))
            n = min(kp, n_ok)
            b = bound_u * np.maximum(1.0, np.abs(lp64[ids[:n]]))
            if n_ok > kp:  # the gap behind the compared ranks (an exact tie across the boundary: behind the pair)
                gap = lp64[ids[kp - 1]] - lp64[ids[kp]]
                if gap == 0.0:
                    ids2, _ = beam_ref.topk_row(np.where(np.arange(V) == ids[kp], -np.inf, lp64), kp + 1)
                    gap = lp64[ids2[kp - 1]] - lp64[ids2[kp]]
                    assert ids[kp - 1] > ids[kp]  # the larger id is the one inside
                assert gap >= 100 * b.max(), (r, gap, b.max())
            assert list(tok[r][:n]) == list(ids[:n]), (r, step, tok[r], ids)
            err = np.abs(lp[r][:n] - lp64[ids[:n]])
            worst = max(worst, float((err / b).max()))
            assert (err <= b).all(), (r, err / U, b / U)
            # fewer allowed ids than kp: the surplus is (0, -inf), never NaN
            assert (lp[r][n:] == -np.inf).all() and (tok[r][n:] == 0).all(), (r, tok[r], lp[r])
        print(f"V {V} rows {rows} kp {kp} step {step} sup {sup} stop {stop}: worst {worst:.3f} of the bound "
              f"({r_topk(V) + 24} u)")
        if rows > 6:
            assert min(kp, expected(V, 6, masked)[2]) == (1 if masked else 2)  # {EOT, V - 1}
            assert expected(V, 1, masked)[2] == 1  # max_initial = 0: <|0.00|> alone
        if kp >= 3 and rows > 3:  # a tie inside the list: the larger id first
            a, b2 = sorted(np.flatnonzero(z[3] == np.float32(19.5)))
            assert list(tok[3][1:3]) == [b2, a]
    if rows == 32:  # each two-sided kind fired and did not
        assert fired_seen == {(k, f) for k in (3, 5, 6) for f in (False, True)}


def test_topk_rules_row_bits_do_not_depend_on_position(torch):
    import whisper_amd

    V = 51866
    _, z_dev, hist, mi = planted(V)
    ts0 = ts0_of(V)
    rec = np.array([tr.record(hist[r], ts0, V, mi[r]) for r in range(9)], np.int32)
    tok, lp, mass, _ = whisper_amd.beam_topk_rules_check(z_dev[:9], 6, rec, ts0, 2)
    for r in range(9):
        t1, l1, m1, _ = whisper_amd.beam_topk_rules_check(z_dev[r:r + 1].clone(), 6, rec[r:r + 1], ts0, 2)
        assert torch.equal(t1[0], tok[r]) and torch.equal(l1[0], lp[r]) and torch.equal(m1[0], mass[r])
    flat = torch.empty(V + 1, device="cuda")
    flat[1:] = z_dev[3]
    t2, l2, _, _ = whisper_amd.beam_topk_rules_check(flat[1:][None, :], 6, rec[3:4], ts0, 2)
    assert torch.equal(t2[0], tok[3]) and torch.equal(l2[0], lp[3])


def test_topk_rules_flag_and_arguments(torch):
    import whisper_amd

    V = 51866
    _, z_dev, hist, mi = planted(V)
    ts0 = ts0_of(V)
    rec = np.array([tr.record(hist[r], ts0, V, mi[r]) for r in range(5)], np.int32)
    for bad in (np.inf, -np.inf, np.nan):
        x = z_dev[:5].clone()
        x[0, 777] = bad  # a text id the row's rules mask (first pick): the flag reads the raw logits
        tok, lp, _, flag = whisper_amd.beam_topk_rules_check(x, 6, rec, ts0)
        assert flag == 1
        assert (tok.cpu().numpy() >= 0).all() and (tok.cpu().numpy() < V).all()
    for kp, t0 in ((10, ts0), (6, EOT), (6, V + 1)):
        with pytest.raises(wq4.WQ4Error):
            whisper_amd.beam_topk_rules_check(z_dev[:5], kp, rec, t0)


# ----------------------------------------------------------------- select --
CTX = 24
KV0 = 3
SEL_V, SEL_TS0 = 51866, 50365
POOL = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108, 109, SEL_TS0, SEL_TS0 + 5, SEL_TS0 + 40, SEL_TS0 + 41,
                 SEL_TS0 + 700, SEL_V - 1])


def planted_pairs(rng, n_clips, K, step):
    """[rows][K + 1] distinct tokens (text and timestamp ids) and non-increasing
    log-probabilities in multiples of 1/8.  Clip 0 is planted:
      step 0  (S = [0, -inf, ..]) every new beam continues beam 0;
      step 1  the best candidate comes from beam 1, the second from beam 0: beam
              0 <- parent 1, beam 1 <- parent 0, what an in-place update of the
              records would corrupt (K = 1: a plain step);
      step 2  beam 0 offers EOT first, then two tokens, then -inf, every other
              beam -inf alone: EOT is filed, beams 2 .. die (K = 1: EOT, then
              -inf: filed, and the beam dies).
    The other clips: random, a -inf tail and EOT now and then."""
    rows = n_clips * K
    tok = np.zeros((rows, K + 1), np.int32)
    lp = np.zeros((rows, K + 1), np.float32)
    for r in range(rows):
        tok[r] = rng.choice(POOL, K + 1, replace=False)
        lp[r] = -np.sort(rng.integers(0, 24, K + 1)) / 8.0
        if step > 0 and rng.random() < 0.2:
            tok[r, rng.integers(0, K + 1)] = EOT
        if r >= K and rng.random() < 0.3:  # (clip 0 keeps full rows: its plants need live beams)
            cut = rng.integers(1, K + 2)
            lp[r, cut:], tok[r, cut:] = -np.inf, 0
    if step == 1 and K > 1:
        lp[0] = -8.0 - np.arange(K + 1) / 8.0
        lp[1] = -32.0 * np.arange(K + 1)
        lp[2:K] = -200.0 - np.arange(K + 1) / 8.0
        for r in range(K):
            tok[r] = rng.choice(POOL, K + 1, replace=False)
    if step == 2:
        tok[:K], lp[:K] = 0, -np.inf
        tok[0, 0], lp[0, 0] = EOT, 0.0
        if K > 1:
            tok[0, 1:3], lp[0, 1:3] = (SEL_TS0 + 41, 103), (-1.0, -2.0)
    return tok, lp


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n_clips", [1, 3])
def test_select_rules_matches_reference(torch, K, n_clips):
    import whisper_amd

    C = K
    rows = n_clips * K
    rng = np.random.default_rng(K * 100 + n_clips * 10)
    shapes = {"top_tok": (rows * (K + 1), np.int32), "top_lp": (rows * (K + 1), np.float32), "S": (rows, np.float32),
              "next_tok": (rows, np.int32), "parent": (rows, np.int32), "anc": (2 * rows * CTX, np.int32),
              "fed": (CTX * rows, np.int32), "fin_sum": (n_clips * C, np.float32), "fin_len": (n_clips * C, np.int32),
              "fin_anc": (n_clips * C * CTX, np.int32), "fin_n": (n_clips, np.int32),
              "complete": (n_clips, np.int32), "state": (4, np.int32), "records": (rows * 8, np.int32)}
    ref = {k: np.full(n + GUARD, -3, dt) for k, (n, dt) in shapes.items()}
    ref["S"][:rows] = -np.inf
    ref["S"][:rows:K] = 0.0
    ref["anc"][:2 * rows * CTX] = np.tile(np.repeat(np.arange(rows), CTX), 2)
    ref["fin_n"][:n_clips] = 0
    ref["complete"][:n_clips] = 0
    ref["state"][:4] = [KV0, KV0, -1, 0]
    hist = [[] for _ in range(rows)]
    ref["records"][:rows * 8] = np.ravel([tr.record(h, SEL_TS0, SEL_V, 50) for h in hist])
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in ref.items()}
    plain = None
    seen = {"same_parent": 0, "swap": 0, "dead": 0, "filed": 0}
    for step in range(3):
        tok, lp = planted_pairs(rng, n_clips, K, step)
        ref["top_tok"][:tok.size], ref["top_lp"][:lp.size] = tok.ravel(), lp.ravel()
        dev["top_tok"][:tok.size] = torch.from_numpy(tok.ravel()).cuda()
        dev["top_lp"][:lp.size] = torch.from_numpy(lp.ravel()).cuda()
        if step == 1:  # the same step without records, through both entries: every output byte equal
            a = {k: v.clone() for k, v in dev.items() if k != "records"}
            b = {k: v.clone() for k, v in a.items()}
            whisper_amd.beam_select_check(a, n_clips, K, C, CTX)
            whisper_amd.beam_select_rules_check(b, n_clips, K, C, CTX, 0, 0)
            for k in a:
                assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
            plain = a
        whisper_amd.beam_select_rules_check(dev, n_clips, K, C, CTX, SEL_TS0, SEL_V)
        if step == 1:  # ... and the records change nothing else
            for k in plain:
                assert plain[k].cpu().numpy().tobytes() == dev[k].cpu().numpy().tobytes(), k
        # the reference step
        pos, kv, st, _ = (int(x) for x in ref["state"][:4])
        anc = ref["anc"][:2 * rows * CTX].reshape(2, rows, CTX)
        cur, nxt = anc[(st + 1) & 1], anc[st & 1]
        fed = ref["fed"][:CTX * rows].reshape(CTX, rows)
        fin_anc = ref["fin_anc"][:n_clips * C * CTX].reshape(n_clips, C, CTX)
        new_hist = list(hist)
        for c in range(n_clips):
            r0 = c * K
            f0, was = int(ref["fin_n"][c]), bool(ref["complete"][c])
            sel = beam_ref.select(ref["S"][r0:r0 + K], tok[r0:r0 + K], lp[r0:r0 + K], K, C, f0, was, EOT)
            for e, (j, s) in enumerate(sel["filed"]):
                ref["fin_sum"][c * C + f0 + e], ref["fin_len"][c * C + f0 + e] = s, st + 1
                fin_anc[c, f0 + e, :kv + 1] = cur[r0 + j, :kv + 1]
            nxt[r0:r0 + K, :kv + 1] = np.stack([cur[r0 + p, :kv + 1] for p in sel["parent"]])
            nxt[r0:r0 + K, kv + 1] = np.arange(r0, r0 + K)
            fed[kv + 1, r0:r0 + K] = sel["next_tok"]
            ref["S"][r0:r0 + K] = sel["S"]
            ref["next_tok"][r0:r0 + K] = sel["next_tok"]
            ref["parent"][r0:r0 + K] = [r0 + p for p in sel["parent"]]
            ref["fin_n"][c], ref["complete"][c] = sel["fin_n"], int(sel["complete"])
            for n in range(K):  # the histories follow the reindexing
                new_hist[r0 + n] = hist[r0 + sel["parent"][n]] + [sel["next_tok"][n]]
            live = [n for n in range(K) if sel["S"][n] > -np.inf]
            par = [sel["parent"][n] for n in live]
            seen["same_parent"] += len(set(par)) < len(par)
            seen["swap"] += K > 1 and sel["parent"][:2] == [1, 0] and len(live) >= 2
            seen["dead"] += len(live) < K
            seen["filed"] += len(sel["filed"]) > 0
        hist = new_hist
        ref["state"][:4] = [pos + 1, kv + 1, st + 1, int(ref["complete"][:n_clips].sum())]
        want_rec = np.array([tr.record(h, SEL_TS0, SEL_V, 50) for h in hist], np.int32)
        got_rec = dev["records"].cpu().numpy()
        assert (got_rec[rows * 8:] == -3).all()  # guard band
        got_rec = got_rec[:rows * 8].reshape(rows, 8)
        for r in range(rows):
            if ref["S"][r] > -np.inf:
                assert list(got_rec[r]) == list(want_rec[r]), (step, r, hist[r], got_rec[r], want_rec[r])
            else:  # a dead beam keeps a valid record
                assert got_rec[r][0] in (0, 1) and SEL_TS0 <= got_rec[r][1] <= SEL_V and got_rec[r][2] == SEL_V - 1
        ref["records"][:rows * 8] = got_rec.ravel()
        for k in shapes:
            got = dev[k].cpu().numpy()
            assert np.array_equal(got, ref[k], equal_nan=True), (step, k, np.flatnonzero(got != ref[k])[:8])
    print(f"K {K} clips {n_clips}: {seen}")
    assert seen["filed"] and seen["dead"]
    if K > 1:
        assert seen["same_parent"] and seen["swap"]


def test_select_rules_rejects_bad_arguments(torch):
    import whisper_amd

    d = {k: torch.zeros(64, dtype=torch.float32 if k in ("top_lp", "S", "fin_sum") else torch.int32, device="cuda")
         for k in list(whisper_amd.BEAM_SELECT_ARRAYS) + ["records"]}
    d["state"][:4] = torch.tensor([3, 3, -1, 0], dtype=torch.int32)
    for ts0, V in ((0, 100), (200, 100)):
        with pytest.raises(wq4.WQ4Error):
            whisper_amd.beam_select_rules_check(d, 1, 1, 1, 8, ts0, V)
