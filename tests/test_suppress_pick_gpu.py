"""Suppress-token lists in the pick kernels (wa_logits_suppress_check,
wa_row_suppress_check, wa_beam_topk_suppress_check; include/whisper_amd.h,
"Suppress-token lists") on planted data.  The reference adds one step to the
existing ones (suppress_ref.premask): the listed ids are -inf in the row before
ts_rules.py / sample_rules.py / beam_ref.py see it.

Planting and bounds are those of test_timestamps_gpu.py (orthogonal hidden rows
of norm 16, float64 logits), test_scores_gpu.py, test_sampling_gpu.py and
test_beam_rules_pick_gpu.py -- the list adds no f32 operation to a reduction,
a listed id is one more -inf term:
  margins   every row's decision margin on the float64 logits (top-2 gap of the
            allowed set / of the keys, |lse_ts - max_text|) is asserted >= 100 x
            the logit bound 4e-6 max|ref| + 1e-6 (single plane: >= 2 x the f16
            bound), so every row of every launch is compared;
  (i)       |lp - lp64| <= (R + 24) u on the kernel's OWN masked f32 row, R the
            count of the mode's file: fused scored 73, timestamps 77, sampled
            75 / 79; rows 9 + ceil(V / 256), 14 + ceil(ts0 / 256), 16 + ..;
            top-k (2 (4 ceil(V / 1024) + 2) + 27 + 24) u max(1, |lp|);
  (ii)      (i) plus twice the logit bound against the float64 logits.

The list of the launches is ALWAYS: an id at every boundary of the mask layout
(bit 0 / 31 of a word, the first / last word of a 128-id workgroup, EOT - 1,
EOT + 1, ts0 - 1) and two text ids.  Each boundary id is planted as a row's raw
maximum (20) beside its unsuppressed neighbour (12): an off-by-one bit index
suppresses the neighbour instead and the row's token is wrong.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import beam_ref
import beam_ts_ref as btr
import sample_rules as smp
import suppress_ref as sr
import test_beam_rules_pick_gpu as tbp
import test_sampling_gpu as tsg
import test_scores_gpu as tsc
import test_timestamps_gpu as tg
import ts_rules as tr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
V = 51866
TS0 = 50365
STEP = 5  # no EOT suppression; step 0 suppresses it
A0, FB, AF, NEXT = 1500, 5000, 1000, 3000  # the histories' text id, the fallback text, rule f's text pair
BOUNDARY = [0, 31, 32, 127, 128, EOT - 1, EOT + 1, TS0 - 1]
NEIGHBOUR = [1, 30, 33, 126, 129, EOT - 2, EOT, TS0]  # the planted winner beside each
ALWAYS = BOUNDARY + [AF, 2000]
FIRST = [220, EOT]


def T(k):
    return TS0 + k


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


# ---------------------------------------------------------- planted rows --
OPEN = [T(10), A0]  # text after a timestamp: text, EOT, or a timestamp > T(10)
# (history, {id: logit}).  Every row but 9 also plants FB at 10: whatever a
# mode masks of the planted pair, the row still decides with room.
PLANTS = [(OPEN, {s: 20.0, w: 12.0}) for s, w in zip(BOUNDARY[:6], NEIGHBOUR[:6])] + [
    # 6 EOT + 1 suppressed beside EOT; a special at 11 takes over where EOT is masked and specials are not
    (OPEN, {EOT + 1: 20.0, EOT: 12.0, EOT + 2: 11.0}),
    # 7 ts0 - 1 suppressed beside <|0.00|>, allowed after text with no timestamp yet
    ([A0], {TS0 - 1: 20.0, TS0: 12.0}),
    # 8 scored: the suppressed id leaves the normaliser (lp about 0, not about -8)
    (OPEN, {2000: 20.0, 2001: 12.0}),
    # 9 rule f: text AF = 16 suppressed, the next text id at 8, 200 timestamps at 8 (lse 13.3)
    (OPEN, {AF: 16.0, NEXT: 8.0, **{T(400 + i): 8.0 for i in range(200)}}),
    # 10, 11 pick 0 against a later pick: FIRST's ids are the best unsuppressed ones
    (OPEN, {32: 20.0, 220: 18.0, 221: 12.0}),
    (OPEN, {127: 20.0, EOT: 18.0, 5001: 12.0}),
    # 12 text + <|30.00|>: the allowed set under the rules is {EOT, V - 1}
    ([T(10), A0, V - 1], {0: 20.0, V - 1: 12.0, EOT: 8.0}),
]
NO_FB = (9,)
POOL = [A0, FB, EOT, TS0, T(1), T(40), T(700)]
# rows 13 .. 31: a random history over POOL, a boundary id at 20 and the fill of
# test_timestamps_gpu.py, which decides every rule state with room
FILL = {A0: 12.0, T(1400): 10.0, T(25): 8.0, EOT: 6.0}


def plant_of(r):
    if r < len(PLANTS):
        p = dict(PLANTS[r][1])
        if r not in NO_FB:
            p[FB] = 10.0
        return p
    return {BOUNDARY[r % 6]: 20.0, **FILL}


@functools.lru_cache(maxsize=None)
def planted_host(D):
    rng = np.random.default_rng(9000 + D)
    emb = (rng.uniform(-1, 1, (V, D)) * 0.03).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((D, 32)))
    unit = q.T  # [32, D], orthonormal rows
    hid = (unit * 16.0).astype(np.float32)
    rows = {}
    for r in range(32):
        for i, val in plant_of(r).items():
            rows.setdefault(i, np.zeros(D))
            rows[i] += unit[r] * (val / 16.0)
    for i, vec in rows.items():
        emb[i] = vec.astype(np.float32)
    hist = [list(p[0]) for p in PLANTS]
    for r in range(len(PLANTS), 32):
        hist.append([int(rng.choice(POOL)) for _ in range(int(rng.integers(0, 6)))])
    ref = hid.astype(np.float64) @ emb.astype(np.float64).T
    groups = {}  # bit-equal embedding rows: equal logits in any one arithmetic (test_timestamps_gpu.py)
    for i in rows:
        groups.setdefault(emb[i].tobytes(), []).append(i)
    for ids in groups.values():
        ref[:, ids] = ref[:, ids[:1]]
    absdot = np.abs(hid).astype(np.float64) @ np.abs(emb).astype(np.float64).T
    f16_bound = (2.0 ** -10 + 2.0 ** -20) * absdot.max(axis=1) + 1e-6
    return hid, emb, ref, hist, f16_bound


@functools.lru_cache(maxsize=None)
def planted(D):
    import torch

    hid, emb, _, _, _ = planted_host(D)
    return torch.from_numpy(hid).cuda(), torch.from_numpy(emb).cuda()


def top_gap(z):
    top = np.unique(z[np.isfinite(z)])[-2:]  # distinct values: bit-equal rows tie in every arithmetic
    return float(top[1] - top[0]) if top.size == 2 else np.inf


def plain_rows(ref, ids, B, suppress):
    """No rule records: the list, then the EOT mask -> (rows, tokens, margins)."""
    z = sr.premask(ref[:B], ids)
    if suppress:
        z[:, EOT] = -np.inf
    return z, np.array([tr.pick(z[b]) for b in range(B)]), np.array([top_gap(z[b]) for b in range(B)])


def logit_bounds(D, B, prec, margins):
    _, _, ref, _, f16b = planted_host(D)
    lb = 4e-6 * np.abs(ref[:B]).max(axis=1) + 1e-6
    assert (margins >= 100 * lb).all(), (margins, lb)
    if prec == 1:  # one f16 plane: the format's own bound
        lb = f16b[:B]
        assert (margins >= 2 * lb).all(), (margins, lb)
    return lb


def check_lp(name, lp, lg, tok, want, wtok, R, lb):
    B = len(tok)
    lg64 = lg.astype(np.float64)
    b1 = (R + 24) * U
    err_i = np.abs(lp - (lg64[np.arange(B), tok] - tg.lse_rows(lg64)))
    err_ii = np.abs(lp - (want[np.arange(B), wtok] - tg.lse_rows(want)))
    bound_ii = b1 + 2 * lb
    print(f"{name}: (i) {err_i.max() / U:.1f} u of {b1 / U:.0f} u, (ii) {(err_ii / bound_ii).max():.3f} of its bound")
    assert (err_i <= b1).all(), (name, err_i / U)
    assert (err_ii <= bound_ii).all(), (name, err_ii, bound_ii)


def check_mask(lg, raw, want):
    """-inf exactly where the reference masks, the kernel's own raw logit elsewhere."""
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(lg), fin)
    assert np.array_equal(lg[fin], raw[fin])


# ----------------------------------------------------------------- fused --
@pytest.mark.parametrize("prec", [0, 1])  # PREC_F16X2 (NS = 2), PREC_F16 (NS = 1)
@pytest.mark.parametrize("D", [128, 384])
def test_fused_greedy_and_scored(torch, D, prec):
    """B = 32 and 3 (padded rows), with and without the EOT suppression."""
    import whisper_amd

    hid_d, emb_d = planted(D)
    _, _, ref, _, _ = planted_host(D)
    for B in (32, 3):
        h = hid_d[:B].contiguous()
        _, raw = whisper_amd.logits_argmax_check(h, emb_d, 40, precision=prec)  # no mask at step 40
        raw = raw.cpu().numpy()
        for step in (STEP, 0):
            want, wtok, margins = plain_rows(ref, ALWAYS, B, step + 1 < 3)
            lb = logit_bounds(D, B, prec, margins)
            gtok, _, glg, _ = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, precision=prec,
                                                                scored=False)
            tok, lp, lg, _ = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, precision=prec)
            tok, lp, lg = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), lg.cpu().numpy()
            assert np.array_equal(gtok.cpu().numpy(), wtok) and np.array_equal(tok, wtok), (tok, wtok)
            assert not np.isin(tok, ALWAYS).any()
            assert glg.cpu().numpy().tobytes() == lg.tobytes()
            check_mask(lg, raw, want)
            if step == STEP:  # the unsuppressed neighbour wins; without the list the boundary id does
                n = min(B, len(BOUNDARY))
                assert tok[:n].tolist() == NEIGHBOUR[:n]
                ctok, clp, _, _ = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, precision=prec)
                assert ctok.cpu().numpy()[:n].tolist() == BOUNDARY[:n]
                # row 8: the suppressed 20.0 is outside the normaliser -- the winner at 12 against FB at
                # 10 and the background's mass (about e^10.9): -0.4, "about 0"; with it inside: about -8
                if B > 8:
                    assert abs(lp[8]) < 1.0 and tok[8] == 2001
                    assert ctok[8] == 2000 and clp[8] > -0.01
                    assert abs(ref[8, 2001] - ref[8, 2000] + 8.0) < 1e-3
            check_lp(f"scored D {D} B {B} step {step} prec {prec}", lp, lg, tok, want, wtok, tsc.r_fused(V), lb)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("D", [128, 384])
def test_fused_timestamps(torch, D, prec):
    """Under rule records: the list before masks a-e, rule f over what both
    leave.  Row 9's rule fires only because of the list (mass = 1, a timestamp
    wins); the same row without the list picks AF."""
    import whisper_amd

    hid_d, emb_d = planted(D)
    _, _, ref, hist, _ = planted_host(D)
    for B in (32, 3):
        h = hid_d[:B].contiguous()
        _, raw = whisper_amd.logits_argmax_check(h, emb_d, 40, precision=prec)
        raw = raw.cpu().numpy()
        for step in (STEP, 0):
            want, wtok, wfired, margins = tg.rule_rows(sr.premask(ref[:B], ALWAYS), hist, B, step)
            lb = logit_bounds(D, B, prec, margins)
            tok, lp, lg, mass = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, histories=hist[:B],
                                                                  precision=prec)
            lg[mass.bool(), :TS0] = float("-inf")  # rule f's mask where the kernel reports it
            tok, lp, lg, mass = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), lg.cpu().numpy(), mass.cpu().numpy()
            assert np.array_equal(tok, wtok), (tok, wtok)
            assert np.array_equal(mass != 0, wfired)
            assert not np.isin(tok, ALWAYS).any()
            check_mask(lg, raw, want)
            if B > 9:
                assert mass[9] == 1 and tok[9] == T(599)
                ctok, _, _, cmass = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, histories=hist[:B],
                                                                      precision=prec)
                assert ctok[9] == AF and cmass[9] == 0
                assert wfired.sum() < B  # not every row fires
            check_lp(f"timestamps D {D} B {B} step {step} prec {prec}", lp, lg, tok, want, wtok, tg.r_fused(), lb)


def masked_row(z, hist, step, records):
    """The float64 row a pick sees after the list: (row, rule f fired, rule f's margin)."""
    return tsg.masked_row(sr.premask(z, ALWAYS), hist, step, records)


@functools.lru_cache(maxsize=None)
def seeds_for(D, records, picks, row_form=False):
    """Per row the first seed from 1000 r on under which, at T = 1 and every
    pick index of `picks`: the float64 keys of the row under the list keep a
    top-2 gap >= 200 x the key bound (and 4 x the single-plane one), and --
    without records -- the draw WITHOUT the list lands on the row's suppressed
    raw maximum."""
    _, _, ref, hist, f16b = planted_host(D)
    lb = 4e-6 * np.abs(ref).max(axis=1) + 1e-6
    out = []
    for r in range(32):
        s = 1000 * r
        while True:
            ok = True
            for p in picks:
                step = (0 if p == 0 else STEP) if row_form else p - 1
                z, _, _ = masked_row(ref[r], hist[r], step, records)
                k = smp.keys(z, 1.0, s, p)
                kmax = np.abs(k[np.isfinite(k)]).max()
                gap = smp.key_gap(k)
                ok = ok and gap >= 200 * tsg.key_bound(lb[r], 1.0, kmax) and gap >= 4 * tsg.key_bound(f16b[r], 1.0, kmax)
                if ok and not records:
                    free, _, _ = tsg.masked_row(ref[r], hist[r], step, False)
                    ok = smp.pick(smp.keys(free, 1.0, s, p)) in ALWAYS
            if ok:
                break
            s += 1
            assert s < 1000 * r + 400, ("no seed meets the conditions", r)
        out.append(s)
    return np.array(out, np.uint64)


def sampled_reference(ref, hist, seeds, B, step, pick, records):
    rows, toks, fired, gaps, kmaxs, mm = [], [], [], [], [], []
    for b in range(B):
        z, f, m = masked_row(ref[b], hist[b], step, records)
        k = smp.keys(z, 1.0, int(seeds[b]), pick)
        rows.append(z)
        toks.append(smp.pick(k))
        fired.append(f)
        gaps.append(smp.key_gap(k))
        kmaxs.append(np.abs(k[np.isfinite(k)]).max())
        mm.append(m)
    return np.stack(rows), np.array(toks), np.array(fired), np.array(gaps), np.array(kmaxs), np.array(mm)


@pytest.mark.parametrize("records", [False, True])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("D", [128, 384])
def test_fused_sampled(torch, D, prec, records):
    """T = 1: the draw under the list is sample_rules' on the pre-masked row,
    with seeds whose list-free draw is the suppressed id.  T = 0: the bits of
    the scored / timestamp form under the list."""
    import whisper_amd

    hid_d, emb_d = planted(D)
    _, _, ref, hist, f16b = planted_host(D)
    seeds = seeds_for(D, records, (1, STEP + 1))
    for B in (32, 3):
        h = hid_d[:B].contiguous()
        hh = hist[:B] if records else None
        for step in (STEP, 0):
            want, wtok, wfired, gaps, kmaxs, mm = sampled_reference(ref, hist, seeds, B, step, step + 1, records)
            lb = 4e-6 * np.abs(ref[:B]).max(axis=1) + 1e-6
            kb = np.array([tsg.key_bound(lb[b], 1.0, kmaxs[b]) for b in range(B)])
            assert (gaps >= 100 * kb).all() and (mm >= 100 * lb).all(), (gaps, kb, mm)
            if prec == 1:
                lb = f16b[:B]
                kb = np.array([tsg.key_bound(lb[b], 1.0, kmaxs[b]) for b in range(B)])
                assert (gaps >= 2 * kb).all() and (mm >= 2 * lb).all(), (gaps, kb, mm)
            tok, lp, lg, mass = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, temperature=1.0,
                                                                  seed=seeds[:B], histories=hh, precision=prec)
            if records:
                lg[mass.bool(), :TS0] = float("-inf")
                assert np.array_equal(mass.cpu().numpy() != 0, wfired)
            tok, lp, lg = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), lg.cpu().numpy()
            assert np.array_equal(tok, wtok), (tok, wtok)
            assert not np.isin(tok, ALWAYS).any()
            assert np.array_equal(np.isfinite(lg), np.isfinite(want))
            if not records:  # the same seeds without the list: the suppressed id
                ftok, _, _, _ = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, temperature=1.0,
                                                                  seed=seeds[:B], precision=prec)
                assert np.isin(ftok.cpu().numpy(), ALWAYS).all()
            check_lp(f"sampled D {D} B {B} step {step} prec {prec} records {records}", lp, lg, tok, want, wtok,
                     tsg.r_fused(records), lb)
            # T = 0: the unsampled form under the list, bit for bit
            ztok, zlp, _, zmass = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, temperature=0.0,
                                                                    seed=seeds[:B], histories=hh, precision=prec)
            gtok, glp, _, gmass = whisper_amd.logits_suppress_check(h, emb_d, ALWAYS, step, TS0, histories=hh,
                                                                    precision=prec)
            assert torch.equal(ztok, gtok) and zlp.cpu().numpy().tobytes() == glp.cpu().numpy().tobytes()
            if records:
                assert torch.equal(zmass, gmass)


# ------------------------------------------------------------ stored rows --
@functools.lru_cache(maxsize=None)
def stored(D):
    import torch

    _, _, ref, hist, _ = planted_host(D)
    z32 = ref.astype(np.float32)
    return z32, torch.from_numpy(z32).cuda(), hist


@pytest.mark.parametrize("D", [128, 384])
def test_row_plain_and_timestamp(torch, D):
    """The planted logits stored as f32 rows: launch_argmax + launch_row_logprob
    (no records) and row_pick (records), n_rows 32 and 3."""
    import whisper_amd

    z32, zd, hist = stored(D)
    z64 = z32.astype(np.float64)
    for n in (32, 3):
        z = zd[:n].contiguous()
        for sup in (False, True):
            want, wtok, margins = plain_rows(z64, ALWAYS, n, sup)
            assert (margins >= 1e-2).all()
            tok, lp, mass = whisper_amd.row_suppress_check(z, ALWAYS, TS0, suppress_eot=sup)
            tok, lp = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
            assert mass is None and np.array_equal(tok, wtok), (tok, wtok)
            err = np.abs(lp - (want[np.arange(n), wtok] - tg.lse_rows(want)))
            assert (err <= (tsc.r_row(0, V) + 24) * U).all(), err / U
            if not sup:
                k = min(n, len(BOUNDARY))
                assert tok[:k].tolist() == NEIGHBOUR[:k]
            want, wtok, wfired, margins = tg.rule_rows(sr.premask(z64[:n], ALWAYS), hist, n, 0 if sup else STEP)
            assert (margins >= 1e-2).all()
            tok, lp, mass = whisper_amd.row_suppress_check(z, ALWAYS, TS0, suppress_eot=sup, histories=hist[:n])
            tok, lp, mass = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), mass.cpu().numpy()
            assert np.array_equal(tok, wtok) and np.array_equal(mass != 0, wfired)
            err = np.abs(lp - (want[np.arange(n), wtok] - tg.lse_rows(want)))
            assert (err <= (tg.r_row() + 24) * U).all(), err / U
            if n > 9:
                assert mass[9] == 1 and tok[9] == T(599)
                ctok, _, cmass = whisper_amd.row_suppress_check(z, [], TS0, suppress_eot=sup, histories=hist[:n])
                assert ctok[9] == AF and cmass[9] == 0


@pytest.mark.parametrize("records", [False, True])
def test_row_sampled(torch, records):
    import whisper_amd

    D = 128
    z32, zd, hist = stored(D)
    z64 = z32.astype(np.float64)
    seeds = seeds_for(D, records, (0, STEP + 1), True)
    for n in (32, 3):
        z = zd[:n].contiguous()
        hh = hist[:n] if records else None
        for pick, sup in ((0, True), (STEP + 1, False)):
            step = 0 if sup else STEP
            want, wtok, wfired, gaps, kmaxs, mm = sampled_reference(z64, hist, seeds, n, step, pick, records)
            kb = np.array([tsg.key_bound(0.0, 1.0, kmaxs[b]) for b in range(n)])
            assert (gaps >= 100 * kb).all() and (mm >= 1e-2).all()
            tok, lp, mass = whisper_amd.row_suppress_check(z, ALWAYS, TS0, suppress_eot=sup, pick=pick, temperature=1.0,
                                                           seed=seeds[:n], histories=hh)
            tok, lp = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
            assert np.array_equal(tok, wtok), (tok, wtok)
            assert np.array_equal(mass.cpu().numpy() != 0, wfired)
            err = np.abs(lp - (want[np.arange(n), wtok] - tg.lse_rows(want)))
            assert (err <= (tsg.r_row(records) + 24) * U).all(), err / U
            if not records:
                ftok, _, _ = whisper_amd.row_suppress_check(z, [], TS0, suppress_eot=sup, pick=pick, temperature=1.0,
                                                            seed=seeds[:n])
                assert np.isin(ftok.cpu().numpy(), ALWAYS).all()


def test_row_pick0_against_later_pick(torch):
    """Rows 10 and 11: with ids = always | first (pick 0) FIRST's ids lose to
    the next planted id; with ids = always (a later pick) they win."""
    import whisper_amd

    z32, zd, hist = stored(128)
    z64 = z32.astype(np.float64)
    z = zd[:12].contiguous()
    _, later, _ = plain_rows(z64, ALWAYS, 12, False)
    _, first, _ = plain_rows(z64, sr.union(ALWAYS, FIRST), 12, False)
    assert later[10:12].tolist() == [220, EOT] and first[10:12].tolist() == [221, 5001]
    for ids, want in ((ALWAYS, later), (sr.union(ALWAYS, FIRST), first)):
        tok, _, _ = whisper_amd.row_suppress_check(z, ids, TS0)
        assert np.array_equal(tok.cpu().numpy(), want)
        tok, _, _ = whisper_amd.row_suppress_check(z, ids, TS0, temperature=0.0, seed=1)
        assert np.array_equal(tok.cpu().numpy(), want)
    assert np.flatnonzero(later != first).tolist() == [6, 10, 11]  # row 6's winner is EOT itself


# ------------------------------------------------------------- beam top-k --
@functools.lru_cache(maxsize=None)
def beam_rows():
    """10 rows: per boundary id s a row with s at 22 and 12 leaders 0.5 apart
    from 20 down, the unsuppressed neighbour first, then text ids (row 7,
    whose neighbour is <|0.00|>: timestamps, with the best text id at 12), two
    more listed ids between them (19.75, 18.25); row 8 the rule-f pair of
    PLANTS[9]; row 9 text + <|30.00|>, whose allowed set under the rules is
    {EOT, V - 1} (EOT at 12 above <|30.00|> at 10: rule f stays quiet), with
    id 0 at 20 and text leaders from 11.5 down."""
    import torch

    rng = np.random.default_rng(77)
    z = (rng.standard_normal((10, V)) * 1.5).astype(np.float32)
    text = np.setdiff1d(np.arange(200, EOT - 200), ALWAYS + [A0, AF, NEXT])
    ladder = np.float32(0.5) * np.arange(12, dtype=np.float32)
    hist = []
    for r, (s, w) in enumerate(zip(BOUNDARY, NEIGHBOUR)):
        side = np.arange(T(100), T(1400)) if w >= TS0 else text
        lead = [w] + [int(i) for i in rng.choice(side, 11, replace=False)]
        z[r, lead] = np.float32(20.0) - ladder
        z[r, s] = 22.0
        z[r, BOUNDARY[(r + 1) % 6]] = 19.75
        z[r, BOUNDARY[(r + 2) % 6]] = 18.25
        if w >= TS0:
            z[r, NEXT] = 12.0
        hist.append([A0] if w >= TS0 else OPEN)
    z[8, AF], z[8, NEXT] = 16.0, 8.0
    z[8, T(400):T(600)] = 8.0
    hist.append(OPEN)
    z[9, 0], z[9, EOT], z[9, V - 1] = 20.0, 12.0, 10.0  # rule f does not fire
    z[9, rng.choice(text, 12, replace=False)] = np.float32(11.5) - ladder
    hist.append([T(10), A0, V - 1])
    return z, torch.from_numpy(z).cuda(), hist


@pytest.mark.parametrize("kp", [2, 6, 9])
@pytest.mark.parametrize("rules", [False, True])
def test_beam_topk(torch, kp, rules):
    import whisper_amd

    z, zd, hist = beam_rows()
    R = z.shape[0]
    bound_u = (tbp.r_topk(V) + 24) * U
    rec = np.array([tr.record(h, TS0, V) for h in hist], np.int32) if rules else None
    for (step, sup, stop), masked in (((-1, True, True), True), ((2, False, True), False), ((2, False, False), True)):
        tok, lp, mass, flag = whisper_amd.beam_topk_suppress_check(zd, kp, ALWAYS, TS0, rec, step, sup, stop)
        assert flag == 0
        tok, lp = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
        for r in range(R):
            zm = sr.premask(z[r].astype(np.float64), ALWAYS)
            if rules:
                ae = tr.masks_ae(zm, hist[r], TS0, masked)
                m_f = btr.rule_f_margin(ae, TS0)
                assert m_f >= 100 * bound_u * max(1.0, abs(tr.lse(ae[TS0:]))), (r, m_f)
                zz, fired, _ = tr.apply_rules(zm, hist[r], TS0, masked)
                assert mass[r] == int(fired)
            else:
                zz = zm.copy()
                if masked:
                    zz[EOT] = -np.inf
            lp64 = beam_ref.log_softmax(zz)
            ids, _ = beam_ref.topk_row(lp64, kp + 1)
            n_ok = int(np.isfinite(zz).sum())
            n = min(kp, n_ok)
            b = bound_u * np.maximum(1.0, np.abs(lp64[ids[:n]]))
            if n_ok > kp and lp64[ids[kp - 1]] != lp64[ids[kp]]:  # (equal values: the larger id is inside)
                assert lp64[ids[kp - 1]] - lp64[ids[kp]] >= 100 * b.max(), r
            assert tok[r][:n].tolist() == ids[:n].tolist(), (r, step, tok[r], ids)
            assert not np.isin(tok[r][:n], ALWAYS).any()
            assert (np.abs(lp[r][:n] - lp64[ids[:n]]) <= b).all(), r
            if rules:  # fewer allowed ids than kp: the surplus stays (0, -inf) though id 0 is listed
                assert (lp[r][n:] == -np.inf).all() and (tok[r][n:] == 0).all(), (r, tok[r], lp[r])
        if rules:
            assert mass[8] == 1 and (tok[8] >= T(400)).all()
            ctok, _, cmass, _ = whisper_amd.beam_topk_suppress_check(zd, kp, [], TS0, rec, step, sup, stop)
            assert cmass[8] == 0 and ctok[8, 0] == AF
            assert np.isfinite(lp[9]).sum() == min(kp, 1 if masked else 2)
        elif not masked:
            assert tok[:8, 0].tolist() == NEIGHBOUR


# ------------------------------------------------------------- empty list --
def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("prec", [0, 1])
def test_empty_list_returns_the_existing_entries_bytes(torch, prec):
    import whisper_amd

    D = 128
    hid_d, emb_d = planted(D)
    _, _, _, hist, _ = planted_host(D)
    seeds = np.arange(32, dtype=np.uint64) + 5
    temps = np.array([tsg.TEMPS[r % 3] for r in range(32)], np.float32)
    for B in (32, 3):
        h = hid_d[:B].contiguous()
        for step in (STEP, 0):
            t0, l0 = whisper_amd.logits_argmax_check(h, emb_d, step, precision=prec)
            t1, _, l1, _ = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, precision=prec, scored=False)
            assert same(t0, t1) and same(l0, l1)
            t0, p0, l0 = whisper_amd.logits_logprob_check(h, emb_d, step, precision=prec)
            t1, p1, l1, _ = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, precision=prec)
            assert same(t0, t1) and same(p0, p1) and same(l0, l1)
            t0, p0, l0, m0 = whisper_amd.logits_timestamp_check(h, emb_d, hist[:B], step, TS0, precision=prec)
            t1, p1, l1, m1 = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, histories=hist[:B],
                                                               precision=prec)
            l1[m1.bool(), :TS0] = float("-inf")
            assert same(t0, t1) and same(p0, p1) and same(l0, l1) and same(m0, m1)
            for hh in (None, hist[:B]):
                t0, p0, l0, m0 = whisper_amd.logits_sample_check(h, emb_d, temps[:B], seeds[:B], step, histories=hh,
                                                                 ts0=TS0, precision=prec)
                t1, p1, l1, m1 = whisper_amd.logits_suppress_check(h, emb_d, [], step, TS0, temperature=temps[:B],
                                                                   seed=seeds[:B], histories=hh, precision=prec)
                if hh is not None:
                    l1[m1.bool(), :TS0] = float("-inf")
                    assert same(m0, m1)
                assert same(t0, t1) and same(p0, p1) and same(l0, l1)
    if prec:
        return
    z32, zd, hist = stored(D)
    for sup in (False, True):
        t1, p1, _ = whisper_amd.row_suppress_check(zd, [], TS0, suppress_eot=sup)
        assert same(p1, whisper_amd.row_logprob_check(zd, 0, V, mask_eot=sup, idx=t1))
        want, wtok, _ = plain_rows(z32.astype(np.float64), [], 32, sup)
        assert np.array_equal(t1.cpu().numpy(), wtok)
        t0, p0, m0 = whisper_amd.row_timestamp_check(zd, hist, TS0, suppress_eot=sup)
        t1, p1, m1 = whisper_amd.row_suppress_check(zd, [], TS0, suppress_eot=sup, histories=hist)
        assert same(t0, t1) and same(p0, p1) and same(m0, m1)
        for hh in (None, hist):
            t0, p0, m0 = whisper_amd.row_sample_check(zd, temps, seeds, 4, suppress_eot=sup, histories=hh, ts0=TS0)
            t1, p1, m1 = whisper_amd.row_suppress_check(zd, [], TS0, suppress_eot=sup, pick=4, temperature=temps,
                                                        seed=seeds, histories=hh)
            assert same(t0, t1) and same(p0, p1) and same(m0, m1)
    zb, zbd, bh = beam_rows()
    rec = np.array([tr.record(x, TS0, V) for x in bh], np.int32)
    for step, sup, stop in ((-1, True, True), (2, False, True), (2, False, False)):
        t0, p0, f0 = whisper_amd.beam_topk_check(zbd, 6, step, sup, stop)
        t1, p1, _, f1 = whisper_amd.beam_topk_suppress_check(zbd, 6, [], TS0, None, step, sup, stop)
        assert same(t0, t1) and same(p0, p1) and f0 == f1
        t0, p0, m0, f0 = whisper_amd.beam_topk_rules_check(zbd, 6, rec, TS0, step, sup, stop)
        t1, p1, m1, f1 = whisper_amd.beam_topk_suppress_check(zbd, 6, [], TS0, rec, step, sup, stop)
        assert same(t0, t1) and same(p0, p1) and same(m0, m1) and f0 == f1


def test_check_entries_reject_bad_lists(torch):
    import whisper_amd
    import wq4

    _, zd, _ = stored(128)
    for ids in ([TS0], [-1], [V]):
        with pytest.raises(wq4.WQ4Error):
            whisper_amd.row_suppress_check(zd[:2].contiguous(), ids, TS0)
        with pytest.raises(wq4.WQ4Error):
            whisper_amd.beam_topk_suppress_check(zd[:2].contiguous(), 3, ids, TS0)
