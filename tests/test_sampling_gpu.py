"""Temperature sampling on the GPU (wa_transcribe_sampled, wa_transcribe_fallback,
include/whisper_amd.h): the KEYS forms of the fused logits + pick kernel and
of the stored-logits row kernel, and the model-level paths against a numpy
driver around the oracle's decoder.  The reference is sample_rules.py (pinned
by test_sampling.py), composed with ts_rules.py for the timestamp form.

Bounds.  u = 2^-24.
  Logit bound: 4e-6 max|ref| + 1e-6 (test_kernels_gpu.py); single-plane f16:
    (2^-10 + 2^-20) max_v sum_d |h_d e_vd| + 1e-6 (test_timestamps_gpu.py).
  Noise bound: the device's logf is documented to 1 ulp.  a = logf(u) carries
    a relative error <= 2^-23, which log(-a) turns into an absolute 2^-23; the
    outer logf adds one ulp of its result, <= 2^-23 |g|.  So |g32 - g64| <=
    2^-23 (1 + |g|) (1 % on top for second-order terms): 2.1e-6 at |g| = 16.64,
    the largest.  Derived, not measured.
  Key bound: key = fmaf(T, g32, z32) rounds once, <= ulp(key) / 2 <= u |key|;
    so |key32 - key64| <= logit bound + T * noise bound + u |key|.
  Decision margins: every row's float64 top-2 key gap is asserted >= 100 x
    the key bound at the row's largest |key| (single plane: also >= 2 x the
    key bound with that format's logit bound), and with timestamp records
    |lse_ts - max_text| >= 100 x the logit bound -- so every row is compared.
    The seeds are found on the CPU: the first seed from the row's base on that
    meets the gap (seeds_for).
  (i)  a kernel's log-probability against float64 numpy on the kernel's OWN
       masked f32 logits: |lp - lp64| <= (R + 24) u as in test_scores_gpu.py.
       The sampled reductions add what the unsampled ones add (their R), then
       d = z_tok - M (one rounding) and lp = d + lpg (one addition): R + 2.
         fused, plain: R = 24 + ceil(ceil(V / 128) / 8) = 75 at V = 51866.
         fused, timestamp records: R = 29 + ceil(ceil(ts0 / 128) / 8) = 79.
         row kernel (both forms join two sides): R = 16 + ceil(n / 256), n the
           longer side (V plain, ts0 with records).
  (ii) against the float64 logits: (i) plus twice the logit bound.
  Model level: 2 * 2e-3 * max|finite picked logits| (test_model_gpu.py's module
       tolerance, on the value and on the normaliser), which is also the key
       margin below which a clip's remaining picks are not compared.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import sample_rules as sr
import ts_rules as tr
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
SEED = 1234
V = 51866
TS0 = 50365
A, BT = 1000, 20000  # text ids
TEMPS = (0.0, 0.2, 1.0)
G_MAX = 16.64


def T_(k):
    return TS0 + k


def noise_bound(g=G_MAX):
    return 2.0 ** -23 * 1.01 * (1.0 + abs(g))


def r_fused(records):
    return (29 + math.ceil(math.ceil(TS0 / 128) / 8)) if records else (24 + math.ceil(math.ceil(V / 128) / 8))


def r_row(records):
    return 16 + math.ceil((TS0 if records else V) / 256)


def lse_rows(z):
    m = z.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


# ------------------------------------------------------------ planted rows --
# Like test_timestamps_gpu.planted, with a logit spread comparable to T: the
# background logits have std 0.28 (maximum about 1.3) and the noise T g reaches
# 2.2 at T = 0.2 and 11 at T = 1, so it decides.  Every row plants EOT at 1.9,
# the timestamp T_(30) at 1.75 (inside the first pick's window, past every
# history's last timestamp) and the text id A at 1.6: a T = 0 row picks one of
# them in every rule state with a gap of at least 0.15, and a T = 0.2 row picks
# one of them or, more often, a background id.  Rows with an even index also
# plant BT at 9, above the timestamps' logsumexp (7.35): with records the mass
# rule fires on the odd rows and not on the even ones (where both sides are open).
HISTORIES = [[], [T_(10), A], [T_(10), A, T_(20)], [T_(10), A, T_(20), T_(20)], [A]]  # first pick, then (last, penult) = 00 10 11 01


@functools.lru_cache(maxsize=None)
def planted_host(D):
    rng = np.random.default_rng(7000 + D)
    emb = (rng.uniform(-1, 1, (V, D)) * 0.03).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((D, 32)))
    unit = q.T  # [32, D], orthonormal rows
    hid = (unit * 16.0).astype(np.float32)
    emb[EOT] = (unit.sum(axis=0) * (1.9 / 16.0)).astype(np.float32)
    emb[A] = (unit.sum(axis=0) * (1.6 / 16.0)).astype(np.float32)
    emb[BT] = (unit[0::2].sum(axis=0) * (9.0 / 16.0)).astype(np.float32)
    emb[T_(30)] = (unit.sum(axis=0) * (1.75 / 16.0)).astype(np.float32)
    ref = hid.astype(np.float64) @ emb.astype(np.float64).T
    hist = [list(HISTORIES[r % len(HISTORIES)]) for r in range(32)]
    temps = np.array([TEMPS[r % 3] for r in range(32)], np.float32)
    absdot = np.abs(hid).astype(np.float64) @ np.abs(emb).astype(np.float64).T
    f16_bound = (2.0 ** -10 + 2.0 ** -20) * absdot.max(axis=1) + 1e-6
    return hid, emb, ref, hist, temps, f16_bound


@functools.lru_cache(maxsize=None)
def planted(D):
    import torch

    hid, emb, ref, hist, temps, f16b = planted_host(D)
    return torch.from_numpy(hid).cuda(), torch.from_numpy(emb).cuda()


def masked_row(z, hist, step, records):
    """(the float64 row the pick sees, rule f fired, rule f's margin)."""
    suppress = step + 1 < 3
    if records:
        zz, fired, _ = tr.apply_rules(z, hist, TS0, suppress)
        ae = tr.masks_ae(z, hist, TS0, suppress)
        lse_ts, mt = tr.lse(ae[TS0:]), float(ae[:TS0].max())
        margin = abs(lse_ts - mt) if np.isfinite(lse_ts) and np.isfinite(mt) else np.inf
        return zz, fired, margin
    zz = np.array(z, np.float64)
    if suppress:
        zz[EOT] = -np.inf
    return zz, False, np.inf


def key_bound(logit_bound, T, kmax):
    return logit_bound + T * noise_bound() + U * kmax


@functools.lru_cache(maxsize=None)
def seeds_for(D, records, picks=(1, 6), row_form=False):
    """Per row the first seed from 1000 r on whose float64 keys keep a top-2 gap
    >= 200 x the key bound (twice what the tests assert; the single-plane
    bound too) at every pick index of `picks`, both with EOT suppressed (pick
    <= 2) and without."""
    hid, emb, ref, hist, temps, f16b = planted_host(D)
    lb = 4e-6 * np.abs(ref).max(axis=1) + 1e-6
    out = []
    for r in range(32):
        s = 1000 * r
        while True:
            ok = True
            for p in picks:
                z, _, _ = masked_row(ref[r], hist[r], p - 1 if not row_form else (0 if p == 0 else 5), records)
                k = sr.keys(z, float(temps[r]), s, p)
                kmax = np.abs(k[np.isfinite(k)]).max()
                gap = sr.key_gap(k)
                ok = ok and gap >= 200 * key_bound(lb[r], float(temps[r]), kmax) and \
                    gap >= 4 * key_bound(f16b[r], float(temps[r]), kmax)
            if ok:
                break
            s += 1
            assert s < 1000 * r + 200, ("no seed meets the gap", r)
        out.append(s)
    return np.array(out, np.uint64)


def reference_rows(ref, hist, temps, seeds, B, step, pick, records):
    rows, toks, fired, gaps, kmaxs, mmargin = [], [], [], [], [], []
    for b in range(B):
        z, f, mm = masked_row(ref[b], hist[b], step, records)
        k = sr.keys(z, float(temps[b]), int(seeds[b]), pick)
        rows.append(z)
        toks.append(sr.pick(k))
        fired.append(f)
        gaps.append(sr.key_gap(k))
        kmaxs.append(np.abs(k[np.isfinite(k)]).max())
        mmargin.append(mm)
    return np.stack(rows), np.array(toks), np.array(fired), np.array(gaps), np.array(kmaxs), np.array(mmargin)


def check_fused(torch, D, B, step, prec, records):
    import whisper_amd

    hid_d, emb_d = planted(D)
    hid, emb, ref, hist, temps, f16b = planted_host(D)
    seeds = seeds_for(D, records)
    want, wtok, wfired, gaps, kmaxs, mmargin = reference_rows(ref, hist, temps, seeds, B, step, step + 1, records)
    greedy = np.array([sr.pick(want[b]) for b in range(B)])
    logit_bound = 4e-6 * np.abs(ref[:B]).max(axis=1) + 1e-6
    kb = np.array([key_bound(logit_bound[b], float(temps[b]), kmaxs[b]) for b in range(B)])
    assert (gaps >= 100 * kb).all(), (gaps, kb)
    assert (mmargin >= 100 * logit_bound).all(), (mmargin, logit_bound)
    if prec == 1:  # one f16 plane: the format's own bound (module docstring)
        logit_bound = f16b[:B]
        kb = np.array([key_bound(logit_bound[b], float(temps[b]), kmaxs[b]) for b in range(B)])
        assert (gaps >= 2 * kb).all() and (mmargin >= 2 * logit_bound).all(), (gaps, kb, mmargin)
    h = hid_d[:B].contiguous()
    tok, lp, lg, mass = whisper_amd.logits_sample_check(h, emb_d, temps[:B], seeds[:B], step,
                                                        histories=hist[:B] if records else None, ts0=TS0,
                                                        precision=prec)
    tok, lp, lg = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), lg.cpu().numpy().astype(np.float64)
    assert np.array_equal(tok, wtok), (tok, wtok)
    assert np.array_equal(np.isfinite(lg), np.isfinite(want))
    hot = temps[:B] > 0
    if B >= 17:
        assert 2 * int((tok[hot] != greedy[hot]).sum()) >= int(hot.sum()), (tok, greedy)  # the noise decides
    # the unsampled kernel on the same data: its rule f flag; T = 0 rows are its picks and log-probabilities exactly
    if records:
        gtok, glp, _, gmass = whisper_amd.logits_timestamp_check(h, emb_d, hist[:B], step, TS0, precision=prec)
        assert np.array_equal(mass.cpu().numpy(), gmass.cpu().numpy())
        assert np.array_equal(mass.cpu().numpy() != 0, wfired)
        if B >= 17:
            assert wfired.any() and not wfired.all()
    else:
        gtok, glp, _ = whisper_amd.logits_logprob_check(h, emb_d, step, precision=prec)
    cold = ~hot
    assert np.array_equal(tok[cold], gtok.cpu().numpy()[cold])
    assert np.array_equal(lp[cold], glp.cpu().numpy().astype(np.float64)[cold])
    b1 = (r_fused(records) + 24) * U
    err_i = np.abs(lp - (lg[np.arange(B), tok] - lse_rows(lg)))
    err_ii = np.abs(lp - (want[np.arange(B), wtok] - lse_rows(want)))
    bound_ii = b1 + 2 * logit_bound
    print(f"D {D} B {B} step {step} prec {prec} records {records}: (i) {err_i.max() / U:.1f} u of {b1 / U:.0f} u, "
          f"(ii) {(err_ii / bound_ii).max():.3f} of its bound, smallest gap / bound {(gaps / kb).min():.0f}, "
          f"{int((tok[hot] != greedy[hot]).sum())} of {int(hot.sum())} T > 0 rows off the greedy token")
    assert (err_i <= b1).all(), (err_i / U, b1 / U)
    assert (err_ii <= bound_ii).all(), (err_ii, bound_ii)


@pytest.mark.parametrize("prec", [0, 1])  # PREC_F16X2 (NS = 2), PREC_F16 (NS = 1)
@pytest.mark.parametrize("D", [128, 384])
def test_fused_sampled_pick(torch, D, prec):
    """V = 51866, B in {1, 17, 32} (the padded case, into the second n-tile,
    both tiles full), step 0 (EOT suppressed, pick 1) and 5 (pick 6); rows with
    temperatures 0, 0.2, 1 and distinct seeds in one launch.  R = 75 (99 u)."""
    for B in (1, 17, 32):
        for step in (0, 5):
            check_fused(torch, D, B, step, prec, False)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("D", [128, 384])
def test_fused_sampled_timestamp_pick(torch, D, prec):
    """The same under rule records: histories of the first pick and all four
    (last, penult) states.  Rule f's flag is the unsampled kernel's -- it does
    not see the noise -- and the token the reference's over the surviving side.
    R = 79 (103 u)."""
    for B in (1, 17, 32):
        for step in (0, 5):
            check_fused(torch, D, B, step, prec, True)


@pytest.mark.parametrize("V_,ts0", [(300, 200), (300, 256), (1100, 1000)])
def test_pick_forms_agree_small_vocab(torch, V_, ts0):
    """The five fused forms are one reduction: at vocabularies of 3 workgroups
    (fewer than the 8 reduction parts, a padded tail; ts0 inside a workgroup
    and on a workgroup boundary) and of 9 (uneven parts), D = 128, B in
    {1, 32}, steps 0 and 5, the sampled check at T = 0 returns the scored
    check's tokens and log-probabilities, with records the timestamp check's
    tokens, log-probabilities and mass flags, and the scored check's tokens
    are the plain check's.  Exact: the forms are compared with each other, so
    no reference margin enters.  Three rows tie at the maximum across a
    workgroup boundary and across ts0."""
    import whisper_amd

    D = 128
    rng = np.random.default_rng(V_ + ts0)
    emb = (rng.uniform(-1, 1, (V_, D)) * 0.03).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((D, 32)))
    hid = (q.T * 16.0).astype(np.float32)
    emb[[5, 133, ts0 - 1, ts0 + 3]] = (q.T.sum(axis=0) * (2.0 / 16.0)).astype(np.float32)
    text = 7
    states = [[], [ts0 + 10, text], [ts0 + 10, text, ts0 + 20], [ts0 + 10, text, ts0 + 20, ts0 + 20], [text]]
    hist = [states[r % 5] for r in range(32)]
    emb_d = torch.from_numpy(emb).cuda()
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for B in (1, 32):
        h = torch.from_numpy(hid[:B]).cuda()
        for step in (0, 5):
            ptok, _ = whisper_amd.logits_argmax_check(h, emb_d, step)
            stok, slp, _ = whisper_amd.logits_logprob_check(h, emb_d, step)
            ttok, tlp, _, tmass = whisper_amd.logits_timestamp_check(h, emb_d, hist[:B], step, ts0)
            tok, lp, _, _ = whisper_amd.logits_sample_check(h, emb_d, 0.0, 11, step)
            rtok, rlp, _, rmass = whisper_amd.logits_sample_check(h, emb_d, 0.0, 11, step, histories=hist[:B], ts0=ts0)
            assert same(stok, ptok), (B, step)
            assert same(tok, stok) and same(lp, slp), (B, step)
            assert same(rtok, ttok) and same(rlp, tlp) and same(rmass, tmass), (B, step)
            assert np.isfinite(slp.cpu().numpy()).all() and np.isfinite(tlp.cpu().numpy()).all()


@pytest.mark.parametrize("records", [False, True])
def test_row_sample_kernel(torch, records):
    """The planted logits stored as f32 rows through the stored-logits kernel,
    n_rows in {1, 32}, pick 0 with EOT suppressed (the prompt's pick) and pick
    6: the reference's tokens on those rows (no logit error: the key bound is T
    x the noise bound and the fmaf's rounding), rule f's flag, bound (i)."""
    import whisper_amd

    D = 128
    hid, emb, ref, hist, temps, f16b = planted_host(D)
    z32 = ref.astype(np.float32)
    zd = torch.from_numpy(z32).cuda()
    seeds = seeds_for(D, records, picks=(0, 6), row_form=True)
    for n in (1, 32):
        for pick, sup in ((0, True), (6, False)):
            step = 0 if sup else 5
            want, wtok, wfired, gaps, kmaxs, mmargin = reference_rows(z32.astype(np.float64), hist, temps, seeds, n,
                                                                      step, pick, records)
            kb = np.array([key_bound(0.0, float(temps[b]), kmaxs[b]) for b in range(n)])
            assert (gaps >= 100 * kb).all() and (mmargin >= 1e-2).all(), (gaps, kb, mmargin)
            tok, lp, mass = whisper_amd.row_sample_check(zd[:n].contiguous(), temps[:n], seeds[:n], pick,
                                                         suppress_eot=sup, histories=hist[:n] if records else None,
                                                         ts0=TS0)
            tok, lp, mass = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), mass.cpu().numpy()
            assert np.array_equal(tok, wtok), (tok, wtok)
            assert np.array_equal(mass != 0, wfired)
            err = np.abs(lp - (want[np.arange(n), wtok] - lse_rows(want)))
            assert (err <= (r_row(records) + 24) * U).all(), err / U
            cold = temps[:n] == 0  # T = 0: the unsampled row kernels' picks and scores
            if records:
                gtok, glp, _ = whisper_amd.row_timestamp_check(zd[:n].contiguous(), hist[:n], TS0, suppress_eot=sup)
                assert np.array_equal(tok[cold], gtok.cpu().numpy()[cold])
                assert np.array_equal(lp[cold], glp.cpu().numpy().astype(np.float64)[cold])
            else:
                glp = whisper_amd.row_logprob_check(zd[:n].contiguous(), 0, V, mask_eot=sup,
                                                    idx=torch.from_numpy(tok.astype(np.int32)).cuda())
                assert np.array_equal(lp[cold], glp.cpu().numpy().astype(np.float64)[cold])
                assert np.array_equal(tok[cold], np.array([sr.pick(want[b]) for b in range(n)])[cold])


# ------------------------------------------------------------------ model --
def mels(clips, n_mels=80):
    return np.stack([wo.synthetic_mel(c, n_mels) for c in clips]).astype(np.float32)


def oracle_sampled(om, mel, lang, max_tokens, temps, seeds, timestamps, max_initial=50):
    """The numpy driver: whisper_oracle's encode / decoder_pass with
    sample_rules (over ts_rules' masked row when timestamps) before every pick.
    Per clip the picks in order (an EOT pick that ends the clip included), and
    per pick its float64 log-probability, the tolerance 2 * 2e-3 * max|finite
    picked logits| and the decision margin: the top-2 key gap and, with
    timestamps, rule f's margin."""
    c = om.cfg
    B = mel.shape[0]
    tt = 50260 + c["n_lang"]
    ts0 = tt + 5
    cache = om.init_cache(om.encode(mel))
    z0 = om.decoder_pass(np.full((B, 1), wo.SOT), np.arange(1), cache, fresh=True).astype(np.float64)
    lo, hi = 50259, 50259 + c["n_lang"]
    tail = [tt] if timestamps else [tt, tt + 4]
    if lang is not None:
        langs = [lang] * B
        logits = om.decoder_pass(np.array([[wo.SOT, lang] + tail] * B), np.arange(2 + len(tail)), cache, fresh=True)
        position = 2 + len(tail)
    else:
        langs = [lo + om.argmax_last(z0[b, lo:hi].astype(np.float32)) for b in range(B)]
        logits = om.decoder_pass(np.array([[lg] + tail for lg in langs]), np.arange(1 + len(tail)), cache, fresh=True)
        position = 1 + 1 + len(tail)
    seq = [[] for _ in range(B)]
    picks = [[] for _ in range(B)]
    done = [False] * B

    def pick_all(logits, suppress, pick):
        nxt = []
        for b in range(B):
            if timestamps:
                z, _, margin = tr.apply_rules(logits[b].astype(np.float64), seq[b], ts0, suppress, max_initial)
                ae = tr.masks_ae(logits[b].astype(np.float64), seq[b], ts0, suppress, max_initial)
                l, mt = tr.lse(ae[ts0:]), float(ae[:ts0].max())
                margin = abs(l - mt) if np.isfinite(l) and np.isfinite(mt) else np.inf
            else:
                z = logits[b].astype(np.float64)
                if suppress:
                    z[EOT] = -np.inf
                margin = np.inf
            k = sr.keys(z, float(temps[b]), int(seeds[b]), pick)
            t = sr.pick(k)
            if not done[b]:
                picks[b].append((t, z[t] - tr.lse(z), 2 * 2e-3 * np.abs(z[np.isfinite(z)]).max(),
                                 min(margin, sr.key_gap(k))))
            nxt.append(t)
        return nxt

    nxt = pick_all(logits, True, 0)
    for step in range(max_tokens):
        for b in range(B):
            if not done[b] and nxt[b] == EOT:
                done[b] = True
            seq[b].append(nxt[b])
        if all(done):
            break
        logits = om.decoder_pass(np.array(nxt)[:, None], np.array([position]), cache, fresh=False)
        position += 1
        nxt = pick_all(logits, step + 1 < wo.MIN_TOKENS, step + 1)
    for b in range(B):
        picks[b] = picks[b][:max_tokens]
    return {"picks": picks, "ts0": ts0, "lang_tok": langs, "z0tol": 2 * 2e-3 * np.abs(z0).max(axis=1),
            "no_speech": np.exp(z0[:, tt + 3] - lse_rows(z0)),
            "lang_prob": np.exp(z0[np.arange(B), langs] - lse_rows(z0[:, lo:hi]))}


def compared_steps(picks):
    k = 0
    while k < len(picks) and picks[k][3] >= picks[k][2]:
        k += 1
    return k


def got_sequence(g, max_tokens):
    n = len(g["tokens"])
    slots = g["logprob_slots"]
    return g["tokens"] + ([EOT] if n < max_tokens and not np.isnan(slots[n]) else [])


def check_against_driver(got, want, max_tokens):
    total = compared = 0
    for b, g in enumerate(got):
        picks = want["picks"][b]
        k = compared_steps(picks)
        total += len(picks)
        compared += k
        assert k >= min(8, len(picks)), (b, k)  # the cap, per clip (met by the driver alone: MODEL_CASES)
        seq = got_sequence(g, max_tokens)
        assert seq[:k] == [p[0] for p in picks[:k]], (b, k, seq, [p[0] for p in picks])
        lp = g["logprob_slots"][:k].astype(np.float64)
        err = np.abs(lp - np.array([p[1] for p in picks[:k]]))
        assert (err <= np.array([p[2] for p in picks[:k]])).all(), (b, err)
        for key in ("no_speech", "lang_prob"):
            p, q = g[key if key == "lang_prob" else "no_speech_prob"], want[key][b]
            assert abs(p - q) <= q * math.expm1(want["z0tol"][b]) + 1e-12, (key, b, p, q)
        assert g["lang_token"] == want["lang_tok"][b]
    assert 2 * compared >= total, (compared, total)  # the cap, over all (clip, pick) pairs
    print(f"compared {compared} of {total} picks")


MODEL_TOKENS = 24
MODEL_TEMPS = (0.0, 0.5, 1.0)
# (language, timestamps) -> (clips, seeds): synthetic_mel indices and per-clip
# seeds on which the driver alone meets both caps with SEED at temperatures
# (0, 0.5, 1) -- here every one of the 24 picks has its margin at or above its
# tolerance.  Found by running the driver on the CPU, one clip at a time: the
# clip at that position of the timestamp test's MODEL_CLIPS first, then clips
# 0 .. 44, with seeds 0 .. 63 each; the first hit is taken (every position was
# served by its MODEL_CLIPS clip, within seeds 0 .. 4).
MODEL_CASES = {
    (50259, False): ([9, 10, 11], [0, 0, 0]),
    (None, False): ([8, 10, 16], [0, 4, 0]),
    (50259, True): ([9, 10, 11], [0, 1, 0]),
    (None, True): ([8, 10, 16], [0, 0, 0]),
}


@pytest.fixture(scope="module")
def oracle_model():
    return wo.SynthWhisper("tiny_test", SEED)


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    yield m
    m.close()


@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("lang", [50259, None])
@pytest.mark.parametrize("n_clips", [2, 3])
def test_transcribe_sampled_matches_driver(torch, oracle_model, gpu_model, n_clips, lang, timestamps):
    """TINY_TEST, Q4_0, 24 tokens, per-clip temperatures (0, 0.5, 1)."""
    clips, seeds = MODEL_CASES[(lang, timestamps)]
    mel = mels(clips[:n_clips])
    temps, seeds = np.array(MODEL_TEMPS[:n_clips], np.float32), np.array(seeds[:n_clips], np.uint64)
    want = oracle_sampled(oracle_model, mel, lang, MODEL_TOKENS, temps, seeds, timestamps)
    got = gpu_model.transcribe_sampled(torch.from_numpy(mel).cuda(), temps, seeds, lang, max_tokens=MODEL_TOKENS,
                                       timestamps=timestamps)
    check_against_driver(got, want, MODEL_TOKENS)
    if timestamps:
        import whisper_amd

        for g in got:
            assert (g["segments"], g["seek_frames"]) == whisper_amd.segments_from_tokens(g["tokens"], want["ts0"])


def same_clip(a, b):
    assert a["tokens"] == b["tokens"]
    assert np.array_equal(a["logprob_slots"], b["logprob_slots"], equal_nan=True)
    assert a["no_speech_prob"] == b["no_speech_prob"] and a["lang_prob"] == b["lang_prob"]
    assert a["lang_token"] == b["lang_token"]


def test_determinism_and_independence(torch, oracle_model, gpu_model):
    """The same call twice: identical tokens and slots.  All-zero temperatures:
    transcribe_scored's (timestamps: transcribe_timestamps') tokens and slots
    bit for bit.  Permuting the clips with their seeds and temperatures
    permutes the results; a differing clip is excused only from a pick whose
    driver margin is below the tolerance."""
    n = MODEL_TOKENS
    for ts in (False, True):
        clips, seeds = MODEL_CASES[(50259, ts)]
        mel = torch.from_numpy(mels(clips)).cuda()
        temps, seeds = np.array(MODEL_TEMPS, np.float32), np.array(seeds, np.uint64)
        one = gpu_model.transcribe_sampled(mel, temps, seeds, 50259, max_tokens=n, timestamps=ts)
        two = gpu_model.transcribe_sampled(mel, temps, seeds, 50259, max_tokens=n, timestamps=ts)
        for a, b in zip(one, two):
            same_clip(a, b)
        zero = gpu_model.transcribe_sampled(mel, 0.0, seeds, 50259, max_tokens=n, timestamps=ts)
        base = gpu_model.transcribe_timestamps(mel, 50259, max_tokens=n) if ts else \
            gpu_model.transcribe_scored(mel, 50259, max_tokens=n)
        for a, b in zip(zero, base):
            same_clip(a, b)
        same_clip(zero[0], one[0])  # a T = 0 clip beside T > 0 clips is the greedy clip
        perm = [2, 0, 1]
        got = gpu_model.transcribe_sampled(mel[perm].contiguous(), temps[perm], seeds[perm], 50259, max_tokens=n,
                                           timestamps=ts)
        want = None
        for j, c in enumerate(perm):
            a, b = got[j], one[c]
            if a["tokens"] != b["tokens"]:
                if want is None:
                    want = oracle_sampled(oracle_model, mels(clips), 50259, n, temps, seeds, ts)
                k = compared_steps(want["picks"][c])
                assert got_sequence(a, n)[:k] == got_sequence(b, n)[:k], (c, k)
    assert any(len(c["tokens"]) for c in one)


def test_pipelined_sampled_match_sequential(torch, oracle_model, monkeypatch):
    """3 batches x 17 clips, max_tokens 8: one unit of three, each group drawing
    with its own batch's seeds and temperatures.  Tokens equal the three
    single-batch sampled calls' (a differing clip is excused from the pick on
    whose driver margin is below the tolerance); scores to the logit tolerance."""
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    NB, B, n = 3, 17, 8
    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=B)
    clip_ids = [[500 + i * B + c for c in range(B)] for i in range(NB)]
    x = torch.from_numpy(np.stack([mels(ids) for ids in clip_ids])).cuda()
    temps = np.array([[MODEL_TEMPS[(i + c) % 3] for c in range(B)] for i in range(NB)], np.float32)
    seeds = np.arange(NB * B, dtype=np.uint64).reshape(NB, B) * np.uint64(977) + np.uint64(5)
    prompt = torch.tensor([[50258, 50259, 50360, 50364]] * B, dtype=torch.int32, device="cuda")
    tol = 1e30
    for i in range(NB):
        m.encode(x[i])
        tol = min(tol, 2 * 2e-3 * float(m.prompt_logits(prompt).abs().amax(dim=1).min()))
    got = m.transcribe_batches_sampled(x, temps, seeds, 50259, max_tokens=n)
    assert (m.pipeline_stats()["pairs"], m.pipeline_stats()["units3"]) == (0, 1)
    differing = 0
    for i in range(NB):
        seq = m.transcribe_sampled(x[i], temps[i], seeds[i], 50259, max_tokens=n)
        for c, (a, b) in enumerate(zip(got[i], seq)):
            k = None
            if a["tokens"] != b["tokens"]:
                differing += 1
                want = oracle_sampled(oracle_model, mels([clip_ids[i][c]]), 50259, n, temps[i, c:c + 1],
                                      seeds[i, c:c + 1], False)
                k = compared_steps(want["picks"][0])
            sa, sb = got_sequence(a, 10 ** 6), got_sequence(b, 10 ** 6)
            k = len(a["tokens"]) if k is None else k
            assert sa[:k] == sb[:k], (i, c, k)
            la, lb = a["logprob_slots"][:k].astype(np.float64), b["logprob_slots"][:k].astype(np.float64)
            assert np.array_equal(np.isnan(la), np.isnan(lb))
            assert np.nanmax(np.abs(la - lb), initial=0.0) <= tol, (la, lb, tol)
            assert a["lang_token"] == b["lang_token"]
    assert differing <= NB * B // 4  # the excuse is for the odd clip, not the rule
    m.close()


def test_wide_group_matches_fused(torch, oracle_model):
    """66 clips decode in two groups of 33 rows, past the fused kernel's 32:
    every step's pick is the stored-logits row kernel at pick index
    DecodeState::step + 1.  The same clips in calls of 22 take the fused
    kernel.  Same tokens, under the excuse rule of the pipelined test; scores
    to the logit tolerance."""
    import whisper_amd

    B, n, part = 66, 8, 22
    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=B)
    ids = [700 + c for c in range(B)]
    x = torch.from_numpy(mels(ids)).cuda()
    temps = np.array([MODEL_TEMPS[c % 3] for c in range(B)], np.float32)
    seeds = np.arange(B, dtype=np.uint64) * np.uint64(131) + np.uint64(9)
    prompt = torch.tensor([[50258, 50259, 50360, 50364]] * B, dtype=torch.int32, device="cuda")
    m.encode(x)
    tol = 2 * 2e-3 * float(m.prompt_logits(prompt).abs().amax(dim=1).min())
    wide = m.transcribe_sampled(x, temps, seeds, 50259, max_tokens=n)
    assert whisper_amd.decode_group_rows(B) > 32 >= whisper_amd.decode_group_rows(part)
    differing = 0
    for p in range(0, B, part):
        sl = slice(p, p + part)
        fused = m.transcribe_sampled(x[sl].contiguous(), temps[sl], seeds[sl], 50259, max_tokens=n)
        for c, (a, b) in enumerate(zip(wide[sl], fused)):
            k = len(a["tokens"])
            if a["tokens"] != b["tokens"]:
                differing += 1
                want = oracle_sampled(oracle_model, mels([ids[p + c]]), 50259, n, temps[p + c:p + c + 1],
                                      seeds[p + c:p + c + 1], False)
                k = compared_steps(want["picks"][0])
            assert got_sequence(a, 10 ** 6)[:k] == got_sequence(b, 10 ** 6)[:k], (p + c, k)
            la, lb = a["logprob_slots"][:k].astype(np.float64), b["logprob_slots"][:k].astype(np.float64)
            assert np.array_equal(np.isnan(la), np.isnan(lb))
            assert np.nanmax(np.abs(la - lb), initial=0.0) <= tol, (la, lb, tol)
    assert differing <= B // 4  # the excuse is for the odd clip, not the rule
    m.close()


def test_fallback_ladder(torch, gpu_model):
    """4 clips, ladder (0, 0.5, 1), 12 tokens.  The threshold sits in the widest
    gap of the clips' greedy mean log-probabilities, so some clips pass rung 0
    and some do not.  Every clip's tokens, slots and rung are those of the
    full-batch transcribe_sampled call at its rung's temperature with seeds
    seed + r, composed by sample_rules.ladder: a frozen row does not disturb a
    live one."""
    n, ladder = 12, (0.0, 0.5, 1.0)
    mel = torch.from_numpy(mels([9, 10, 11, 8])).cuda()
    seeds = np.array([11, 22, 33, 44], np.uint64)
    greedy = gpu_model.transcribe_scored(mel, 50259, max_tokens=n)
    means = np.sort([sr.mean_logprob(c["logprob_slots"]) for c in greedy])
    i = int(np.argmax(np.diff(means)))
    thr = float((means[i] + means[i + 1]) / 2)
    rungs, rung_steps = [], []
    for r, t in enumerate(ladder):
        rungs.append(gpu_model.transcribe_sampled(mel, t, seeds + np.uint64(r), 50259, max_tokens=n))
        rung_steps.append(gpu_model.last_timings()["steps"])
    for a, b in zip(rungs[0], greedy):
        same_clip(a, b)

    def composed(lp_thr, ns_thr):
        res = [[(sr.mean_logprob(c["logprob_slots"]), c["no_speech_prob"]) for c in rung] for rung in rungs]
        return sr.ladder(res, lp_thr, ns_thr)

    def check(got, want_rungs):
        assert [c["rung"] for c in got] == want_rungs, ([c["rung"] for c in got], want_rungs)
        for c, g in enumerate(got):
            same_clip(g, rungs[g["rung"]][c])
            assert g["temperature"] == np.float32(ladder[g["rung"]])

    nan = float("nan")
    want = composed(thr, nan)
    assert 0 in want and any(r > 0 for r in want)  # some clips pass rung 0, some do not
    check(gpu_model.transcribe_fallback(mel, seeds, ladder, thr, None, 50259, max_tokens=n), want)
    # a clip that passes no rung keeps the last rung's result; every rung decodes every clip, and the steps add up
    check(gpu_model.transcribe_fallback(mel, seeds, ladder, math.inf, None, 50259, max_tokens=n), [2, 2, 2, 2])
    assert gpu_model.last_timings()["steps"] == sum(rung_steps)
    # every clip is silence above a no-speech threshold of 0: rung 0
    check(gpu_model.transcribe_fallback(mel, seeds, ladder, math.inf, 0.0, 50259, max_tokens=n), [0, 0, 0, 0])
    # NaN thresholds: rung 0 for all
    check(gpu_model.transcribe_fallback(mel, seeds, ladder, None, None, 50259, max_tokens=n), [0, 0, 0, 0])
    # with timestamps the ladder composes the timestamp calls
    ts_rungs = [gpu_model.transcribe_sampled(mel, t, seeds + np.uint64(r), 50259, max_tokens=n, timestamps=True)
                for r, t in enumerate(ladder)]
    got = gpu_model.transcribe_fallback(mel, seeds, ladder, math.inf, None, 50259, max_tokens=n, timestamps=True)
    for c, g in enumerate(got):
        assert g["rung"] == 2
        same_clip(g, ts_rungs[2][c])
        assert g["segments"] == ts_rungs[2][c]["segments"]


def test_sampling_leaves_other_paths_alone(torch):
    """Plain, scored and timestamp calls return what they returned before a
    sampled call, on the graph keys they had; the sampled key is a fourth; the
    buffers are allocated once and counted."""
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    mel = torch.from_numpy(mels([11, 12, 13])).cuda()
    plain = m.transcribe(mel, 50259, max_tokens=12)
    key_plain = m.decode_graph_key(0)
    scored = m.transcribe_scored(mel, 50259, max_tokens=12)
    key_scored = m.decode_graph_key(0)
    ts = m.transcribe_timestamps(mel, 50259, max_tokens=12)
    key_ts = m.decode_graph_key(0)
    n0 = m.device_bytes()
    smp = m.transcribe_sampled(mel, 0.8, [1, 2, 3], 50259, max_tokens=12)
    key_smp = m.decode_graph_key(0)
    assert len({key_plain, key_scored, key_ts, key_smp}) == 4 and min(key_plain, key_scored, key_ts, key_smp) >= 0
    assert m.device_bytes() > n0
    n1 = m.device_bytes()
    assert [c["tokens"] for c in smp] != plain
    assert m.transcribe(mel, 50259, max_tokens=12) == plain
    assert m.decode_graph_key(0) == key_plain
    for call, before, key in ((m.transcribe_scored, scored, key_scored), (m.transcribe_timestamps, ts, key_ts)):
        again = call(mel, 50259, max_tokens=12)
        assert m.decode_graph_key(0) == key
        for a, b in zip(again, before):
            same_clip(a, b)
    smp2 = m.transcribe_sampled(mel, [0.8, 0.1, 0.0], [1, 2, 3], 50259, max_tokens=12)
    assert m.device_bytes() == n1  # allocated once
    assert m.decode_graph_key(0) == key_smp  # temperatures and seeds are read at run time, not baked in
    same_clip(smp2[0], smp[0])
    m.transcribe_fallback(mel, [1, 2, 3], (0.0, 1.0), math.inf, None, 50259, max_tokens=12)
    assert m.device_bytes() == n1
    smp_ts = m.transcribe_sampled(mel, 0.8, [1, 2, 3], 50259, max_tokens=12, timestamps=True)
    assert m.decode_graph_key(0) not in (key_plain, key_scored, key_ts, key_smp)
    assert all(c["tokens"][0] >= m.timestamp_begin for c in smp_ts)
    m.close()
