"""Timestamp decoding on the GPU (wa_transcribe_timestamps, include/whisper_amd.h):
the TS form of the fused logits + pick kernel, the stored-logits row kernel,
the bookkeeping kernel's rule records, and the model-level paths against a
numpy driver around the oracle's decoder.  The rule's reference is ts_rules.py
(pinned by test_timestamps.py).

Bounds.  u = 2^-24.
  Decision margins: every planted row's margin on the float64 logits -- the
    allowed set's top-2 gap and |lse_ts - max_text| -- is asserted >= 100 x the
    logit bound of test_kernels_gpu.py (4e-6 max|ref| + 1e-6), so every token
    is compared.
  (i)  a kernel's log-probability against float64 numpy on the kernel's OWN
       masked f32 logits: |lp - lp64| <= (R + 24) u as in test_scores_gpu.py.
         fused kernel (pick_from_lds<2, 1, 0>): per side a thread adds its 16 terms
           (16 additions), 3 shuffle adds, the last workgroup's thread adds the
           side's rescaled candidates -- ceil(ceil(ts0 / 128) / 8) on the text
           side, the longer one -- and 3 shuffle adds; joining the sides is one
           addition more with a subtract, an expf and a multiply on each term
           (counted as 4): R = 27 + ceil(ceil(ts0 / 128) / 8) = 77 at
           ts0 = 50365.
         row kernel (row_pick_kernel<0>): ceil(ts0 / 256) additions per
           thread on the text side, 6 shuffle adds, 3 adds over the waves, the
           join as above: R = 14 + ceil(ts0 / 256) = 211.
  (ii) against the float64 logits: (i) plus twice the logit bound.
  Single-plane f16 operands (WQ4_PREC_F16, NS = 1): the logit bound above is
    that of the f16-pair product.  With one plane each operand is one RNE f16,
    relative error <= 2^-11, so a logit is off by at most
    (2^-10 + 2^-20) sum_d |h_d e_vd| (+ 1e-6 for the f32 accumulation and
    flushed subnormals); that bound, maximised over the row's ids, replaces the
    logit bound in (ii), and the margins are asserted >= 2 x it (no logit moves
    by more than the bound, so no decision can flip), on top of the 100 x
    rule, which every row meets in both precisions.
  Model level: 2 * 2e-3 * max|finite picked logits| (test_model_gpu.py's module
       tolerance, on the value and on the normaliser), which is also the margin
       below which a clip's remaining steps are not compared.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import ts_rules as tr
import whisper_oracle as wo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
SEED = 1234
V = 51866
TS0 = 50365
A, BT = 1000, 20000  # text ids


def T(k):
    return TS0 + k


def r_fused(ts0=TS0):
    return 27 + math.ceil(math.ceil(ts0 / 128) / 8)


def r_row(ts0=TS0):
    return 14 + math.ceil(ts0 / 256)


def lse_rows(z):
    m = z.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


# ---------------------------------------------------------- planted rows --
# (history, {id: logit}, winner at a step that does not suppress EOT).  The
# hidden rows are orthogonal, so a planted embedding row a * unit(hid[r]) adds
# a * |hid[r]| to row r alone; the background logits have std 0.28 (maximum
# about 1.3, logsumexp over all timestamps about 7.4).
OPEN = [T(10), A]  # text after a timestamp: text, or a timestamp > T(10)
PLANTS = [
    # 0 first pick: the raw maximum a text token, the best timestamp beyond max_initial
    ([], {A: 20.0, T(80): 16.0, T(30): 12.0}, T(30)),
    # 1 last & penult: the best timestamp beats all text but must lose
    ([T(10), A, T(20), T(20)], {T(1000): 20.0, A: 12.0}, A),
    # 2 last & !penult: the best text must lose; EOT wins (the timestamps' mass stays below it)
    ([T(10), A, T(20)], {A: 20.0, EOT: 16.0, T(50): 12.0}, EOT),
    # 3 last & !penult: a timestamp wins
    ([T(10), A, T(20)], {A: 20.0, EOT: 12.0, T(50): 16.0}, T(50)),
    # 4 monotonic, inclusive bound (last & !penult allows t itself): T(39) is the best and masked
    ([T(10), A, T(40)], {T(39): 20.0, T(40): 16.0}, T(40)),
    # 5 monotonic, strict bound: t and below masked
    ([T(10), A, T(40), T(40), BT], {T(40): 20.0, T(39): 18.0, T(41): 16.0, A: 10.0}, T(41)),
    # 6 mass rule firing: 200 timestamps 3 below the best text logit; no single one wins, the sum does
    (OPEN, {A: 16.0, **{T(100 + i): 13.0 for i in range(200)}}, T(299)),
    # 7 mass rule not firing: 200 timestamps at 8 (lse 13.3) against text at 16
    (OPEN, {A: 16.0, **{T(400 + i): 8.0 for i in range(200)}}, A),
    # 8 a special id the raw maximum
    (OPEN, {50300: 20.0, A: 12.0, T(700): 6.0}, A),
    # 9 a tie between two allowed timestamps (identical embedding rows): the larger id
    (OPEN, {T(800): 16.0, T(900): 16.0, A: 10.0}, T(900)),
    # 10 ts0 - 1 (NO_TIMESTAMPS, a special: it can only lose) the raw maximum, ts0 the winner
    ([], {TS0 - 1: 20.0, TS0: 12.0}, TS0),
    # 11 V - 1 the winner, ts0 - 1 again above it
    (OPEN, {TS0 - 1: 20.0, V - 1: 16.0, A: 10.0}, V - 1),
    # 12 the allowed timestamps are V - 1 alone
    ([T(10), A, V - 1], {A: 20.0, V - 1: 12.0, EOT: 8.0}, V - 1),
    # 13 ts0 a winner after text with no timestamp yet
    ([A], {TS0: 16.0, BT: 10.0}, TS0),
    # 14 EOT the winner among text
    (OPEN, {EOT: 20.0, A: 12.0}, EOT),
    # 15 first pick with the bound's last id the winner
    ([], {T(51): 20.0, T(50): 16.0}, T(50)),
]
POOL = [A, BT, EOT, TS0, T(1), T(40), T(700), V - 1]
# rows 16 .. 31: a random history over POOL without V - 1 and this plant, which
# decides every state with room: the first pick takes T(25); text-only states
# and text + later timestamps take A (the timestamps' mass, about 10.2, stays
# below 12); after text + timestamp T(1400) beats EOT
FILL = {A: 12.0, T(1400): 10.0, T(25): 8.0, EOT: 6.0}
STEP = 5  # no EOT suppression; step 0 suppresses it


@functools.lru_cache(maxsize=None)
def planted_host(D):
    """32 orthogonal hidden rows of norm 16, the planted embedding, the float64
    logits and the rows' histories; rows 16 .. 31: random histories over the
    FILL plant."""
    rng = np.random.default_rng(D)
    emb = (rng.uniform(-1, 1, (V, D)) * 0.03).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((D, 32)))
    unit = q.T  # [32, D], orthonormal rows
    hid = (unit * 16.0).astype(np.float32)
    rows = {}
    for r in range(32):
        for i, val in (PLANTS[r][1] if r < len(PLANTS) else FILL).items():
            rows.setdefault(i, np.zeros(D))
            rows[i] += unit[r] * (val / 16.0)
    for i, vec in rows.items():
        emb[i] = vec.astype(np.float32)
    hist = [list(p[0]) for p in PLANTS]
    for r in range(len(PLANTS), 32):
        hist.append([int(rng.choice(POOL[:-1])) for _ in range(int(rng.integers(0, 6)))])
    ref = hid.astype(np.float64) @ emb.astype(np.float64).T
    # bit-equal embedding rows have equal logits in any one arithmetic; a blocked
    # float64 product may differ in the last bit between columns, so copy them
    groups = {}
    for i in rows:
        groups.setdefault(emb[i].tobytes(), []).append(i)
    for ids in groups.values():
        ref[:, ids] = ref[:, ids[:1]]
    return hid, emb, ref, hist


@functools.lru_cache(maxsize=None)
def f16_logit_bound(D):
    """Per row: the single-plane logit bound (2^-10 + 2^-20) max_v sum_d |h_d e_vd| + 1e-6."""
    hid, emb, _, _ = planted_host(D)
    return (2.0 ** -10 + 2.0 ** -20) * (np.abs(hid).astype(np.float64) @ np.abs(emb).astype(np.float64).T).max(axis=1) + 1e-6


@functools.lru_cache(maxsize=None)
def planted(D):
    """planted_host with the hidden rows and the embedding on the device (once)."""
    import torch

    hid, emb, ref, hist = planted_host(D)
    return hid, torch.from_numpy(hid).cuda(), torch.from_numpy(emb).cuda(), ref, hist


def rule_rows(ref, hist, B, step):
    """The numpy rule on float64 rows: (masked rows, tokens, fired, margins)."""
    out, toks, fired, margins = [], [], [], []
    for b in range(B):
        z, f, m = tr.apply_rules(ref[b], hist[b], TS0, step + 1 < 3)
        out.append(z)
        toks.append(tr.pick(z))
        fired.append(f)
        margins.append(m)
    return np.stack(out), np.array(toks), np.array(fired), np.array(margins)


def check_fused(torch, D, B, step, prec):
    import whisper_amd

    hid, hid_d, emb_d, ref, hist = planted(D)
    want, wtok, wfired, margins = rule_rows(ref[:B], hist, B, step)
    fin = np.isfinite(want)
    amax = np.abs(ref[:B]).max(axis=1)
    logit_bound = 4e-6 * amax + 1e-6
    # every row decides with room: nothing is excused
    planted_rows = min(B, len(PLANTS))
    assert (margins >= 100 * logit_bound).all(), (margins, logit_bound)
    if prec == 1:  # one f16 plane: the format's own bound (module docstring)
        logit_bound = f16_logit_bound(D)[:B]
        assert (margins >= 2 * logit_bound).all(), (margins, logit_bound)
    poison = torch.full((32,), 12345.0, device="cuda", dtype=torch.float32)
    tok, lp, lg, mass = whisper_amd.logits_timestamp_check(hid_d[:B].contiguous(), emb_d, hist[:B], step, TS0,
                                                           precision=prec, logprob=poison)
    _, raw = whisper_amd.logits_argmax_check(hid_d[:B].contiguous(), emb_d, 40, precision=prec)  # no mask at step 40
    tok, lp, lg = tok.cpu().numpy(), lp.cpu().numpy(), lg.cpu().numpy()
    raw, mass = raw.cpu().numpy(), mass.cpu().numpy()
    assert (lp[B:] == 12345.0).all()  # rows B .. 31 untouched
    assert np.array_equal(tok, wtok), (tok, wtok)
    assert np.array_equal(mass != 0, wfired)
    # the masks exactly: -inf where the rule masks, the kernel's own logit elsewhere
    for b in range(B):
        assert np.array_equal(np.isfinite(lg[b]), fin[b]), b
        assert np.array_equal(lg[b][fin[b]], raw[b][fin[b]]), b
    if step == STEP:
        for r in range(planted_rows):
            assert tok[r] == PLANTS[r][2], (r, tok[r], PLANTS[r][2])
    lp = lp[:B].astype(np.float64)
    lg64 = lg.astype(np.float64)
    b1 = (r_fused() + 24) * U
    err_i = np.abs(lp - (lg64[np.arange(B), tok] - lse_rows(lg64)))
    lp_ii = want[np.arange(B), wtok] - lse_rows(want)
    err_ii = np.abs(lp - lp_ii)
    bound_ii = b1 + 2 * logit_bound
    print(f"D {D} B {B} step {step} prec {prec}: (i) {err_i.max() / U:.1f} u of {b1 / U:.0f} u, "
          f"(ii) {(err_ii / bound_ii).max():.3f} of its bound, smallest margin {margins.min():.3g}")
    assert (err_i <= b1).all(), (err_i / U, b1 / U)
    assert (err_ii <= bound_ii).all(), (err_ii, bound_ii)


@pytest.mark.parametrize("prec", [0, 1])  # PREC_F16X2 (NS = 2), PREC_F16 (NS = 1)
@pytest.mark.parametrize("D", [128, 384])
def test_fused_timestamp_pick(torch, D, prec):
    """V = 51866 (the ids are absolute), B in {1, 5, 32}, with and without the
    EOT suppression; R = 77 (bound (i): 101 u).  ts0 - 1 is NO_TIMESTAMPS, a
    special id: the rule never lets it win, so rows 10 and 11 plant it as the
    raw maximum at the boundary and it must lose to ts0 / V - 1."""
    for B in (1, 5, 32):
        for step in (STEP, 0):
            check_fused(torch, D, B, step, prec)


@pytest.mark.parametrize("D", [128, 384])
def test_row_timestamp_kernel(torch, D):
    """The same planted logits, stored as f32 rows, through the row kernel:
    the tokens of the rule on those rows, and bound (i) with R = 211."""
    import whisper_amd

    _, _, _, ref, hist = planted(D)
    z32 = ref.astype(np.float32)
    zd = torch.from_numpy(z32).cuda()
    for sup in (False, True):
        want, wtok, wfired, margins = rule_rows(z32.astype(np.float64), hist, 32, 0 if sup else STEP)
        tok, lp, mass = whisper_amd.row_timestamp_check(zd, hist, TS0, suppress_eot=sup)
        tok, lp, mass = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), mass.cpu().numpy()
        ok = margins >= 1e-2  # f32 sums decide the mass rule: every row has far more room
        assert ok.all(), margins
        assert np.array_equal(tok[ok], wtok[ok]) and np.array_equal(mass[ok] != 0, wfired[ok])
        if not sup:
            assert [int(t) for t in tok[:len(PLANTS)]] == [p[2] for p in PLANTS]
        err = np.abs(lp - (want[np.arange(32), wtok] - lse_rows(want)))[ok]
        assert (err <= (r_row() + 24) * U).all(), err / U


def test_bookkeeping_records():
    """Every (last, penult) transition, t = ts0 + 1500, max_initial variants:
    the records after each launch equal the numpy restatement of the prefix."""
    import whisper_amd

    seqs = [
        [T(0), A, BT, T(5), T(5), A, T(9), T(9), T(1500 - 1), A],
        [A, A, T(3), A, T(3), T(4), A, EOT, T(1500), T(1500)],
        [T(1500), A, T(1500), T(1500), A, A, A, A, A, A],
        [T(2), T(2), T(2), A, T(7), EOT, T(8), T(8), BT, T(9)],
        [EOT, EOT, A, T(1), A, T(1), A, T(2), T(2), T(3)],
    ]
    rng = np.random.default_rng(3)
    seqs += [[int(rng.choice(POOL)) for _ in range(10)] for _ in range(40)]
    toks = np.array(seqs, np.int32)
    pairs = set()
    for mi in (50, -1):
        got = whisper_amd.timestamp_bookkeep_check(toks, TS0, V, mi)
        for s in range(toks.shape[1]):
            for r in range(toks.shape[0]):
                assert got[s, r].tolist() == tr.record(seqs[r][:s + 1], TS0, V, mi), (r, s)
                if s:
                    pairs.add((tuple(got[s - 1, r, 4:6]), tuple(got[s, r, 4:6])))
    assert len({p[1] for p in pairs}) == 4 and len(pairs) >= 8  # all four (last, penult) states, reached from each other


# ------------------------------------------------------------------ model --
def mels(n, n_mels=80, first=0):
    return np.stack([wo.synthetic_mel(first + c, n_mels) for c in range(n)]).astype(np.float32)


def oracle_timestamps(om, mel, lang, max_tokens, max_initial=50):
    """The numpy driver: whisper_oracle's encode / decoder_pass with the rule
    of ts_rules.py before every pick.  Per clip: the picks in order (an EOT
    pick that ends the clip included), and per pick its float64
    log-probability, the tolerance 2 * 2e-3 * max|finite picked logits| and the
    decision margin."""
    c = om.cfg
    B = mel.shape[0]
    tt = 50260 + c["n_lang"]
    ts0 = tt + 5
    cache = om.init_cache(om.encode(mel))
    z0 = om.decoder_pass(np.full((B, 1), wo.SOT), np.arange(1), cache, fresh=True).astype(np.float64)
    lo, hi = 50259, 50259 + c["n_lang"]
    if lang is not None:
        langs = [lang] * B
        logits = om.decoder_pass(np.array([[wo.SOT, lang, tt]] * B), np.arange(3), cache, fresh=True)
        position = 3
    else:
        langs = [lo + om.argmax_last(z0[b, lo:hi].astype(np.float32)) for b in range(B)]
        logits = om.decoder_pass(np.array([[lg, tt] for lg in langs]), np.arange(2), cache, fresh=True)
        position = 1 + 2
    seq = [[] for _ in range(B)]  # every pick fed so far (the rule's history)
    picks = [[] for _ in range(B)]  # (token, lp, tol, margin) while the clip is live
    done = [False] * B
    n_out = [0] * B

    def pick_all(logits, suppress):
        nxt = []
        for b in range(B):
            z, _, margin = tr.apply_rules(logits[b].astype(np.float64), seq[b], ts0, suppress, max_initial)
            t = tr.pick(z)
            if not done[b]:
                picks[b].append((t, z[t] - tr.lse(z), 2 * 2e-3 * np.abs(z[np.isfinite(z)]).max(), margin))
            nxt.append(t)
        return nxt

    nxt = pick_all(logits, True)
    for step in range(max_tokens):
        for b in range(B):
            if not done[b]:
                if nxt[b] == EOT:
                    done[b] = True
                else:
                    n_out[b] += 1
            seq[b].append(nxt[b])
        if all(done):
            break
        logits = om.decoder_pass(np.array(nxt)[:, None], np.array([position]), cache, fresh=False)
        position += 1
        nxt = pick_all(logits, step + 1 < wo.MIN_TOKENS)
    for b in range(B):  # picks 0 .. max_tokens - 1 reach a bookkeeping step; one more may have been taken
        picks[b] = picks[b][:max_tokens]
    ns_tok = tt + 3
    return {"picks": picks, "ts0": ts0, "lang_tok": langs, "z0tol": 2 * 2e-3 * np.abs(z0).max(axis=1),
            "no_speech": np.exp(z0[:, ns_tok] - lse_rows(z0)),
            "lang_prob": np.exp(z0[np.arange(B), langs] - lse_rows(z0[:, lo:hi]))}


def compared_steps(picks):
    """Picks of a clip that are compared: up to the first whose margin is below its tolerance."""
    k = 0
    while k < len(picks) and picks[k][3] >= picks[k][2]:
        k += 1
    return k


def got_sequence(g, max_tokens):
    """The clip's picks as returned: its tokens, then the EOT pick when its slot was stored."""
    n = len(g["tokens"])
    slots = g["logprob_slots"]
    return g["tokens"] + ([EOT] if n < max_tokens and not np.isnan(slots[n]) else [])


def check_against_driver(got, want, max_tokens):
    import whisper_amd

    total = compared = n_ts = n_text = 0
    for b, g in enumerate(got):
        picks = want["picks"][b]
        k = compared_steps(picks)
        total += len(picks)
        compared += k
        assert k >= min(8, len(picks)), (b, k)  # the cap, per clip (checked for these clips on the CPU)
        seq = got_sequence(g, max_tokens)
        assert seq[:k] == [p[0] for p in picks[:k]], (b, k, seq, [p[0] for p in picks])
        lp = g["logprob_slots"][:k].astype(np.float64)
        err = np.abs(lp - np.array([p[1] for p in picks[:k]]))
        assert (err <= np.array([p[2] for p in picks[:k]])).all(), (b, err)
        n_ts += sum(t >= want["ts0"] for t in seq)
        n_text += sum(t < want["ts0"] for t in seq)
        segs, seek = whisper_amd.segments_from_tokens(g["tokens"], want["ts0"])
        assert g["segments"] == segs and g["seek_frames"] == seek
        for key in ("no_speech", "lang_prob"):
            p, q = g[key if key == "lang_prob" else "no_speech_prob"], want[key][b]
            assert abs(p - q) <= q * math.expm1(want["z0tol"][b]) + 1e-12, (key, b, p, q)
        assert g["lang_token"] == want["lang_tok"][b]
    assert 2 * compared >= total, (compared, total)  # the cap, over all (clip, step) pairs
    print(f"compared {compared} of {total} picks; returned {n_ts} timestamp and {n_text} text picks")
    return n_ts, n_text


MODEL_TOKENS = 24
# Clips (synthetic_mel indices) on which the driver alone meets the cap with
# SEED -- every pick's margin at or above its tolerance for >= 8 picks (here:
# all 24) -- found by running the driver over clips 0 .. 44 on the CPU.  With
# auto-detect most clips sit within a factor of three of the tolerance at pick
# 1, on either side of it.
MODEL_CLIPS = {50259: [9, 10, 11], None: [8, 10, 16]}


@pytest.fixture(scope="module")
def oracle_model():
    return wo.SynthWhisper("tiny_test", SEED)


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    yield m
    m.close()


@pytest.mark.parametrize("lang", [50259, None])
@pytest.mark.parametrize("n_clips", [2, 3])
def test_transcribe_timestamps_matches_driver(torch, oracle_model, gpu_model, n_clips, lang):
    """TINY_TEST, Q4_0, 24 tokens, explicit language and auto-detect."""
    mel = np.stack([wo.synthetic_mel(c, 80) for c in MODEL_CLIPS[lang][:n_clips]]).astype(np.float32)
    want = oracle_timestamps(oracle_model, mel, lang, MODEL_TOKENS)
    got = gpu_model.transcribe_timestamps(torch.from_numpy(mel).cuda(), lang, max_tokens=MODEL_TOKENS)
    check_against_driver(got, want, MODEL_TOKENS)


def close_clip(a, b, tol, k=None):
    """Two returned clips agree: tokens (the first k picks; None: all) and scores to tol."""
    sa, sb = got_sequence(a, 10 ** 6), got_sequence(b, 10 ** 6)
    if k is None:
        assert a["tokens"] == b["tokens"]
        k = len(a["tokens"])
    assert sa[:k] == sb[:k]
    la, lb = a["logprob_slots"][:k].astype(np.float64), b["logprob_slots"][:k].astype(np.float64)
    assert np.array_equal(np.isnan(la), np.isnan(lb))
    assert np.nanmax(np.abs(la - lb), initial=0.0) <= tol, (la, lb, tol)
    for key in ("no_speech_prob", "lang_prob"):
        assert abs(a[key] - b[key]) <= b[key] * math.expm1(tol) + 1e-12, key
    assert a["lang_token"] == b["lang_token"]


def test_pipelined_timestamps_match_sequential(torch, oracle_model, monkeypatch):
    """One call of 3 batches x 17 clips: one unit of three, group j decoding
    the batch in lane j under its own rule records.  Tokens equal the three
    single-batch calls'; a clip that differs is run through the numpy driver
    and must differ only from a step on whose margin is below the tolerance
    (the excuse rule of the model test).  Scores to the logit tolerance."""
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    NB, B, n = 3, 17, 8
    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=B)
    x = torch.from_numpy(np.stack([mels(B, first=500 + i * B) for i in range(NB)])).cuda()
    prompt = torch.tensor([[50258, 50259, 50360]] * B, dtype=torch.int32, device="cuda")
    tol = 1e30
    for i in range(NB):
        m.encode(x[i])
        tol = min(tol, 2 * 2e-3 * float(m.prompt_logits(prompt).abs().amax(dim=1).min()))
    for lang in (50259, None):
        got = m.transcribe_batches_timestamps(x, lang, max_tokens=n)
        assert (m.pipeline_stats()["pairs"], m.pipeline_stats()["units3"]) == (0, 1)
        for i in range(NB):
            seq = m.transcribe_timestamps(x[i], lang, max_tokens=n)
            for c, (a, b) in enumerate(zip(got[i], seq)):
                k = None
                if a["tokens"] != b["tokens"]:
                    mel = mels(1, first=500 + i * B + c)
                    k = compared_steps(oracle_timestamps(oracle_model, mel, lang, n)["picks"][0])
                close_clip(a, b, tol, k)
                assert a["segments"] == whisper_amd.segments_from_tokens(a["tokens"], m.timestamp_begin)[0]
    m.close()


def test_timestamps_leave_other_paths_alone(torch):
    """A plain and a scored transcribe return what they returned before a
    timestamp call on the model, on the graphs they had; the mode is part of
    the step graph's key; the buffers are allocated once and counted."""
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    mel = torch.from_numpy(mels(3, first=11)).cuda()
    plain = m.transcribe(mel, 50259, max_tokens=12)
    key_plain = m.decode_graph_key(0)
    scored = m.transcribe_scored(mel, 50259, max_tokens=12)
    key_scored = m.decode_graph_key(0)
    n0 = m.device_bytes()
    ts = m.transcribe_timestamps(mel, 50259, max_tokens=12)
    key_ts = m.decode_graph_key(0)
    assert len({key_plain, key_scored, key_ts}) == 3 and min(key_plain, key_scored, key_ts) >= 0
    assert m.device_bytes() > n0
    n1 = m.device_bytes()
    assert all(c["tokens"][0] >= m.timestamp_begin for c in ts)  # the first pick is a timestamp
    assert [c["tokens"] for c in ts] != plain
    assert m.transcribe(mel, 50259, max_tokens=12) == plain
    assert m.decode_graph_key(0) == key_plain
    again = m.transcribe_scored(mel, 50259, max_tokens=12)
    assert m.decode_graph_key(0) == key_scored
    for a, b in zip(again, scored):
        assert a["tokens"] == b["tokens"]
        assert np.allclose(a["logprob_slots"], b["logprob_slots"], rtol=0, atol=1e-5, equal_nan=True)
        assert abs(a["no_speech_prob"] - b["no_speech_prob"]) <= 1e-6 and abs(a["lang_prob"] - b["lang_prob"]) <= 1e-6
    ts2 = m.transcribe_timestamps(mel, None, max_tokens=12, max_initial=-1)
    assert m.device_bytes() == n1  # allocated once
    assert m.decode_graph_key(0) == key_ts  # max_initial lives in the records, not in the graph
    assert [c["tokens"] for c in m.transcribe_timestamps(mel, 50259, max_tokens=12)] == [c["tokens"] for c in ts]
    assert len(ts2) == 3
    m.close()
