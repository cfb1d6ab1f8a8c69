"""Scored transcribes on the GPU (wa_transcribe_scored, include/whisper_amd.h):
per-token log-probabilities from the fused logits + greedy-pick kernel, the
row kernel behind the stored-logits scores, and the model-level scores against
the numpy oracle.

Bounds.  u = 2^-24 (f32 unit roundoff).
  (i)  a kernel's log-probability against float64 numpy on the kernel's OWN
       f32 logits: |lp - lp64| <= (R + 24) u, R the longest chain of f32
       additions in the reduction as built, 24 for the rounding of v - m on the
       terms that matter, expf, the rescale multiply and logf.
         fused kernel (pick_from_lds<1, 1, 0>): a thread adds its 16 terms
           to 0 (16 additions), 3 shuffle adds, the last workgroup's thread
           adds ceil(groups / 8) rescaled candidates to 0, 3 shuffle adds:
           R = 22 + ceil(ceil(V / 128) / 8)  (73 at V = 51866, 23 to V = 1024).
         row kernel (row_logprob_kernel): ceil((hi - lo) / 256) additions per
           thread, 6 shuffle adds, 3 adds over the waves:
           R = 9 + ceil((hi - lo) / 256).
  (ii) the fused kernel against hid @ emb.T in float64: bound (i) plus twice
       the logit bound 4e-6 max|ref| + 1e-6 of test_kernels_gpu.py
       (log-sum-exp is 1-Lipschitz in the sup norm; once for z[tok], once for
       the normaliser).
  Model level: the module tolerance of test_model_gpu.py on logits,
       2e-3 max|oracle logits|, applied to the value and to the normaliser:
       2 * 2e-3 * max|finite picked logits|; through exp for probabilities.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import whisper_oracle as wo

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EOT = 50257
SEED = 1234


def r_fused(V):
    return 22 + math.ceil(math.ceil(V / 128) / 8)


def r_row(lo, hi):
    return 9 + math.ceil((hi - lo) / 256)


def lse64(z):
    """logsumexp of float64 rows (-inf entries add 0)."""
    m = z.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))[..., 0]


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


# ------------------------------------------------------------ fused kernel --
@functools.lru_cache(maxsize=None)
def planted(V, D):
    """32 hidden rows and an embedding with planted rows (on the device once,
    the float64 logits once).  Row 0: an exact tie of the maximum between two
    identical embedding rows; row 1: EOT the raw maximum with a runner-up
    (V > EOT only); row 2: a tie with the last vocabulary row; row 3: hidden
    row scaled until its maximum logit exceeds 100; row 4: one logit 30 above
    the rest (planted last); rows 5 ..: plain."""
    import torch

    rng = np.random.default_rng(V * 31 + D)
    emb = (rng.uniform(-1, 1, (V, D)) * 0.03).astype(np.float32)
    hid = rng.standard_normal((32, D)).astype(np.float32)
    big = hid / np.linalg.norm(hid, axis=1, keepdims=True)
    ids = {"tie": (V // 50, V * 3 // 4), "last": (7, V - 1), "peak": V // 3 + 1}
    emb[ids["tie"][0]] = emb[ids["tie"][1]] = big[0] * 3.0
    if V > EOT:
        emb[EOT] = big[1] * 3.0
        emb[50100] = big[1] * 2.5
    emb[ids["last"][0]] = emb[ids["last"][1]] = big[2] * 3.0
    z3 = hid[3].astype(np.float64) @ emb.astype(np.float64).T
    hid[3] *= np.float32(2.0 ** math.ceil(math.log2(110.0 / z3.max())))
    z4 = hid[4].astype(np.float64) @ emb.astype(np.float64).T
    z4[ids["peak"]] = -np.inf
    emb[ids["peak"]] = (big[4].astype(np.float64) * (z4.max() + 30.0) / np.linalg.norm(hid[4])).astype(np.float32)
    ref = hid.astype(np.float64) @ emb.astype(np.float64).T
    return hid, torch.from_numpy(hid).cuda(), torch.from_numpy(emb).cuda(), ref, ids


def check_fused(torch, V, D, B, step):
    import whisper_amd

    hid, hid_d, emb_d, ref, ids = planted(V, D)
    ref = ref[:B].copy()
    if step + 1 < 3 and V > EOT:
        ref[:, EOT] = -np.inf
    poison = torch.full((32,), 12345.0, device="cuda", dtype=torch.float32)
    tok, lp, lg = whisper_amd.logits_logprob_check(hid_d[:B].contiguous(), emb_d, step, logprob=poison)
    tok0, _ = whisper_amd.logits_argmax_check(hid_d[:B].contiguous(), emb_d, step, want_logits=False)
    tok, lp, lg = tok.cpu().numpy(), lp.cpu().numpy(), lg.cpu().numpy().astype(np.float64)
    assert np.array_equal(tok, tok0.cpu().numpy())
    assert (lp[B:] == 12345.0).all()  # rows B .. 31 untouched
    lp = lp[:B].astype(np.float64)
    b1 = (r_fused(V) + 24) * U
    # (i) the reduction, on the kernel's own logit rows
    lp_i = lg[np.arange(B), tok] - lse64(lg)
    assert np.array_equal(lg[np.arange(B), tok], lg.max(axis=1))
    err_i = np.abs(lp - lp_i)
    # (ii) the whole kernel, against float64 logits
    fin = np.isfinite(ref)
    amax = np.abs(np.where(fin, ref, 0.0)).max(axis=1)
    lp_ii = ref[np.arange(B), tok] - lse64(ref)
    err_ii = np.abs(lp - lp_ii)
    print(f"V {V} D {D} B {B} step {step}: (i) {err_i.max() / U:.1f} u of {b1 / U:.0f} u, "
          f"(ii) {(err_ii / (b1 + 2 * (4e-6 * amax + 1e-6))).max():.3f} of its bound")
    assert (err_i <= b1).all(), (err_i / U, b1 / U)
    assert (err_ii <= b1 + 2 * (4e-6 * amax + 1e-6)).all(), (err_ii, amax)
    # planted rows
    a, b = ids["tie"]
    assert lg[0, a] == lg[0, b] and tok[0] == b
    assert abs(lp[0] + math.log(2.0)) <= 1e-5  # both maxima count in S; the rest is e^-100 away
    if B > 1 and V > EOT:
        assert tok[1] == (50100 if step + 1 < 3 else EOT)
        if step + 1 < 3:
            assert lg[1, EOT] == -np.inf
    if B > 2:
        assert tok[2] == V - 1
    if B > 3:
        assert lg[3].max() > 100.0  # a sum without max-subtraction overflows f32
        assert np.isfinite(lp[3])
    if B > 4:
        assert tok[4] == ids["peak"] and -1e-6 <= lp[4] <= 0.0  # S is about 1


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("V", [26, 128, 410])
def test_fused_logprob_small_vocab(torch, V, D):
    """V = 26: one partial workgroup; 128: one full; 410: three full and a
    26-row tail.  R = 23 (bound (i): 47 u)."""
    for B in (1, 6, 32):
        for step in (0, 40):
            check_fused(torch, V, D, B, step)


@pytest.mark.parametrize("B", [1, 6, 32])
def test_fused_logprob_large_v3_vocab(torch, B):
    """V = 51866, D = 1280 (the shape of test_logits_argmax_ties_and_eot):
    406 workgroups, R = 73 (bound (i): 97 u); EOT masked at step 0."""
    for step in (0, 40):
        check_fused(torch, 51866, 1280, B, step)


@pytest.mark.parametrize("V,D", [(410, 128), (51866, 1280)])
def test_fused_logprob_flat_row(torch, V, D):
    """Identical embedding rows give identical logits: S = V exactly and
    lp = -log V -- at V = 51866 and step 0, -log(V - 1): EOT left the sum."""
    import whisper_amd

    rng = np.random.default_rng(V)
    row = (rng.uniform(-1, 1, D) * 0.03).astype(np.float32)
    emb = torch.from_numpy(np.tile(row, (V, 1))).cuda()
    hid = torch.from_numpy(rng.standard_normal((3, D)).astype(np.float32)).cuda()
    for step in (0, 2, 40):
        tok, lp, lg = whisper_amd.logits_logprob_check(hid, emb, step)
        n = V - 1 if (step + 1 < 3 and V > EOT) else V
        lg = lg.cpu().numpy()
        assert (np.isfinite(lg).sum(axis=1) == n).all()
        assert (tok.cpu().numpy() == V - 1).all()
        err = np.abs(lp.cpu().numpy().astype(np.float64) + math.log(n))
        assert (err <= (r_fused(V) + 24) * U).all(), (step, err / U)


# -------------------------------------------------------------- row kernel --
@pytest.mark.parametrize("V", [26, 410, 51866])
def test_row_logprob_kernel(torch, V):
    """z[id] - logsumexp(z[lo:hi]) over stored rows: the full range and
    sub-ranges (the language range at V = 51866), EOT masked or not, ids from
    an array and fixed, a row with -inf entries; bound (i) with R = 9 +
    ceil((hi - lo) / 256).  Unit-variance rows keep |lp| < 16, where the
    rounding of v - m, logf and the result fit the 24 u of the bound."""
    import whisper_amd

    rng = np.random.default_rng(V + 5)
    R = 5
    z = rng.standard_normal((R, V)).astype(np.float32)
    z[1, rng.choice(V, V // 3, replace=False)] = -np.inf
    if V > EOT:
        z[2, EOT] = 12.0  # EOT the raw maximum of row 2, more than half of its sum
        z[:, 5] = 0.25  # column 5 finite in every row (the fixed id of the masking check below)
    zd = torch.from_numpy(z).cuda()
    ranges = [(0, V), (3, 20), (V - 7, V)]
    if V > 300:
        ranges += [(1, 258), (130, 131 + 256)]
    if V > EOT:
        ranges += [(50259, 50359), (50000, 50300)]
    worst = 0.0
    for lo, hi in ranges:
        for mask in (False, True):
            z64 = z.astype(np.float64)
            if mask and V > EOT:
                z64[:, EOT] = -np.inf
            sub = z64[:, lo:hi]
            want_lse = lse64(sub)
            # ids: each row's (masked) maximum, then arbitrary finite entries
            arg = lo + np.argmax(sub, axis=1)
            rnd = np.array([lo + rng.choice(np.flatnonzero(np.isfinite(sub[r]))) for r in range(R)])
            for ids in (arg, rnd):
                got = whisper_amd.row_logprob_check(zd, lo, hi, mask, idx=torch.from_numpy(ids.astype(np.int32)).cuda())
                err = np.abs(got.cpu().numpy().astype(np.float64) - (z64[np.arange(R), ids] - want_lse))
                worst = max(worst, err.max() / ((r_row(lo, hi) + 24) * U))
                assert (err <= (r_row(lo, hi) + 24) * U).all(), (lo, hi, mask, err / U)
            cols = np.flatnonzero(np.isfinite(sub).all(axis=0))  # one id for every row: finite in all of them
            fixed = lo + int(cols[len(cols) // 2])
            got = whisper_amd.row_logprob_check(zd, lo, hi, mask, fixed_idx=fixed)
            err = np.abs(got.cpu().numpy().astype(np.float64) - (z64[:, fixed] - want_lse))
            assert (err <= (r_row(lo, hi) + 24) * U).all(), (lo, hi, mask, "fixed", err / U)
    print(f"row kernel V {V}: worst error {worst:.3f} of bound (i)")
    # an id outside the range is NaN
    assert np.isnan(whisper_amd.row_logprob_check(zd, 3, 20, fixed_idx=21).cpu().numpy()).all()
    if V > EOT:  # masked, the raw maximum EOT leaves the sum: the runner-up's lp rises
        a = whisper_amd.row_logprob_check(zd, 0, V, False, fixed_idx=5).cpu().numpy()
        b = whisper_amd.row_logprob_check(zd, 0, V, True, fixed_idx=5).cpu().numpy()
        assert (b >= a).all() and b[2] > a[2] + 0.5


# ------------------------------------------------------------------- model --
def mels(n, n_mels=80, first=0):
    return np.stack([wo.synthetic_mel(first + c, n_mels) for c in range(n)]).astype(np.float32)


@pytest.fixture(scope="module")
def oracle_model():
    return wo.SynthWhisper("tiny_test", SEED)


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    yield m
    m.close()


def oracle_scores(om, mel, lang, max_tokens):
    """Tokens, per-slot float64 log-probabilities with their tolerances (NaN
    where the definition leaves a slot empty) and the SOT-position scores."""
    trace = {}
    toks = om.transcribe(mel, lang, max_tokens=max_tokens, trace=trace)
    picked = trace["picked"]
    B = mel.shape[0]
    lp = np.full((B, max_tokens + 1), np.nan)
    tol = np.zeros((B, max_tokens + 1))
    for b in range(B):
        n = len(toks[b])
        seq = list(toks[b]) + ([EOT] if n < max_tokens else [])  # a clip short of max_tokens stopped on EOT
        for s, t in enumerate(seq):
            row = picked[s][b].astype(np.float64)
            lp[b, s] = row[t] - lse64(row)
            tol[b, s] = 2 * 2e-3 * np.abs(row[np.isfinite(row)]).max()
    cache = om.init_cache(trace["enc"])
    z0 = om.decoder_pass(np.full((B, 1), wo.SOT), np.arange(1), cache, fresh=True).astype(np.float64)
    c = om.cfg
    lo, hi = 50259, 50259 + c["n_lang"]
    ns_tok = 50260 + c["n_lang"] + 3
    det = [lo + om.argmax_last(z0[b, lo:hi].astype(np.float32)) for b in range(B)]
    lang_tok = det if lang is None else [lang] * B
    return {"tokens": toks, "lp": lp, "tol": tol, "z0tol": 2 * 2e-3 * np.abs(z0).max(axis=1),
            "no_speech": np.exp(z0[:, ns_tok] - lse64(z0)), "lang_tok": lang_tok,
            "lang_prob": np.exp(z0[np.arange(B), lang_tok] - lse64(z0[:, lo:hi]))}


def check_against_oracle(got, want, max_tokens):
    for b, g in enumerate(got):
        assert g["tokens"] == want["tokens"][b]
        slots = g["logprob_slots"]
        assert slots.shape == (max_tokens + 1,)
        assert np.array_equal(np.isnan(slots), np.isnan(want["lp"][b])), (b, slots, want["lp"][b])
        k = ~np.isnan(slots)
        err = np.abs(slots[k].astype(np.float64) - want["lp"][b][k])
        print(f"clip {b}: {k.sum()} slots, worst error {err.max():.2e}, tolerance {want['tol'][b][k].min():.2e}")
        assert (err <= want["tol"][b][k]).all(), (b, err, want["tol"][b][k])
        assert len(g["token_logprob"]) == k.sum() and np.array_equal(g["token_logprob"], slots[k])
        assert abs(g["avg_logprob"] - np.mean(slots[k].astype(np.float64))) <= 1e-6
        # probabilities: the log tolerance through exp
        for key in ("no_speech", "lang_prob"):
            p, q = g[key if key == "lang_prob" else "no_speech_prob"], want[key][b]
            assert abs(p - q) <= q * math.expm1(want["z0tol"][b]) + 1e-12, (key, b, p, q)
        assert g["lang_token"] == want["lang_tok"][b]


@pytest.fixture(scope="module")
def scored_runs(torch, oracle_model, gpu_model):
    """transcribe_scored of mels(2), 32 tokens, explicit and auto language, with the oracle's scores."""
    mel = mels(2)
    out = {}
    for lang in (50259, None):
        out[lang] = (gpu_model.transcribe_scored(torch.from_numpy(mel).cuda(), lang, max_tokens=32),
                     oracle_scores(oracle_model, mel, lang, 32))
    return out


@pytest.mark.parametrize("lang", [50259, None])
def test_transcribe_scored_matches_oracle(torch, gpu_model, scored_runs, lang):
    got, want = scored_runs[lang]
    plain = gpu_model.transcribe(torch.from_numpy(mels(2)).cuda(), lang, max_tokens=32)
    assert [g["tokens"] for g in got] == plain
    check_against_oracle(got, want, 32)


def test_no_speech_is_causal(scored_runs):
    """The explicit prompt's SOT row (row 0 of four) equals the auto-detect
    prompt's single-SOT pass up to the logit tolerance."""
    (exp, want), (auto, _) = scored_runs[50259], scored_runs[None]
    for b in range(2):
        p, q = exp[b]["no_speech_prob"], auto[b]["no_speech_prob"]
        assert abs(p - q) <= q * math.expm1(want["z0tol"][b]) + 1e-12, (b, p, q)


def test_eot_slot(torch, tmp_path):
    """The scaled-EOT-embedding checkpoint of test_ragged_eot_stop_matches_oracle:
    clips stop at different steps; a clip that stopped on EOT has the EOT
    pick's log-probability in slot n, a clip that ran out has NaN there."""
    import whisper_amd
    import write_gguf

    tensors = write_gguf.synthetic_tensors("tiny_test", SEED)
    tensors["decoder.token_embedding.weight"][wo.EOT] *= 10.0
    p = tmp_path / "eot.gguf"
    write_gguf.write_gguf(str(p), tensors, "eot")
    g = whisper_amd.WhisperModel.from_gguf(str(p), "tiny_test", max_batch=6)
    ref = wo.SynthWhisper("tiny_test", SEED)
    ref.w["decoder.token_embedding.weight"][wo.EOT] *= 10.0
    mel = mels(6, first=30)
    want = oracle_scores(ref, mel, 50259, 24)
    lens = [len(t) for t in want["tokens"]]
    assert min(lens) < 24 and max(lens) == 24 and len(set(lens)) > 1, lens  # ragged: some stop, some run out
    got = g.transcribe_scored(torch.from_numpy(mel).cuda(), 50259, max_tokens=24)
    check_against_oracle(got, want, 24)
    for b, n in enumerate(lens):
        slot = got[b]["logprob_slots"][n]
        assert np.isnan(slot) if n == 24 else np.isfinite(slot)
        assert len(got[b]["token_logprob"]) == (n if n == 24 else n + 1)
    g.close()


def close_scores(a, b, tol):
    assert a["tokens"] == b["tokens"]
    sa, sb = a["logprob_slots"], b["logprob_slots"]
    assert np.array_equal(np.isnan(sa), np.isnan(sb))
    k = ~np.isnan(sa)
    assert np.abs(sa[k].astype(np.float64) - sb[k]).max() <= tol, (sa, sb, tol)
    for key in ("no_speech_prob", "lang_prob"):
        assert abs(a[key] - b[key]) <= b[key] * math.expm1(tol) + 1e-12, key
    assert a["lang_token"] == b["lang_token"]


def logit_tolerance(m, mel):
    """2 * 2e-3 * max|logit|, the logit scale taken from the clips' prompt rows
    (the smallest clip maximum: the tightest tolerance)."""
    import torch

    m.encode(mel)
    prompt = torch.tensor([[50258, 50259, 50360, 50364]] * mel.shape[0], dtype=torch.int32, device="cuda")
    return 2 * 2e-3 * float(m.prompt_logits(prompt).abs().amax(dim=1).min())


def test_two_groups_match_single_group(torch):
    """16 clips decode in two groups of 8, each with its own score buffers and
    step graph; the same clips two at a time take one group."""
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=16)
    mel = torch.from_numpy(mels(16, first=20)).cuda()
    tol = logit_tolerance(m, mel)
    for lang in (50259, None):
        got = m.transcribe_scored(mel, lang, max_tokens=8)
        assert [g["tokens"] for g in got] == m.transcribe(mel, lang, max_tokens=8)
        for c0 in range(0, 16, 2):
            for a, b in zip(got[c0:c0 + 2], m.transcribe_scored(mel[c0:c0 + 2], lang, max_tokens=8)):
                close_scores(a, b, tol)
    m.close()


@pytest.mark.parametrize("NB,B,units", [(3, 17, (0, 1)), (2, 16, (1, 0))])
def test_pipelined_scores_match_sequential(torch, monkeypatch, NB, B, units):
    """transcribe_batches_scored: three batches of 17 clips form one unit of
    three, two of 16 a pair -- group j scores the batch in lane j.  A unit may
    use another frame split than the sequential call: equal tokens, scores to
    the logit tolerance."""
    import whisper_amd

    monkeypatch.delenv("WA_ENC_OVERLAP", raising=False)
    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=B)
    x = torch.from_numpy(np.stack([mels(B, first=500 + i * B) for i in range(NB)])).cuda()
    tol = min(logit_tolerance(m, x[i]) for i in range(NB))
    for lang in (50259, None):
        got = m.transcribe_batches_scored(x, lang, max_tokens=8)
        assert (m.pipeline_stats()["pairs"], m.pipeline_stats()["units3"]) == units
        assert [[g["tokens"] for g in bt] for bt in got] == m.transcribe_batches(x, lang, max_tokens=8)
        for i in range(NB):
            for a, b in zip(got[i], m.transcribe_scored(x[i], lang, max_tokens=8)):
                close_scores(a, b, tol)
    m.close()


def test_scoring_leaves_unscored_path_alone(torch):
    """The graph key of a plain transcribe is what it was before any scored
    call on the model, and a plain call after a scored one returns the plain
    call's tokens."""
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=4)
    mel = torch.from_numpy(mels(3, first=11)).cuda()
    before = m.transcribe(mel, 50259, max_tokens=12)
    n0 = m.device_bytes()  # after the first few-clip transcribe allocated its cross K / V caches
    key = m.decode_graph_key(0)
    assert key >= 0
    scored = m.transcribe_scored(mel, 50259, max_tokens=12)
    assert m.decode_graph_key(0) != key  # scoring is part of the step graph's key
    assert m.device_bytes() > n0  # the score buffers, counted
    n1 = m.device_bytes()
    assert m.transcribe(mel, 50259, max_tokens=12) == before
    assert m.decode_graph_key(0) == key
    assert [g["tokens"] for g in scored] == before
    m.transcribe_scored(mel, None, max_tokens=12)
    assert m.device_bytes() == n1  # allocated once
    m.close()
