"""Temperature sampling and the fallback ladder (wa_transcribe_sampled,
wa_transcribe_fallback): what can be tested without a GPU -- the exports, the
argument checks that precede every device call, the host statement of the
noise against its numpy restatement (sample_rules.py), that restatement
against hand-computed values and the softmax it must draw from, and the
ladder rule by hand.

Noise bound.  u is compared bit for bit.  g = -log(-log u) in f32 is two
correctly-to-1-ulp logf calls: a = logf(u) carries a relative error <= 2^-23,
which log(-a) turns into an absolute error <= 2^-23 (d log a = da / a), and the
outer logf adds one ulp of its result, <= 2^-23 |g|; the negations are exact.
So |g32 - g64| <= 2^-23 (1 + |g|), with 1 % on top for the second-order terms:
2.1e-6 at the largest |g| = 16.64.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import sample_rules as sr
import whisper_amd

EINVAL = 1
V = 51866

NEW = ("wa_transcribe_sampled", "wa_transcribe_batches_sampled", "wa_transcribe_fallback", "wa_sample_noise",
       "wa_logits_pick_check", "wa_row_pick_check")


def g_bound(g64):
    return 2.0 ** -23 * 1.01 * (1.0 + np.abs(g64))


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    L = whisper_amd.lib()
    assert hasattr(L, name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def test_python_surface():
    for n in ("transcribe_sampled", "transcribe_batches_sampled", "transcribe_fallback"):
        assert callable(getattr(whisper_amd.WhisperModel, n))
    for n in ("sample_noise", "logits_sample_check", "row_sample_check"):
        assert callable(getattr(whisper_amd, n))
    assert [f[0] for f in whisper_amd.Sampling._fields_] == ["temperature", "seed", "timestamps", "max_initial"]
    assert [f[0] for f in whisper_amd.Fallback._fields_] == ["temperatures", "n_temperatures", "logprob_threshold",
                                                             "no_speech_threshold", "seed", "timestamps",
                                                             "max_initial"]


def test_entries_reject_bad_arguments():
    """Null struct, negative / NaN / inf temperature, 0 or more than 8 rungs and
    max_tokens out of range are WQ4_EINVAL before any device work (the model
    here is not a model: nothing may touch it beyond its clip capacity)."""
    L = whisper_amd.lib()
    model, mel = (ctypes.c_uint8 * 4096)(), (ctypes.c_float * 16)()
    tok, nt = (ctypes.c_int32 * 1024)(), (ctypes.c_int32 * 16)()
    addr = lambda b: ctypes.c_void_p(ctypes.addressof(b))
    f32p, u64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64)
    seed = (ctypes.c_uint64 * 8)()
    err = lambda: L.wa_last_error().decode()

    def sampling(t):
        arr = (ctypes.c_float * 8)(*([t] * 8))
        return whisper_amd.Sampling(ctypes.cast(arr, f32p), ctypes.cast(seed, u64p), 0, 50), arr

    f, g, h = L.wa_transcribe_sampled, L.wa_transcribe_batches_sampled, L.wa_transcribe_fallback
    ok, keep = sampling(0.5)
    assert f(addr(model), addr(mel), 1, 50259, 8, 1, None, tok, nt, None, None) == EINVAL and "null" in err()
    assert f(None, addr(mel), 1, 50259, 8, 1, ctypes.byref(ok), tok, nt, None, None) == EINVAL and "null" in err()
    assert g(addr(model), addr(mel), 2, 1, 50259, 8, 1, None, tok, nt, None, None) == EINVAL and "null" in err()
    for mt in (0, 225):
        assert f(addr(model), addr(mel), 1, 50259, mt, 1, ctypes.byref(ok), tok, nt, None, None) == EINVAL
        assert "max_tokens" in err()
        assert g(addr(model), addr(mel), 2, 1, 50259, mt, 1, ctypes.byref(ok), tok, nt, None, None) == EINVAL
        assert "max_tokens" in err()
    for bad in (-0.1, float("nan"), float("inf")):
        s, keep2 = sampling(bad)
        assert f(addr(model), addr(mel), 1, 50259, 8, 1, ctypes.byref(s), tok, nt, None, None) == EINVAL
        assert "temperature" in err()
        assert g(addr(model), addr(mel), 2, 1, 50259, 8, 1, ctypes.byref(s), tok, nt, None, None) == EINVAL
        assert "temperature" in err()
    nopt = whisper_amd.Sampling(None, ctypes.cast(seed, u64p), 0, 50)
    assert f(addr(model), addr(mel), 1, 50259, 8, 1, ctypes.byref(nopt), tok, nt, None, None) == EINVAL

    def fallback(temps, n=None):
        arr = (ctypes.c_float * 16)(*temps)
        return whisper_amd.Fallback(ctypes.cast(arr, f32p), len(temps) if n is None else n, -1.0, 0.6,
                                    ctypes.cast(seed, u64p), 0, 50), arr

    assert h(addr(model), addr(mel), 1, 50259, 8, 1, None, tok, nt, None, None, None) == EINVAL and "null" in err()
    for n in (0, 9):
        fb, keep3 = fallback([0.0] * 9, n)
        assert h(addr(model), addr(mel), 1, 50259, 8, 1, ctypes.byref(fb), tok, nt, None, None, None) == EINVAL
        assert "rungs" in err()
    for bad in (-1.0, float("nan"), float("inf")):
        fb, keep3 = fallback([0.0, bad])
        assert h(addr(model), addr(mel), 1, 50259, 8, 1, ctypes.byref(fb), tok, nt, None, None, None) == EINVAL
        assert "temperature" in err()
    fb, keep3 = fallback([0.0, 0.5])
    for mt in (0, 225):
        assert h(addr(model), addr(mel), 1, 50259, mt, 1, ctypes.byref(fb), tok, nt, None, None, None) == EINVAL
        assert "max_tokens" in err()
    # the host-only noise entry
    assert L.wa_sample_noise(0, -1, 0, 4, None, None) == EINVAL


def test_mix_by_hand():
    """splitmix64's published stream from state 0 is mix(GOLD), mix(2 GOLD), ...:
    0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4; and mix(0) = 0, mix(1) worked by hand."""
    assert sr.mix(0) == 0
    assert sr.mix(sr.GOLD) == 0xE220A8397B1DCDAF
    assert sr.mix((2 * sr.GOLD) & sr.M64) == 0x6E789E6AA1B965F4
    # x = 1: x ^ (x >> 30) = 1; * C1 = C1; C1 ^ (C1 >> 27); * C2; ^ (>> 31)
    x = sr.C1
    x ^= x >> 27
    x = (x * sr.C2) & sr.M64
    x ^= x >> 31
    assert sr.mix(1) == x == 0x5692161D100B05E5
    # the array form is the scalar form
    a = np.array([0, 1, sr.GOLD, sr.M64], np.uint64)
    assert [int(v) for v in sr.mix(a)] == [sr.mix(int(v)) for v in a]
    assert sr.pick_key(0, 0) == 0xE220A8397B1DCDAF  # the key of seed 0's prompt pick


@pytest.mark.parametrize("seed,pick", [(0, 0), (2 ** 64 - 1, 0), (1234, 7), (0xDEADBEEFCAFEF00D, 224), (1, 1)])
def test_noise_matches_reference(seed, pick):
    """Every id of a row: u bit for bit, exactly representable in f32 and
    strictly inside (0, 1); g within the bound of the module docstring, and finite."""
    ids = np.arange(V)
    u64, g64 = sr.noise(seed, pick, ids)
    u, g = whisper_amd.sample_noise(seed, pick, 0, V)
    assert u.dtype == np.float32 and g.dtype == np.float32
    assert np.array_equal(u64.astype(np.float32).astype(np.float64), u64)  # representable
    assert np.array_equal(u.astype(np.float64), u64)
    assert (u64 >= 2.0 ** -24).all() and (u64 <= 1 - 2.0 ** -24).all() and (u > 0).all() and (u < 1).all()
    assert np.isfinite(g).all() and g64.min() >= -2.82 and g64.max() <= 16.64
    err = np.abs(g.astype(np.float64) - g64)
    assert (err <= g_bound(g64)).all(), (err / g_bound(g64)).max()
    # a window in the middle of the row is the same noise (id0 is an offset, not a restart)
    u2, g2 = whisper_amd.sample_noise(seed, pick, 40000, 100)
    assert np.array_equal(u2, u[40000:40100]) and np.array_equal(g2, g[40000:40100])


def test_noise_extremes_are_finite():
    """h = 0 and h = 2^23 - 1: g = 2.8134 (negated) and 16.6355, both finite in f32."""
    for h, want in ((0, -math.log(-math.log(2.0 ** -24))), (2 ** 23 - 1, -math.log(-math.log(1 - 2.0 ** -24)))):
        u = np.float32((h + 0.5) * 2.0 ** -23)
        assert float(u) == (h + 0.5) * 2.0 ** -23 and 0 < u < 1
        g = -np.log(-np.log(u, dtype=np.float32), dtype=np.float32)
        assert np.isfinite(g) and abs(float(g) - want) <= g_bound(want)


def test_gumbel_max_draws_from_the_tempered_softmax():
    """2e5 seeds (0 .. 199999, pick 3) over an 8-way row at T = 0.7: the picks'
    frequencies against softmax(z / T).  Pearson's chi-square has 7 degrees of
    freedom; its 99.9th percentile is 24.32, the bound.  Fixed seeds: the test
    is deterministic."""
    z = np.array([1.2, 0.3, -0.5, 0.9, 0.0, -1.4, 0.6, 1.0])
    T, N, pick = 0.7, 200000, 3
    seeds = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = sr.mix(seeds + np.uint64((sr.GOLD * (pick + 1)) & sr.M64))
    assert int(k[5]) == sr.pick_key(5, pick)
    h = sr.mix(k[:, None] ^ np.arange(8, dtype=np.uint64)[None, :]) >> np.uint64(41)
    g = -np.log(-np.log((h.astype(np.float64) + 0.5) * 2.0 ** -23))
    picks = np.argmax(z + T * g, axis=1)
    assert picks[5] == sr.pick(sr.keys(z, T, 5, pick))  # the vectorised draw is the reference's
    p = np.exp(z / T) / np.exp(z / T).sum()
    obs = np.bincount(picks, minlength=8)
    chi2 = float(((obs - N * p) ** 2 / (N * p)).sum())
    print(f"chi-square {chi2:.2f} on 7 degrees of freedom")
    assert chi2 <= 24.32


def test_keys_edge_cases():
    z = np.array([0.5, -np.inf, 0.5, 0.1])
    assert np.array_equal(sr.keys(z, 0.0, 9, 1), z) and sr.pick(sr.keys(z, 0.0, 9, 1)) == 2  # T = 0: greedy, last maximum
    k = sr.keys(z, 1.0, 9, 1)
    assert k[1] == -np.inf and np.isfinite(k[[0, 2, 3]]).all()  # a masked logit stays masked
    assert sr.key_gap(np.array([1.0, 3.0, 2.5, -np.inf])) == 0.5


def test_ladder_rule_by_hand():
    thr, ns = -1.0, 0.6
    good, poor, silent = (-0.4, 0.1), (-1.7, 0.1), (-1.7, 0.9)
    # passes at rung 0; fails twice then passes at rung 2; never passes: the last rung; silence stays at 0
    rungs = [[good, poor, poor, silent], [good, poor, poor, poor], [good, good, poor, poor]]
    assert sr.ladder(rungs, thr, ns) == [0, 2, 2, 0]
    assert sr.ladder(rungs[:2], thr, ns) == [0, 1, 1, 0]  # the never-passing clip keeps the last rung run
    # NaN thresholds switch the tests off: no log-probability test, nobody moves; no silence test, clip 3 moves
    nan = float("nan")
    assert sr.ladder(rungs, nan, ns) == [0, 0, 0, 0]
    assert sr.ladder(rungs, thr, nan) == [0, 2, 2, 2]
    assert sr.ladder(rungs, math.inf, nan) == [2, 2, 2, 2]
    assert sr.ladder(rungs, math.inf, 0.0) == [0, 0, 0, 0]  # every clip is "silence" above 0
    # the mean is over the non-NaN slots
    assert sr.mean_logprob(np.array([-1.0, -2.0, np.nan, np.nan], np.float32)) == -1.5
    assert sr.needs_next(-1.0, 0.0, -1.0, 0.6) is False  # strictly below the threshold
