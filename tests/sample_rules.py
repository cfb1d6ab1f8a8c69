"""Numpy restatement of temperature sampling and the fallback ladder
(include/whisper_amd.h, wa_transcribe_sampled / wa_transcribe_fallback), the
reference of test_sampling.py and test_sampling_gpu.py.  A helper module, not
a test.  It composes with ts_rules.apply_rules for the timestamp form: the
rules mask the row first, the keys are taken over what they leave.
"""
from __future__ import annotations

import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix(x):
    """splitmix64's finaliser on uint64 (a Python int or an array), wrapping."""
    if isinstance(x, (int, np.integer)):
        x = int(x) & M64
        x ^= x >> 30
        x = (x * C1) & M64
        x ^= x >> 27
        x = (x * C2) & M64
        return x ^ (x >> 31)
    x = np.asarray(x, np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(C1)
        x ^= x >> np.uint64(27)
        x *= np.uint64(C2)
        x ^= x >> np.uint64(31)
    return x


def pick_key(seed: int, pick: int) -> int:
    return mix((int(seed) + GOLD * (int(pick) + 1)) & M64)


def noise(seed: int, pick: int, ids):
    """(u, g) of the token ids at (seed, pick): u float64 (every value exactly
    representable in f32, strictly inside (0, 1)), g = -log(-log(u)) float64."""
    ids = np.asarray(ids, np.uint64)
    h = mix(np.uint64(pick_key(seed, pick)) ^ ids) >> np.uint64(41)
    u = (h.astype(np.float64) + 0.5) * 2.0 ** -23
    return u, -np.log(-np.log(u))


def keys(z, T: float, seed: int, pick: int):
    """key_v = z_v + T g_v in float64; T = 0 evaluates no noise; -inf stays -inf."""
    z = np.asarray(z, np.float64)
    if T == 0:
        return z.copy()
    _, g = noise(seed, pick, np.arange(z.shape[-1]))
    return np.where(np.isfinite(z), z + float(T) * g, z)


def pick(k) -> int:
    """The largest key, the largest index among equal keys."""
    k = np.asarray(k)
    return int(len(k) - 1 - np.argmax(k[::-1]))


def key_gap(k) -> float:
    """The gap between the two largest keys (inf with fewer than two finite)."""
    f = k[np.isfinite(k)]
    if f.size < 2:
        return np.inf
    top = np.partition(f, f.size - 2)[-2:]
    return float(top[1] - top[0])


def mean_logprob(slots) -> float:
    """The mean of the non-NaN log-probability slots of a clip (float64)."""
    s = np.asarray(slots, np.float64)
    return float(s[~np.isnan(s)].mean())


def needs_next(mean_lp: float, no_speech: float, logprob_threshold: float, no_speech_threshold: float) -> bool:
    """The ladder rule after a rung; a NaN threshold makes its comparison false."""
    return bool(mean_lp < logprob_threshold) and not bool(no_speech > no_speech_threshold)


def ladder(results_per_rung, logprob_threshold: float, no_speech_threshold: float):
    """results_per_rung[r][c] = (mean_lp, no_speech_prob) of clip c decoded at
    rung r.  The rung each clip keeps: the first it passes, else the last."""
    R, B = len(results_per_rung), len(results_per_rung[0])
    out = []
    for c in range(B):
        r = 0
        while r < R - 1 and needs_next(*results_per_rung[r][c], logprob_threshold, no_speech_threshold):
            r += 1
        out.append(r)
    return out
