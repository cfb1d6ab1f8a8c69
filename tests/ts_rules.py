"""Numpy restatement of the timestamp rules (include/whisper_amd.h,
wa_transcribe_timestamps: masks a-f, then the pick), the reference of
test_timestamps.py and test_timestamps_gpu.py.  A helper module, not a test.
"""
from __future__ import annotations

import numpy as np

EOT = 50257
NEG = -np.inf


def lse(z) -> float:
    """logsumexp of a float64 vector; -inf when nothing is finite."""
    z = np.asarray(z, np.float64)
    m = z.max() if z.size else NEG
    if not np.isfinite(m):
        return NEG
    return float(m + np.log(np.exp(z - m).sum()))


def history_flags(s, ts0):
    last = len(s) >= 1 and s[-1] >= ts0
    penult = len(s) < 2 or s[-2] >= ts0
    ts = [t for t in s if t >= ts0]
    return last, penult, (ts[-1] if ts else None)


def masks_ae(z, s, ts0, suppress_eot, max_initial=50):
    """z (float64 [V]) after masks a-e for the sampled tokens s."""
    z = np.array(z, np.float64)
    if suppress_eot:  # a
        z[EOT] = NEG
    z[EOT + 1:ts0] = NEG  # b
    last, penult, t = history_flags(s, ts0)
    if last and penult:  # c
        z[ts0:] = NEG
    elif last:
        z[:EOT] = NEG
    if t is not None:  # d
        z[ts0:(t if (last and not penult) else t + 1)] = NEG
    if len(s) == 0:  # e
        z[:ts0] = NEG
        if max_initial >= 0:
            z[ts0 + max_initial + 1:] = NEG
    return z


def apply_rules(z, s, ts0, suppress_eot, max_initial=50):
    """(z after a-f, rule f fired, the decision margin).  The margin is the
    smaller of the allowed set's top-2 gap (between distinct values; inf with
    one) and |lse_ts - max_text| (inf when a side is empty)."""
    z = masks_ae(z, s, ts0, suppress_eot, max_initial)
    lse_ts, mt = lse(z[ts0:]), float(z[:ts0].max())
    fired = lse_ts > mt
    m_mass = abs(lse_ts - mt) if np.isfinite(lse_ts) and np.isfinite(mt) else np.inf
    if fired:
        z[:ts0] = NEG
    # distinct values: bit-equal logits (identical embedding rows) are equal in
    # every arithmetic and the pick resolves them by index, not by value
    top = np.unique(z[np.isfinite(z)])[-2:]
    m_top = float(top[1] - top[0]) if top.size == 2 else np.inf
    return z, bool(fired), min(m_top, m_mass)


def pick(z) -> int:
    """The largest value, the largest index among equal maxima."""
    return int(len(z) - 1 - np.argmax(z[::-1]))


def record(s, ts0, V, max_initial=50):
    """The rule record [text_ok, ts_lo, ts_hi, first, last, penult, t_last, 0]
    of the history s, from the history itself (the kernel advances it token by
    token)."""
    if len(s) == 0:
        return [0, ts0, V - 1 if max_initial < 0 else min(V - 1, ts0 + max_initial), 1, 0, 1, -1, 0]
    last, penult, t = history_flags(s, ts0)
    t = -1 if t is None else t
    if last and penult:
        text_ok, lo = 1, V
    elif last:
        text_ok, lo = 0, t
    else:
        text_ok, lo = 1, (t + 1 if t >= 0 else ts0)
    return [text_ok, lo, V - 1, 0, int(last), int(penult), t, 0]


def allowed_from_record(rec, ts0, V, suppress_eot):
    """Boolean [V]: the ids a record leaves after masks a-e (how the kernels read it)."""
    text_ok, lo, hi, first = rec[:4]
    ok = np.zeros(V, bool)
    ok[:EOT] = bool(text_ok)
    ok[EOT] = not (suppress_eot or first)
    ids = np.arange(ts0, V)
    ok[ts0:] = (ids >= lo) & (ids <= hi)
    return ok
