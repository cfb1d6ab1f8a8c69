"""Numpy restatement of the suppress-token lists (include/whisper_amd.h,
"Suppress-token lists"): the validity rule of wa_suppress_check and the one
step the lists add to a pick -- the listed ids read as -inf before anything
else.  Everything after that step is the existing references' (ts_rules.py,
sample_rules.py, beam_ref.py, beam_ts_ref.py, the drivers around
whisper_oracle), applied to the pre-masked row.  A helper module, not a test.
"""
from __future__ import annotations

import numpy as np

EOT = 50257
MIN_TEXT = 16  # ids of [0, EOT) the two lists must leave
NEG = -np.inf
# SOT, TRANSLATE, TRANSCRIBE, <|startoflm|>, <|startofprev|>, <|nospeech|> (Large-V3 / TINY_TEST)
SPECIALS = [50258, 50359, 50360, 50361, 50362, 50363]


def valid(always, first, ts0) -> bool:
    """wa_suppress_check on the host: `always` in [0, EOT) or (EOT, ts0), `first`
    in [0, ts0), duplicates allowed, at least MIN_TEXT text ids outside the union."""
    always, first = [int(i) for i in always], [int(i) for i in first]
    if ts0 <= EOT:
        return False
    if any(i < 0 or i >= ts0 or i == EOT for i in always):
        return False
    if any(i < 0 or i >= ts0 for i in first):
        return False
    text = {i for i in always + first if i < EOT}
    return EOT - len(text) >= MIN_TEXT


def union(always, first):
    """The ids of pick 0: both lists."""
    return list(always) + list(first)


def premask(z, ids):
    """z ([..., V]) with the listed ids at -inf: a copy, in z's float type."""
    z = np.array(z, copy=True)
    if len(ids):
        z[..., np.asarray(ids, np.int64)] = NEG
    return z
