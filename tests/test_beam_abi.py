"""The host-only beam entries of the C ABI (no GPU): wa_beam_check's argument
checks and wa_beam_rank against beam_ref.rank."""
from __future__ import annotations

import numpy as np
import pytest

import beam_ref
import whisper_amd
import wq4

EINVAL = 1


def test_symbols_are_exported():
    L = whisper_amd.lib()
    for name in ("wa_transcribe_beam", "wa_beam_check", "wa_beam_rank", "wa_beam_topk_check", "wa_beam_select_check",
                 "wa_self_attention_check"):
        assert hasattr(L, name), name


def test_beam_check_edges():
    ok = whisper_amd.beam_check
    # OK at the edges
    assert ok(1, 1, 1, 1) == 0
    assert ok(8, 8, 4, 32) == 0
    assert ok(8, 16, 4, 32) == 0
    assert ok(5, 5, 6, 30) == 0
    assert ok(1, 16, 32, 32) == 0
    # beam_size outside [1, 8]
    assert ok(0, 1, 1, 32) == EINVAL and ok(9, 9, 1, 32) == EINVAL and ok(-1, 1, 1, 32) == EINVAL
    # max_candidates outside [beam_size, 16]
    assert ok(5, 4, 1, 32) == EINVAL and ok(5, 17, 1, 32) == EINVAL and ok(1, 0, 1, 32) == EINVAL
    # rows past max_batch, no clips
    assert ok(5, 5, 7, 34) == EINVAL and ok(8, 8, 5, 32) == EINVAL and ok(1, 1, 2, 1) == EINVAL
    assert ok(1, 1, 0, 32) == EINVAL
    # null
    assert ok(1, 1, 1, 1, null=True) == EINVAL
    assert "null" in whisper_amd.lib().wa_last_error().decode()


def test_transcribe_beam_rejects_null_pointers():
    import ctypes

    L = whisper_amd.lib()
    b = whisper_amd.Beam(1, 1, float("nan"))
    assert L.wa_transcribe_beam(None, None, 1, 50259, 4, 1, ctypes.byref(b), None, None, None, None, None) == EINVAL
    assert L.wa_beam_rank(None, None, 1, float("nan"), None) == EINVAL


@pytest.mark.parametrize("penalty", [None, 0.0, 0.6, 1.0, 2.5])
def test_rank_matches_reference(penalty):
    rng = np.random.default_rng(5)
    for n in (1, 2, 5, 16):
        for _ in range(40):
            sums = -rng.uniform(0.1, 30.0, n).astype(np.float32)
            lens = rng.integers(0, 40, n).astype(np.int32)
            assert whisper_amd.beam_rank(sums, lens, penalty) == beam_ref.rank(sums, lens, penalty)
    # equal scores: the first in list order; an empty sequence counts as one token
    assert whisper_amd.beam_rank([-4.0, -2.0, -2.0], [4, 2, 2], None) == 0
    assert whisper_amd.beam_rank([-2.0, -1.0, -1.0], [0, 1, 0], None) == 1
    assert whisper_amd.beam_rank([-4.0, -2.0], [4, 1], 1.0) == beam_ref.rank([-4.0, -2.0], [4, 1], 1.0) == 1
    with pytest.raises(wq4.WQ4Error):
        whisper_amd.beam_rank(np.zeros(0, np.float32), np.zeros(0, np.int32))
