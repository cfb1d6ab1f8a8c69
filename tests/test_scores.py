"""Scored transcribes (wa_transcribe_scored and its check entries): what can be
tested without a GPU -- the exports and the argument checks, which precede
every device call.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import whisper_amd

EINVAL = 1

NEW = ("wa_transcribe_scored", "wa_transcribe_batches_scored", "wa_logits_pick_check", "wa_row_logprob_check")


def test_wq4_einval_value():
    import re

    import wq4

    text = open(wq4.HEADER_PATH).read()
    assert int(re.search(r"WQ4_EINVAL\s*=\s*(\d+)", text).group(1)) == EINVAL


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    L = whisper_amd.lib()
    assert hasattr(L, name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def _bufs(n=4096):
    """Non-null host buffers: the entries under test return before reading them."""
    model = (ctypes.c_uint8 * n)()
    mel = (ctypes.c_float * 16)()
    tok = (ctypes.c_int32 * 1024)()
    nt = (ctypes.c_int32 * 16)()
    return model, mel, tok, nt


def _scores():
    lp = np.zeros(1024, np.float32)
    sc = whisper_amd.Scores(lp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None, None, None)
    return sc, lp


def test_transcribe_scored_rejects_bad_arguments():
    L = whisper_amd.lib()
    model, mel, tok, nt = _bufs()
    sc, _keep = _scores()
    vp = ctypes.c_void_p
    addr = lambda b: vp(ctypes.addressof(b))
    # null model
    assert L.wa_transcribe_scored(None, addr(mel), 1, 50259, 8, 1, tok, nt, ctypes.byref(sc), None) == EINVAL
    assert "null" in L.wa_last_error().decode()
    # null scores (checked before the model is read)
    assert L.wa_transcribe_scored(addr(model), addr(mel), 1, 50259, 8, 1, tok, nt, None, None) == EINVAL
    assert "null" in L.wa_last_error().decode()
    # max_tokens > 224
    assert L.wa_transcribe_scored(addr(model), addr(mel), 1, 50259, 225, 1, tok, nt, ctypes.byref(sc), None) == EINVAL
    assert "max_tokens" in L.wa_last_error().decode()


def test_transcribe_batches_scored_rejects_bad_arguments():
    L = whisper_amd.lib()
    model, mel, tok, nt = _bufs()
    sc, _keep = _scores()
    vp = ctypes.c_void_p
    addr = lambda b: vp(ctypes.addressof(b))
    f = L.wa_transcribe_batches_scored
    assert f(None, addr(mel), 2, 1, 50259, 8, 1, tok, nt, ctypes.byref(sc), None) == EINVAL
    assert f(addr(model), addr(mel), 2, 1, 50259, 8, 1, tok, nt, None, None) == EINVAL
    assert "null" in L.wa_last_error().decode()
    assert f(addr(model), addr(mel), 2, 1, 50259, 225, 1, tok, nt, ctypes.byref(sc), None) == EINVAL
    assert "max_tokens" in L.wa_last_error().decode()


def test_plain_entries_check_in_the_same_order():
    """wa_transcribe and wa_transcribe_batches check like the scored entries:
    null pointers, n_batches, max_tokens, and the clip count -- the only read of
    the model, which here is a block of zero bytes -- last of all."""
    L = whisper_amd.lib()
    model, mel, tok, nt = _bufs()
    vp = ctypes.c_void_p
    addr = lambda b: vp(ctypes.addressof(b))
    err = lambda: L.wa_last_error().decode()
    f, g = L.wa_transcribe, L.wa_transcribe_batches
    assert f(None, addr(mel), 1, 50259, 8, 1, tok, nt, None) == EINVAL and "null" in err()
    assert f(addr(model), None, 1, 50259, 8, 1, tok, nt, None) == EINVAL and "null" in err()
    assert g(None, addr(mel), 2, 1, 50259, 8, 1, tok, nt, None) == EINVAL and "null" in err()
    assert g(addr(model), addr(mel), 0, 1, 50259, 8, 1, tok, nt, None) == EINVAL and "n_batches" in err()
    for mt in (0, 225):
        # n_clips = 1 is out of the zero model's range too: max_tokens is reported
        assert f(addr(model), addr(mel), 1, 50259, mt, 1, tok, nt, None) == EINVAL and "max_tokens" in err()
        assert g(addr(model), addr(mel), 2, 1, 50259, mt, 1, tok, nt, None) == EINVAL and "max_tokens" in err()
        assert g(addr(model), addr(mel), 0, 1, 50259, mt, 1, tok, nt, None) == EINVAL and "n_batches" in err()
    assert f(addr(model), addr(mel), 1, 50259, 8, 1, tok, nt, None) == EINVAL and "n_clips" in err()
    assert g(addr(model), addr(mel), 2, 1, 50259, 8, 1, tok, nt, None) == EINVAL and "n_clips" in err()


def test_logits_logprob_check_rejects_bad_arguments():
    L = whisper_amd.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = lambda hid, emb, n, D, V, tok, lp: L.wa_logits_pick_check(0, hid, emb, n, D, V, 0, 0, None, 0, None, None, 0,
                                                                  None, tok, lp, None, None)
    ok = dict(hid=p, emb=p, tok=p)  # (a null logprob is the greedy form: rejected below with the other modes)
    for null in ("hid", "emb", "tok"):
        a = dict(ok, **{null: None})
        assert f(a["hid"], a["emb"], 1, 128, 26, a["tok"], p) == EINVAL, null
    rec = (ctypes.c_int32 * 8)()
    assert L.wa_logits_pick_check(0, p, p, 1, 128, 26, 0, 0, None, 0, None, None, 20, rec, p, None, None,
                                  None) == EINVAL  # a timestamp pick needs logprob_dev
    for n in (0, -1, 33):
        assert f(p, p, n, 128, 26, p, p) == EINVAL, n
    assert f(p, p, 1, 100, 26, p, p) == EINVAL  # D not a multiple of 128


def test_row_logprob_check_rejects_bad_arguments():
    L = whisper_amd.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    f = L.wa_row_logprob_check
    assert f(0, None, 1, 26, 0, 26, 0, None, 3, p) == EINVAL
    assert f(0, p, 1, 26, 0, 26, 0, None, 3, None) == EINVAL
    for n in (0, 33):
        assert f(0, p, n, 26, 0, 26, 0, None, 3, p) == EINVAL, n
    for lo, hi in ((5, 5), (6, 5), (-1, 4), (0, 27)):
        assert f(0, p, 1, 26, lo, hi, 0, None, 3, p) == EINVAL, (lo, hi)
