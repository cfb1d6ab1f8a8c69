"""Caller prompts (wa_transcribe_prompted, wa_transcribe_long_prompted): what
can be checked without a GPU -- the exported surface, the long-form prompt
rule against its restatement (prompt_ref.py), the argument checks, and the
oracle fixture of the GPU tests (float32 and float64 emit the same tokens)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import prompt_ref as R
import whisper_amd

EINVAL = 1
i32p = ctypes.POINTER(ctypes.c_int32)

NEW = ("wa_transcribe_prompted", "wa_transcribe_fallback_prompted", "wa_transcribe_long_prompted",
       "wa_long_result_prompt_len", "wa_long_prompt_window", "wa_long_prompt_next", "wa_prompt_check",
       "wa_prompt_logits_ragged", "wa_self_attention_prefill_check", "wa_cross_attention_prefill_check",
       "wa_self_attention_check", "wa_embed_check")


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    assert hasattr(whisper_amd.lib(), name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def test_python_surface():
    for n in ("transcribe_prompted", "fallback_prompted", "prompt_logits_ragged", "transcribe_long"):
        assert callable(getattr(whisper_amd.WhisperModel, n))
    for n in ("self_attention_prefill_check", "cross_attention_prefill_check", "self_attention_pad_check",
              "embed_pad_check", "long_prompt_window", "long_prompt_next"):
        assert callable(getattr(whisper_amd, n))


def test_graph_key_is_untouched():
    """Prompted graphs are kept apart by a field beside the key: the key's value stays."""
    assert whisper_amd.decode_graph_key_check(7, 2, 511, 511, 1, 1, 1, 3, 15, 64) == \
        ((((((((7 * 3 + 2) * 512 + 511) * 512 + 511) * 2 + 1) * 2 + 1) * 2 + 1) * 4 + 3) * 16 + 15) * 65 + 64


# ------------------------------------------------------ the long-form rule --
def ts(seconds):
    return R.TS0 + int(round(seconds / 0.02))


# hand-written windows: (tokens, skipped, temperature of the kept rung)
W_TWO_SEGMENTS = [ts(0.0), 11, 12, ts(2.0), ts(2.0), 13, ts(4.5), ts(4.5)]
W_OPEN_END = [ts(0.0), 21, 22, 23, ts(7.0)]
W_NO_TIMESTAMPS = [31, 32, 33]
W_LONG = [ts(0.0)] + list(range(1000, 1180)) + [ts(20.0), ts(20.0)]
STREAMS = {
    "empty_initial": ([], [(W_TWO_SEGMENTS, False, 0.0), (W_OPEN_END, False, 0.0), (W_NO_TIMESTAMPS, False, 0.2)]),
    "long_initial": (list(range(2000, 2300)), [(W_TWO_SEGMENTS, False, 0.0), (W_LONG, False, 0.4), (W_OPEN_END, False, 0.0)]),
    "hot_rung_resets": ([5, 6, 7], [(W_TWO_SEGMENTS, False, 0.0), (W_OPEN_END, False, 0.6), (W_NO_TIMESTAMPS, False, 0.0),
                                    (W_TWO_SEGMENTS, False, 0.5)]),
    "skipped_window": ([5, 6, 7], [(W_TWO_SEGMENTS, False, 0.0), (W_LONG, True, 0.8), (W_OPEN_END, False, 0.0)]),
}


def emitted(tokens):
    """Tokens of a window that its segments hold (what follows the last closed pair is not emitted)."""
    return sum(b - a for a, b in R.segments(tokens))


@pytest.mark.parametrize("condition", [True, False])
@pytest.mark.parametrize("max_tokens", [224, 100, 12])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_long_prompt_rule_matches_restatement(name, max_tokens, condition):
    initial, windows = STREAMS[name]
    prev, reset = list(initial), 0
    lib_prev, lib_reset = list(initial), 0
    ks = []
    for tokens, skipped, temp in windows + [([], False, 0.0)]:  # (one more prompt after the last window)
        want, k = R.long_prompt_window(prev, reset, 448, max_tokens)
        got, gk = whisper_amd.long_prompt_window(lib_prev, lib_reset, 448, max_tokens, R.STARTOFPREV, R.LANG, R.TRANSCRIBE)
        assert (got, gk) == (want, k)
        assert len(got) + max_tokens <= 448 and k <= 223
        assert got[-3:] == [R.SOT, R.LANG, R.TRANSCRIBE] and (k == 0) == (len(got) == 3)
        ks.append(k)
        prev, reset = R.long_prompt_next(prev, reset, tokens, skipped, temp, condition)
        lib_prev, lib_reset = whisper_amd.long_prompt_next(lib_prev, lib_reset, tokens, R.TS0, skipped, temp, condition)
        assert (lib_prev, lib_reset) == (prev, reset)
    cap = min(223, 448 - 4 - max_tokens)
    if name == "empty_initial":
        assert ks[0] == 0 and (ks[1] == min(emitted(W_TWO_SEGMENTS), cap) if condition else ks[1] == 0)
    if name == "long_initial":
        assert ks[0] == cap  # 300 initial ids: the bound, not the length
    if name == "hot_rung_resets" and condition:
        assert ks[2] == 0 and ks[3] == min(emitted(W_NO_TIMESTAMPS), cap)  # the rung at 0.6 cut the history; 0.5 does not
        assert ks[4] == min(emitted(W_NO_TIMESTAMPS) + emitted(W_TWO_SEGMENTS), cap)
    if name == "skipped_window":
        assert ks[2] == ks[1]  # the skipped window added nothing
    if not condition:
        assert all(k == 0 for k in ks[1:])  # only the initial prompt ever conditions, and only window 0


def test_segments_restated_as_the_library_slices():
    for toks in (W_TWO_SEGMENTS, W_OPEN_END, W_NO_TIMESTAMPS, W_LONG, [ts(0.0), ts(0.0)], []):
        segs, _ = whisper_amd.segments_from_tokens(toks, R.TS0)
        assert [list(s[2]) for s in segs] == [toks[a:b] for a, b in R.segments(toks)]


# ------------------------------------------------------- argument checks --
def prompt_struct(tokens, n, ld):
    t = np.ascontiguousarray(tokens, np.int32)
    nn = np.ascontiguousarray(n, np.int32)
    return whisper_amd.Prompt(t.ctypes.data_as(i32p), nn.ctypes.data_as(i32p), ld), (t, nn)


@pytest.mark.parametrize("bad", ["n0", "n_over_ld", "id_neg", "id_vocab", "too_long", "null_tokens", "ld0"])
def test_prompt_check_rejects(bad):
    L = whisper_amd.lib()
    V, ctx, ld = 51866, 448, 300
    tok = np.full((2, ld), 7, np.int32)
    n = np.array([4, 250], np.int32)
    max_tokens = 100
    p, keep = prompt_struct(tok, n, ld)
    assert L.wa_prompt_check(ctypes.byref(p), 2, V, ctx, max_tokens) == 0
    assert L.wa_prompt_check(ctypes.byref(p), 2, V, ctx, 198) == 0  # 250 + 198 == 448
    if bad == "n0":
        n[1] = 0
    elif bad == "n_over_ld":
        n[1] = ld + 1
    elif bad == "id_neg":
        tok[1, 249] = -1
    elif bad == "id_vocab":
        tok[0, 3] = V
    elif bad == "too_long":
        max_tokens = 199
    elif bad == "null_tokens":
        p.tokens = None
    else:
        p.ld = 0
    assert L.wa_prompt_check(ctypes.byref(p), 2, V, ctx, max_tokens) == EINVAL
    assert L.wa_last_error()
    tok[0, 5] = V  # past the clip's n_tokens: not read
    del keep


def test_entries_reject_before_any_device_work():
    """Null pointers are WQ4_EINVAL at once; a negative long-form language is
    refused for a model that is not a model (nothing may touch it)."""
    L = whisper_amd.lib()
    model, audio = (ctypes.c_uint8 * 65536)(), (ctypes.c_float * 16)()
    addr = lambda b: ctypes.c_void_p(ctypes.addressof(b))
    out, nout = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 2)()
    p, keep = prompt_struct(np.full((1, 4), 7, np.int32), [4], 4)
    assert L.wa_transcribe_prompted(None, addr(audio), 1, ctypes.byref(p), 4, 1, None, out, nout, None, None) == EINVAL
    assert L.wa_transcribe_prompted(addr(model), addr(audio), 1, None, 4, 1, None, out, nout, None, None) == EINVAL
    assert L.wa_transcribe_fallback_prompted(addr(model), addr(audio), 1, ctypes.byref(p), 4, 1, None, out, nout, None,
                                             None, None) == EINVAL
    assert L.wa_prompt_logits_ragged(None, ctypes.byref(p), 1, addr(audio), None) == EINVAL
    temps, seed = (ctypes.c_float * 2)(0.0, 0.4), (ctypes.c_uint64 * 2)(1, 2)
    off, n = (ctypes.c_int64 * 2)(0, 8), (ctypes.c_int64 * 2)(8, 8)
    for cond in (0, 1):
        opt = whisper_amd.LongOptions(12, 5, -1, 50, ctypes.cast(temps, ctypes.POINTER(ctypes.c_float)), 2, -1.0, 0.6,
                                      ctypes.cast(seed, ctypes.POINTER(ctypes.c_uint64)))
        lp = whisper_amd.LongPrompt(None, None, 0, cond, 0.5)
        h = ctypes.c_void_p(0xDEAD)
        assert L.wa_transcribe_long_prompted(addr(model), addr(audio), 2, off, n, ctypes.byref(opt), ctypes.byref(lp),
                                             ctypes.byref(h), None) == EINVAL
        assert "lang_token" in L.wa_last_error().decode() and h.value is None
    k = ctypes.c_int()
    assert L.wa_long_result_prompt_len(None, 0, 0, ctypes.byref(k)) == EINVAL
    del keep


# ------------------------------------------------------ the oracle fixture --
def test_fixture_has_no_near_ties():
    """The GPU tests compare tokens with the float32 oracle composed from
    decoder_pass: the float64 oracle must emit the same tokens under every
    prompt, or a GPU mismatch could be a tie broken the other way."""
    a, b = R.reference("float32"), R.reference("float64")
    for x, y in zip(a["batch"] + [a["long"]], b["batch"] + [b["long"]]):
        assert x["tokens"] == y["tokens"] and len(x["tokens"]) > 0
        assert R.wo.SynthWhisper.argmax_last(x["first"]) == R.wo.SynthWhisper.argmax_last(y["first"])
    batch, long = R.prompts()
    assert [len(p) for p in batch] == list(R.LENGTHS) and len(long) == R.LONG


def test_composition_equals_the_oracle_transcribe_on_the_default_prompt():
    """The composed reference under [SOT, lang, TRANSCRIBE, NO_TIMESTAMPS] is the oracle's own transcribe."""
    om = R.wo.SynthWhisper("tiny_test", R.SEED)
    mel = R.mels(1)
    want = om.transcribe(mel, R.LANG, max_tokens=R.STEPS)
    assert R.reference("float32")["batch"][0]["tokens"] == want[0]
