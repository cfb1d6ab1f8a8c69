"""whisper_amd -- Python binding of the Whisper model runtime (include/whisper_amd.h).

Mirrors WhisperModel::{new, encode, transcribe} (zerr0o/whisper-burn
src/model/whisper.rs) over lib/libwhisper_amd.so; every Q4 projection runs in
lib/libwq4.so.  Loud failure if the native libraries are missing.  The ctypes
declarations are _ffi.py's, the kernel check wrappers of the parity tests
checks.py's; both are re-exported here.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

import wq4

from ._ffi import (CHECKS_HEADER_PATH, HEADER_PATH, LIB_PATH, Beam, BeamOptions, BeamResult, Fallback,  # noqa: F401
                   LongOptions, LongPrompt, LongSegment, LongWindow, Prompt, Sampling, Scores, Segment, _as, _dev,
                   _i32, _i64, _ptr, _torch, check, lib)
from .checks import *  # noqa: F401,F403  -- the check wrappers and probes
from .checks import _id_list, _sampling_arrays

VARIANTS = {"large_v3": 0, "medium": 1, "tiny_test": 2}
CFG_KEYS = ["n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "n_text_ctx",
            "n_text_state", "n_text_head", "n_text_layer", "n_vocab", "n_lang"]
RULE_FIELDS = ("text_ok", "ts_lo", "ts_hi", "first", "last", "penult", "t_last", "pad")  # a rule record's 8 int32


def decode_group_rows(n_clips: int) -> int:
    """Clips in the largest decode group of a transcribe batch of n_clips:
    the row count of every captured decode-step launch (wa_decode_group_rows)."""
    return int(lib().wa_decode_group_rows(n_clips))


def synth_uniform(seed: int, name: str, n: int, lo: float, hi: float) -> np.ndarray:
    out = np.empty(n, np.float32)
    check(lib().wa_synth_uniform(seed, name.encode(), n, lo, hi, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
    return out


MEL_FRAMES = 3000
MEL_CHUNK = 480000


def mel_filterbank(n_mels: int = 128) -> tuple[np.ndarray, np.ndarray]:
    """(filters [n_mels, 201], periodic Hann window [400]) as the product builds
    them (src/audio/mel.rs:272-320); host-only."""
    fb = np.empty((n_mels, 201), np.float32)
    win = np.empty(400, np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    check(lib().wa_mel_filterbank(n_mels, fb.ctypes.data_as(f32p), win.ctypes.data_as(f32p)))
    return fb, win


def log_mel(audio, n_mels: int = 128, n_samples: Optional[int] = None, out=None):
    """MelSpectrogram::compute_log (src/audio/mel.rs:126-157) with the pad /
    truncate / transpose of transcribe.rs:44-76, for a batch of clips on the
    GPU.  audio: cuda f32 [B, L] (16 kHz mono; the first n_samples of each row
    are used, default L) -> cuda f32 [B, n_mels, 3000], the transcribe input."""
    torch = _torch()
    assert audio.dtype == torch.float32 and audio.is_cuda and audio.dim() == 2
    if audio.stride(1) != 1:
        audio = audio.contiguous()
    B, L = audio.shape
    n = L if n_samples is None else int(n_samples)
    if out is None:
        out = torch.empty((B, n_mels, MEL_FRAMES), device=audio.device, dtype=torch.float32)
    dev = audio.device.index if audio.device.index is not None else torch.cuda.current_device()
    check(lib().wa_log_mel(dev, ctypes.c_void_p(audio.data_ptr()), B, n, audio.stride(0), n_mels,
                           ctypes.c_void_p(out.data_ptr()),
                           ctypes.c_void_p(torch.cuda.current_stream(audio.device).cuda_stream)))
    return out


def long_mel_max(audio, offset, n_samples, n_mels: int = 128, out=None):
    """The recording maxima of long-form windows (wa_long_mel_max): audio a cuda
    f32 buffer holding every recording, recording r its n_samples[r] samples
    from element offset[r] -> cuda f32 [len(offset)], max(-10, the largest raw
    log-mel value of the recording)."""
    torch = _torch()
    assert audio.dtype == torch.float32 and audio.is_cuda and audio.is_contiguous()
    off, n = _i64(offset), _i64(n_samples)
    assert off.size == n.size and (off.size == 0 or int((off + n).max()) <= audio.numel())
    if out is None:
        out = torch.empty(off.size, device=audio.device, dtype=torch.float32)
    check(lib().wa_long_mel_max(_dev(audio), _ptr(audio), int(off.size), _as(off, ctypes.c_int64),
                                _as(n, ctypes.c_int64), n_mels, _ptr(out),
                                ctypes.c_void_p(torch.cuda.current_stream(audio.device).cuda_stream)))
    return out


def long_mel_windows(audio, offset, n_samples, seek, max_index, max_dev, n_mels: int = 128, out=None):
    """Windows of long recordings (wa_long_mel_windows): clip c is the 3000
    frames from mel frame seek[c] of the recording (offset[c], n_samples[c])
    in the cuda f32 buffer `audio`, normalised against max_dev[max_index[c]]
    (long_mel_max), exact zeros past the recording's n_samples // 160 content
    frames -> cuda f32 [len(seek), n_mels, 3000], the transcribe input."""
    torch = _torch()
    assert audio.dtype == torch.float32 and audio.is_cuda and audio.is_contiguous()
    assert max_dev.dtype == torch.float32 and max_dev.is_cuda and max_dev.is_contiguous()
    off, n, sk, mi = _i64(offset), _i64(n_samples), _i32(seek), _i32(max_index)
    B = int(sk.size)
    assert off.size == B and n.size == B and mi.size == B
    assert B == 0 or (int((off + n).max()) <= audio.numel() and int(mi.max()) < max_dev.numel())
    if out is None:
        out = torch.empty((B, n_mels, MEL_FRAMES), device=audio.device, dtype=torch.float32)
    check(lib().wa_long_mel_windows(_dev(audio), _ptr(audio), B, _as(off, ctypes.c_int64), _as(n, ctypes.c_int64),
                                    _as(sk, ctypes.c_int32), _as(mi, ctypes.c_int32), _ptr(max_dev), n_mels,
                                    _ptr(out), ctypes.c_void_p(torch.cuda.current_stream(audio.device).cuda_stream)))
    return out


def long_advance(tokens, ts0: int, size: int, no_speech_prob: float, avg_logprob: float,
                 logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6):
    """The skip and advance rules of one long-form window (wa_long_advance; host
    only) -> (skipped, advance in mel frames).  None switches a threshold off."""
    toks = _i32(tokens)
    nan = float("nan")
    sk, adv = ctypes.c_int(), ctypes.c_int()
    check(lib().wa_long_advance(_as(toks, ctypes.c_int32), int(toks.size), int(ts0), int(size), float(no_speech_prob),
                                float(avg_logprob), nan if logprob_threshold is None else float(logprob_threshold),
                                nan if no_speech_threshold is None else float(no_speech_threshold),
                                ctypes.byref(sk), ctypes.byref(adv)))
    return bool(sk.value), int(adv.value)


def long_round(content_frames, seek, windows, max_batch: int, max_windows: int) -> list[int]:
    """The recordings of the next long-form round (wa_long_round; host only):
    in index order those with seek < content_frames and windows < max_windows,
    up to max_batch of them."""
    c, s, w = _i32(content_frames), _i32(seek), _i32(windows)
    assert c.size == s.size == w.size
    out, n = (ctypes.c_int * max(1, int(max_batch)))(), ctypes.c_int()
    check(lib().wa_long_round(_as(c, ctypes.c_int32), _as(s, ctypes.c_int32), _as(w, ctypes.c_int32), int(c.size),
                              int(max_batch), int(max_windows), out, ctypes.byref(n)))
    return [int(out[i]) for i in range(n.value)]


def beam_check(beam_size: int, max_candidates: int, n_clips: int, max_batch: int, null: bool = False) -> int:
    """wa_beam_check's status (0 = OK) for these arguments; null: a null wa_beam."""
    b = Beam(int(beam_size), int(max_candidates), float("nan"))
    return int(lib().wa_beam_check(None if null else ctypes.byref(b), n_clips, max_batch))


def beam_rank(sum_logprob, n_tokens, length_penalty: Optional[float] = None) -> int:
    """The rank of wa_transcribe_beam over one clip's candidates (wa_beam_rank)."""
    s = np.ascontiguousarray(sum_logprob, np.float32)
    n = np.ascontiguousarray(n_tokens, np.int32)
    assert s.ndim == 1 and s.shape == n.shape
    best = ctypes.c_int32(-1)
    check(lib().wa_beam_rank(s.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                             n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(s.size),
                             float("nan") if length_penalty is None else float(length_penalty), ctypes.byref(best)))
    return int(best.value)


def _prompt_arrays(prompts, n: Optional[int] = None, min_len: int = 1):
    """A list of id sequences -> (tokens [n, ld] int32, n_tokens [n] int32, ld); lengths below min_len keep ld >= 1."""
    prompts = [np.asarray(p, np.int64).reshape(-1) for p in prompts]
    assert n is None or len(prompts) == n
    ld = max([1] + [p.size for p in prompts])
    tok = np.zeros((len(prompts), ld), np.int32)
    for i, p in enumerate(prompts):
        tok[i, :p.size] = np.clip(p, -(1 << 31), (1 << 31) - 1)
    return tok, np.asarray([p.size for p in prompts], np.int32), ld


def align_words(jump, word_lens):
    """Token jump frames -> word times (wa_align_words, host only): jump the N
    frames of a clip (the last row is EOT), word_lens the words' token counts,
    summing to N - 1 -> (start_s, end_s) f32 [len(word_lens)]."""
    jump, wl = _i32(jump), _i32(word_lens)
    start, end = np.zeros(wl.size, np.float32), np.zeros(wl.size, np.float32)
    check(lib().wa_align_words(_as(jump, ctypes.c_int32), jump.size, _as(wl, ctypes.c_int32), wl.size,
                               _as(start, ctypes.c_float), _as(end, ctypes.c_float)))
    return start, end


def long_prompt_window(prev, reset: int, n_text_ctx: int, max_tokens: int, startofprev: int, lang_token: int,
                       task_token: int) -> tuple[list[int], int]:
    """A window's prompt and its previous-text length k (wa_long_prompt_window, host only)."""
    prev = _i32(prev)
    out = np.zeros(n_text_ctx + 4, np.int32)
    n, k = ctypes.c_int(), ctypes.c_int()
    check(lib().wa_long_prompt_window(_as(prev, ctypes.c_int32), int(prev.size), int(reset), n_text_ctx, max_tokens,
                                      startofprev, lang_token, task_token, _as(out, ctypes.c_int32), int(out.size),
                                      ctypes.byref(n), ctypes.byref(k)))
    return out[:n.value].tolist(), k.value


def long_prompt_next(prev, reset: int, tokens, ts0: int, skipped: bool, temperature: float,
                     condition_on_previous_text: bool, reset_temperature: float = 0.5) -> tuple[list[int], int]:
    """What a decoded window adds to a recording's previous text (wa_long_prompt_next, host only)."""
    prev, tokens = _i32(prev), _i32(tokens)
    buf = np.zeros(prev.size + tokens.size + 1, np.int32)
    buf[:prev.size] = prev
    n, r = ctypes.c_int(int(prev.size)), ctypes.c_int(int(reset))
    check(lib().wa_long_prompt_next(_as(buf, ctypes.c_int32), ctypes.byref(n), ctypes.byref(r),
                                    _as(tokens, ctypes.c_int32), int(tokens.size), ts0, 1 if skipped else 0,
                                    float(temperature), 1 if condition_on_previous_text else 0,
                                    float(reset_temperature)))
    return buf[:n.value].tolist(), r.value


def segments_from_tokens(tokens, ts0: int = 50365, cap: Optional[int] = None):
    """The segments of one 30-s window's tokens (wa_segments_from_tokens; host
    only): ([(start_s, end_s, tokens of the segment)], seek_frames).  ts0 is
    <|0.00|>: 50365 for Large-V3 / TINY_TEST, 50364 for Medium.  cap: room
    for that many segments (default: enough); too small raises WQ4Error."""
    toks = np.ascontiguousarray(tokens, np.int32).reshape(-1)
    n = int(toks.size)
    room = max(1, n) if cap is None else int(cap)
    segs = (Segment * max(1, room))()
    ns, seek = ctypes.c_int(), ctypes.c_int()
    check(lib().wa_segments_from_tokens(toks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, int(ts0), segs, room,
                                        ctypes.byref(ns), ctypes.byref(seek)))
    out = [(float(segs[i].start_s), float(segs[i].end_s), toks[segs[i].tok_begin:segs[i].tok_end].tolist())
           for i in range(ns.value)]
    return out, int(seek.value)


def sample_noise(seed: int, pick: int, id0: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The sampling noise of ids id0 .. id0 + n - 1 at (seed, pick) as the
    kernels define it (wa_sample_noise; host only): (u, g) float32 [n]."""
    u, g = np.empty(n, np.float32), np.empty(n, np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    check(lib().wa_sample_noise(int(seed) & (2 ** 64 - 1), int(pick), int(id0), int(n), u.ctypes.data_as(f32p),
                                g.ctypes.data_as(f32p)))
    return u, g


def suppress_check(always=(), first=(), ts0: int = 50365) -> bool:
    """Whether the two suppress-token lists are valid for a model whose
    <|0.00|> is ts0 (wa_suppress_check; host only): `always` ids in [0, EOT) or
    (EOT, ts0), `first` ids in [0, ts0), at least 16 text ids left."""
    _a, ap, na = _id_list(always)
    _f, fp, nf = _id_list(first)
    return lib().wa_suppress_check(ap, na, fp, nf, int(ts0)) == 0


def _scored_clip(toks, n, lp, ns, lt, lpr) -> dict:
    """One clip of a scored transcribe: lp its max_tokens + 1 log-probability slots."""
    n = int(n)
    k = n + 1 if n < len(lp) and not np.isnan(lp[n]) else n  # the EOT pick's slot, when the clip stopped on EOT
    seen = lp[~np.isnan(lp)]
    return {"tokens": toks[:n].tolist(), "token_logprob": lp[:k].copy(),
            "avg_logprob": float(seen.astype(np.float64).mean()) if seen.size else float("nan"),
            "no_speech_prob": float(ns), "lang_token": int(lt), "lang_prob": float(lpr), "logprob_slots": lp.copy()}


class GgufReader:
    """GgufReader (src/gguf/reader.rs): header, tensor index, tensor bytes."""

    def __init__(self, path: str):
        h = ctypes.c_void_p(None)
        check(lib().wa_gguf_open(path.encode(), ctypes.byref(h)))
        self._h = h

    @property
    def version(self) -> int:
        return lib().wa_gguf_version(self._h)

    def tensors(self) -> list[dict]:
        """File-order tensor index: name, dims (GGUF order), type, offset, nbytes."""
        out = []
        for i in range(lib().wa_gguf_tensor_count(self._h)):
            name = ctypes.create_string_buffer(512)
            nd, ty = ctypes.c_int(), ctypes.c_int()
            dims = (ctypes.c_uint64 * 8)()
            off, nb = ctypes.c_uint64(), ctypes.c_uint64()
            check(lib().wa_gguf_tensor_info(self._h, i, name, 512, ctypes.byref(nd), dims, ctypes.byref(ty),
                                            ctypes.byref(off), ctypes.byref(nb)))
            out.append({"name": name.value.decode(), "dims": list(dims[: nd.value]), "type": ty.value,
                        "offset": off.value, "nbytes": nb.value})
        return out

    def tensor_data(self, name: str) -> np.ndarray:
        info = next(t for t in self.tensors() if t["name"] == name)
        buf = np.empty(info["nbytes"], np.uint8)
        check(lib().wa_gguf_tensor_data(self._h, name.encode(), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         buf.size))
        return buf

    def close(self):
        if self._h and self._h.value:
            lib().wa_gguf_close(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WhisperModel:
    """A Whisper model resident on one MI355X: synthetic weights (default) or
    a GGUF checkpoint (WhisperModel.from_gguf, src/gguf/loader.rs)."""

    WEIGHTS = {"q4_0": 0, "f16": 1}

    def __init__(self, variant: str = "large_v3", seed: int = 1234, max_batch: int = 1, device: int = 0,
                 precision: int = wq4.PREC_F16X2, gguf_path: Optional[str] = None, weights: str = "q4_0"):
        h = ctypes.c_void_p(None)
        if gguf_path is None:
            check(lib().wa_model_create_synthetic_ex(device, VARIANTS[variant], seed, max_batch, precision,
                                                     self.WEIGHTS[weights], ctypes.byref(h)))
        else:
            check(lib().wa_model_create_from_gguf(device, gguf_path.encode(), VARIANTS[variant], max_batch,
                                                  precision, ctypes.byref(h)))
        self._h = h
        self.device = device
        self.variant = variant
        self.max_batch = max_batch
        cfg = (ctypes.c_int32 * len(CFG_KEYS))()
        check(lib().wa_model_config(h, cfg))
        self.config = dict(zip(CFG_KEYS, list(cfg)))
        self.weights = {0: "q4_0", 1: "f16"}[lib().wa_model_weight_type(h)]

    @classmethod
    def from_gguf(cls, path: str, variant: str = "large_v3", max_batch: int = 1, device: int = 0,
                  precision: int = wq4.PREC_F16X2) -> "WhisperModel":
        """load_whisper_from_gguf (src/gguf/loader.rs:26-45)."""
        return cls(variant, 0, max_batch, device, precision, gguf_path=path)

    @property
    def wide_range(self) -> bool:
        """True once a transcribe overflowed the LayerNorm fold's operand range
        and the model switched to the LayerNorm path (wa_model_wide_range >= 1)."""
        return lib().wa_model_wide_range(self._h) >= 1

    @property
    def range_tier(self) -> int:
        """0 the product path, 1 the LayerNorm path, 2 the LayerNorm path with
        every FFN on per-call operand scales, 3 also every attention output in
        f32 with its output projection on per-call operand scales
        (wa_model_wide_range)."""
        return lib().wa_model_wide_range(self._h)

    def device_bytes(self) -> int:
        return int(lib().wa_model_device_bytes(self._h))

    def set_suppress_tokens(self, always=(), first=()) -> None:
        """OpenAI's SuppressTokens (`always`: masked at every pick) and
        SuppressBlank (`first`: masked in addition at a clip's first pick) id
        lists for every later transcribe of this model (wa_model_set_suppress);
        two empty lists clear them.  Invalid lists raise WQ4Error and set
        nothing.  Not to be called while a transcribe runs."""
        _a, ap, na = _id_list(always)
        _f, fp, nf = _id_list(first)
        check(lib().wa_model_set_suppress(self._h, ap, na, fp, nf))

    @property
    def suppress_tokens(self) -> tuple:
        """(always, first) as set: two tuples of ids (wa_model_suppress_ids)."""
        out = []
        for which in (0, 1):
            n = ctypes.c_int(0)
            lib().wa_model_suppress_ids(self._h, which, None, 0, ctypes.byref(n))  # the count
            buf = (ctypes.c_int32 * max(1, n.value))()
            check(lib().wa_model_suppress_ids(self._h, which, buf, n.value, ctypes.byref(n)))
            out.append(tuple(int(buf[i]) for i in range(n.value)))
        return tuple(out)

    def _stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def transcribe(self, mel, lang_token: Optional[int] = 50259, max_tokens: int = 224, eot_stop: bool = True):
        """whisper.rs:51-128 for a batch of clips; mel: cuda f32 [B, n_mels, 3000].
        Returns a list of token-id lists (special tokens excluded)."""
        torch = _torch()
        mel = mel.contiguous()
        assert mel.dtype == torch.float32 and mel.is_cuda
        B = mel.shape[0]
        toks = np.zeros((B, max_tokens), np.int32)
        nt = np.zeros(B, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        check(lib().wa_transcribe(self._h, ctypes.c_void_p(mel.data_ptr()), B,
                                  -1 if lang_token is None else int(lang_token), max_tokens, 1 if eot_stop else 0,
                                  toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), self._stream()))
        return [toks[b, : nt[b]].tolist() for b in range(B)]

    def transcribe_beam(self, mel, beam_size: int = 5, patience: float = 1.0, length_penalty: Optional[float] = None,
                        lang_token: Optional[int] = 50259, max_tokens: int = 224, eot_stop: bool = True,
                        return_candidates: bool = False, timestamps: bool = False, max_initial: int = 50,
                        prompts=None):
        """Beam search (wa_transcribe_beam; OpenAI's beam_size / patience /
        length_penalty): mel cuda f32 [B, n_mels, 3000] with B * beam_size <=
        max_batch.  Returns the best candidate's token list per clip, or with
        return_candidates a dict per clip: tokens, sum_logprob, best, candidates
        (list order: dicts of tokens and sum_logprob), no_speech_prob,
        lang_token, lang_prob.
        timestamps / max_initial: the prompt and rules of transcribe_timestamps
        (wa_transcribe_beam_ex); every returned clip and candidate then also
        carries segments and seek_frames (segments_from_tokens), so a dict per
        clip is returned in any case.  prompts: one id sequence per clip, as
        transcribe_prompted (lang_token is ignored; with timestamps the prompt
        leaves NO_TIMESTAMPS out)."""
        torch = _torch()
        mel = mel.contiguous()
        assert mel.dtype == torch.float32 and mel.is_cuda
        B, K = mel.shape[0], int(beam_size)
        C = int(round(K * patience))
        toks = np.zeros((B, max_tokens), np.int32)
        nt = np.zeros(B, np.int32)
        ct = np.zeros((B, max(C, 1), max_tokens), np.int32)
        cn, cs = np.zeros((B, max(C, 1)), np.int32), np.zeros((B, max(C, 1)), np.float32)
        nc, best = np.zeros(B, np.int32), np.zeros(B, np.int32)
        ns, lpr, lt = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32)
        i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        sc = Scores(None, ns.ctypes.data_as(f32p), lt.ctypes.data_as(i32p), lpr.ctypes.data_as(f32p))
        res = BeamResult(ct.ctypes.data_as(i32p), cn.ctypes.data_as(i32p), cs.ctypes.data_as(f32p),
                         nc.ctypes.data_as(i32p), best.ctypes.data_as(i32p))
        bm = Beam(K, C, float("nan") if length_penalty is None else float(length_penalty))
        if timestamps or prompts is not None:
            pr = None
            if prompts is not None:
                ptok, pn, pld = _prompt_arrays(prompts, B)
                pr = Prompt(ptok.ctypes.data_as(i32p), pn.ctypes.data_as(i32p), pld)
            opt = BeamOptions(1 if timestamps else 0, int(max_initial),
                              None if pr is None else ctypes.cast(ctypes.pointer(pr), ctypes.c_void_p))
            check(lib().wa_transcribe_beam_ex(self._h, _ptr(mel), B, -1 if lang_token is None else int(lang_token),
                                              max_tokens, 1 if eot_stop else 0, ctypes.byref(bm), ctypes.byref(opt),
                                              toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), ctypes.byref(sc),
                                              ctypes.byref(res), self._stream()))
        else:
            check(lib().wa_transcribe_beam(self._h, _ptr(mel), B, -1 if lang_token is None else int(lang_token),
                                           max_tokens, 1 if eot_stop else 0, ctypes.byref(bm),
                                           toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), ctypes.byref(sc),
                                           ctypes.byref(res), self._stream()))
        if not return_candidates and not timestamps:
            return [toks[b, : nt[b]].tolist() for b in range(B)]
        out = [{"tokens": toks[b, : nt[b]].tolist(), "sum_logprob": float(cs[b, best[b]]), "best": int(best[b]),
                "candidates": [{"tokens": ct[b, i, : cn[b, i]].tolist(), "sum_logprob": float(cs[b, i])}
                               for i in range(nc[b])],
                "no_speech_prob": float(ns[b]), "lang_token": int(lt[b]), "lang_prob": float(lpr[b])}
               for b in range(B)]
        if timestamps:
            for c in out:
                self._timestamped([c] + c["candidates"])
        return out

    def transcribe_batches(self, mels, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                           eot_stop: bool = True):
        """transcribe over mels cuda f32 [NB, B, n_mels, 3000], the next batch's
        encoder pipelined beside each decode (wa_transcribe_batches).  Returns
        NB lists of B token-id lists."""
        torch = _torch()
        mels = mels.contiguous()
        assert mels.dtype == torch.float32 and mels.is_cuda and mels.dim() == 4
        NB, B = mels.shape[0], mels.shape[1]
        toks = np.zeros((NB, B, max_tokens), np.int32)
        nt = np.zeros((NB, B), np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        check(lib().wa_transcribe_batches(self._h, ctypes.c_void_p(mels.data_ptr()), NB, B,
                                          -1 if lang_token is None else int(lang_token), max_tokens,
                                          1 if eot_stop else 0, toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p),
                                          self._stream()))
        return [[toks[i, b, : nt[i, b]].tolist() for b in range(B)] for i in range(NB)]

    @property
    def timestamp_begin(self) -> int:
        """<|0.00|>, the id after NO_TIMESTAMPS (50365 for Large-V3 / TINY_TEST, 50364 for Medium)."""
        return 50260 + self.config["n_lang"] + 4 + 1

    def _timestamped(self, clips):
        for c in clips:
            c["segments"], c["seek_frames"] = segments_from_tokens(c["tokens"], self.timestamp_begin)
        return clips

    def transcribe_timestamps(self, mel, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                              eot_stop: bool = True, max_initial: int = 50) -> list[dict]:
        """transcribe with timestamp tokens (wa_transcribe_timestamps): the prompt
        without NO_TIMESTAMPS, every pick under OpenAI's timestamp rules.  Per
        clip the dict of transcribe_scored (tokens: text and timestamp ids
        interleaved; the scores over the masked rows) plus segments, a list of
        (start_s, end_s, tokens), and seek_frames, the mel frame a following
        window would start at (segments_from_tokens)."""
        return self._timestamped(self._scored(mel, None, lang_token, max_tokens, eot_stop, max_initial))

    def transcribe_batches_timestamps(self, mels, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                                      eot_stop: bool = True, max_initial: int = 50) -> list[list[dict]]:
        """transcribe_batches with timestamp tokens (wa_transcribe_batches_timestamps):
        mels cuda f32 [NB, B, n_mels, 3000] -> NB lists of B dicts as transcribe_timestamps."""
        assert mels.dim() == 4
        return [self._timestamped(b)
                for b in self._scored(mels, mels.shape[0], lang_token, max_tokens, eot_stop, max_initial)]

    def transcribe_sampled(self, mel, temperature, seed, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                           eot_stop: bool = True, timestamps: bool = False, max_initial: int = 50) -> list[dict]:
        """transcribe with every pick drawn from softmax(z / T) (wa_transcribe_sampled):
        temperature (finite, >= 0; 0 decodes greedily) and seed per clip, or one
        value for all.  Per clip the dict of transcribe_scored -- the scores
        are untempered log-probabilities -- and with timestamps=True that of
        transcribe_timestamps (segments, seek_frames)."""
        clips = self._scored(mel, None, lang_token, max_tokens, eot_stop, max_initial,
                             sampling=(temperature, seed, timestamps))
        return self._timestamped(clips) if timestamps else clips

    def transcribe_batches_sampled(self, mels, temperature, seed, lang_token: Optional[int] = 50259,
                                   max_tokens: int = 224, eot_stop: bool = True, timestamps: bool = False,
                                   max_initial: int = 50) -> list[list[dict]]:
        """transcribe_batches with sampled picks (wa_transcribe_batches_sampled): mels
        cuda f32 [NB, B, n_mels, 3000], temperature / seed [NB, B] (or one value
        for all) -> NB lists of B dicts as transcribe_sampled."""
        assert mels.dim() == 4
        out = self._scored(mels, mels.shape[0], lang_token, max_tokens, eot_stop, max_initial,
                           sampling=(temperature, seed, timestamps))
        return [self._timestamped(b) for b in out] if timestamps else out

    def transcribe_fallback(self, mel, seed, temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                            logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                            lang_token: Optional[int] = 50259, max_tokens: int = 224, eot_stop: bool = True,
                            timestamps: bool = False, max_initial: int = 50) -> list[dict]:
        """The temperature fallback (wa_transcribe_fallback): decode at
        temperatures[0]; a clip whose mean log-probability is below
        logprob_threshold -- unless its no_speech_prob is above
        no_speech_threshold -- is decoded again at the next temperature, over
        the same encoder pass.  None switches a threshold off.  Rung r decodes
        clip c with seed[c] + r.  Per clip the dict of transcribe_sampled of the
        rung it kept, plus "rung" and "temperature"."""
        clips = self._scored(mel, None, lang_token, max_tokens, eot_stop, max_initial,
                             fallback=(temperatures, logprob_threshold, no_speech_threshold, seed, timestamps))
        return self._timestamped(clips) if timestamps else clips

    def transcribe_prompted(self, mel, prompts, max_tokens: int = 224, eot_stop: bool = True, temperature=None,
                            seed=0, timestamps: bool = False, max_initial: int = 50) -> list[dict]:
        """transcribe under the caller's prompts (wa_transcribe_prompted):
        prompts, one sequence of token ids per clip, of any lengths with
        max(len) + max_tokens <= n_text_ctx -- all of it the caller's
        (<|startofprev|> and previous text, SOT, language, task,
        NO_TIMESTAMPS).  temperature None: the greedy pick without timestamp
        rules; else as transcribe_sampled (0 decodes greedily; timestamps
        selects the rules).  Per clip the dict of transcribe_scored, the scores
        taken at the prompt's last SOT."""
        sampling = None if temperature is None else (temperature, seed, timestamps)
        clips = self._scored(mel, None, None, max_tokens, eot_stop, max_initial, sampling=sampling, prompts=prompts)
        return self._timestamped(clips) if timestamps and sampling is not None else clips

    def fallback_prompted(self, mel, prompts, seed, temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                          logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                          max_tokens: int = 224, eot_stop: bool = True, timestamps: bool = False,
                          max_initial: int = 50) -> list[dict]:
        """transcribe_fallback under the caller's prompts (wa_transcribe_fallback_prompted)."""
        clips = self._scored(mel, None, None, max_tokens, eot_stop, max_initial, prompts=prompts,
                             fallback=(temperatures, logprob_threshold, no_speech_threshold, seed, timestamps))
        return self._timestamped(clips) if timestamps else clips

    def prompt_logits_ragged(self, prompts):
        """After encode(): the prefill over prompts of any lengths (one id
        sequence per encoded clip) -> last-position logits [B, n_vocab]."""
        torch = _torch()
        ptok, pn, pld = _prompt_arrays(prompts)
        i32p = ctypes.POINTER(ctypes.c_int32)
        pr = Prompt(ptok.ctypes.data_as(i32p), pn.ctypes.data_as(i32p), pld)
        out = torch.empty((len(prompts), self.config["n_vocab"]), device=f"cuda:{self.device}", dtype=torch.float32)
        check(lib().wa_prompt_logits_ragged(self._h, ctypes.byref(pr), len(prompts), _ptr(out), self._stream()))
        return out

    def set_alignment_heads(self, pairs) -> None:
        """The (layer, head) pairs align() averages (wa_model_set_alignment_heads);
        an empty list restores the default, every head of the upper half of
        the decoder layers."""
        a = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        check(lib().wa_model_set_alignment_heads(self._h, _as(a, ctypes.c_int32), a.shape[0]))

    def align(self, mel, tokens, first_row=3, n_frames=3000, return_matrix: bool = False) -> list[dict]:
        """Token-level times of finished id sequences (wa_align, OpenAI's
        find_alignment): mel cuda f32 [B, n_mels, 3000]; tokens one whole id
        sequence per clip (SOT, language, task, NO_TIMESTAMPS, text ..., EOT);
        first_row (3 for that layout) and n_frames (the clip's content mel
        frames) one value or one per clip.  Per clip a dict: jump int32 [N], the
        frame at which token tokens[first_row + 1 + i] starts; start_s [N] =
        jump / 50; end_s [N - 1] = the next token's start (the last row, EOT,
        has none); matrix (return_matrix) cuda f32 [N, n_frames // 2], the head
        mean of the filtered attention weights the path was found in."""
        torch = _torch()
        mel = mel.contiguous()
        assert mel.dtype == torch.float32 and mel.is_cuda
        B = mel.shape[0]
        ptok, pn, pld = _prompt_arrays(tokens, B)
        fr = np.ascontiguousarray(np.broadcast_to(np.asarray(first_row, np.int32), (B,)))
        nf = np.ascontiguousarray(np.broadcast_to(np.asarray(n_frames, np.int32), (B,)))
        i32p = ctypes.POINTER(ctypes.c_int32)
        pr = Prompt(ptok.ctypes.data_as(i32p), pn.ctypes.data_as(i32p), pld)
        jump, rows = np.zeros((B, pld), np.int32), np.zeros(B, np.int32)
        mat = None
        if return_matrix:
            mat = torch.empty((B, pld, self.config["n_audio_ctx"]), device=mel.device, dtype=torch.float32)
        check(lib().wa_align(self._h, ctypes.c_void_p(mel.data_ptr()), B, ctypes.byref(pr), fr.ctypes.data_as(i32p),
                             nf.ctypes.data_as(i32p), jump.ctypes.data_as(i32p), rows.ctypes.data_as(i32p),
                             None if mat is None else _ptr(mat), self._stream()))
        out = []
        for b in range(B):
            j = jump[b, :rows[b]].copy()
            t = j.astype(np.float32) / np.float32(50.0)
            clip = dict(jump=j, start_s=t, end_s=t[1:].copy())
            if mat is not None:
                clip["matrix"] = mat[b, :rows[b], :nf[b] // 2]
            out.append(clip)
        return out

    def align_timings(self) -> dict:
        """Device times (ms) of the last align(): encoder, prefill with the capture, DTW, total."""
        t = (ctypes.c_float * 4)()
        check(lib().wa_last_align_timings(self._h, t))
        return dict(zip(("encoder_ms", "prefill_ms", "dtw_ms", "total_ms"), [float(v) for v in t]))

    def transcribe_long(self, audio, n_samples=None, seed=0, temperatures=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0),
                        logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                        lang_token: Optional[int] = 50259, max_tokens: int = 224, max_windows: int = 1 << 20,
                        max_initial: int = 50, initial_prompts=None, condition_on_previous_text: bool = False,
                        reset_temperature: float = 0.5) -> list[dict]:
        """Long-form transcription (wa_transcribe_long): OpenAI transcribe()'s
        loop -- the window at seek, timestamp decode with the temperature
        ladder, the silence skip, segments in absolute seconds, seek advanced
        to the last closed timestamp -- over many recordings at once, batches
        filled across recordings.  audio: a list of 1-D cuda f32 tensors (16
        kHz mono), or a 2-D tensor whose row r holds n_samples[r] samples
        (default: the whole row).  seed: one per recording, or one for all;
        window w of a recording decodes with seed + 8 w.  None switches a
        threshold off.  Per recording a dict: "windows", each the dict of
        transcribe_fallback's clip plus seek, size, advance (mel frames) and
        skipped; "segments", (start_s, end_s, tokens) in seconds of the
        recording; "truncated", whether max_windows ended it early.
        initial_prompts (one id sequence per recording, possibly empty) and
        condition_on_previous_text (OpenAI's default is True; here the caller
        chooses) run wa_transcribe_long_prompted: every window is prompted with
        the recording's previous text, and its dict gains "prompt_len".  The
        defaults are wa_transcribe_long."""
        torch = _torch()
        if isinstance(audio, (list, tuple)):
            assert n_samples is None and all(a.dim() == 1 for a in audio)
            n = _i64([a.numel() for a in audio])
            off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
            buf = torch.cat([a.reshape(-1) for a in audio]) if len(audio) > 1 else audio[0].contiguous()
            if buf.numel() == 0:
                buf = torch.zeros(1, device=buf.device, dtype=torch.float32)
        else:
            assert audio.dim() == 2
            buf = audio if audio.stride(1) == 1 and audio.numel() else audio.contiguous()
            S, L = buf.shape
            n = np.full(S, L, np.int64) if n_samples is None else np.broadcast_to(_i64(n_samples), (S,)).copy()
            assert int(n.max()) <= L
            off = np.arange(S, dtype=np.int64) * buf.stride(0)
        assert buf.dtype == torch.float32 and buf.is_cuda
        S = int(n.size)
        tl = np.ascontiguousarray(np.asarray(temperatures, np.float32).reshape(-1))
        _, sd = _sampling_arrays(0.0, seed, S)
        nan = float("nan")
        opt = LongOptions(int(max_tokens), int(max_windows), -1 if lang_token is None else int(lang_token),
                          int(max_initial), _as(tl, ctypes.c_float), int(tl.size),
                          nan if logprob_threshold is None else float(logprob_threshold),
                          nan if no_speech_threshold is None else float(no_speech_threshold),
                          _as(sd, ctypes.c_uint64))
        h = ctypes.c_void_p(None)
        prompted = initial_prompts is not None or condition_on_previous_text
        if prompted:
            itok, inn, ild = _prompt_arrays(initial_prompts if initial_prompts is not None else [[]] * S, S)
            lp = LongPrompt(_as(itok, ctypes.c_int32), _as(inn, ctypes.c_int32), ild,
                            1 if condition_on_previous_text else 0, float(reset_temperature))
            check(lib().wa_transcribe_long_prompted(self._h, _ptr(buf), S, _as(off, ctypes.c_int64),
                                                    _as(n, ctypes.c_int64), ctypes.byref(opt), ctypes.byref(lp),
                                                    ctypes.byref(h), self._stream()))
        else:
            check(lib().wa_transcribe_long(self._h, _ptr(buf), S, _as(off, ctypes.c_int64), _as(n, ctypes.c_int64),
                                           ctypes.byref(opt), ctypes.byref(h), self._stream()))
        try:
            return [self._long_stream(h, r, max_tokens, prompted) for r in range(S)]
        finally:
            lib().wa_long_result_free(h)

    @staticmethod
    def _long_stream(h, r: int, max_tokens: int, prompted: bool = False) -> dict:
        L = lib()
        nw, tr, nsg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(L.wa_long_result_stream(h, r, ctypes.byref(nw), ctypes.byref(tr), ctypes.byref(nsg)))
        wins = (LongWindow * max(1, nw.value))()
        segs = (LongSegment * max(1, nsg.value))()
        check(L.wa_long_result_windows(h, r, wins, nw.value, ctypes.byref(nw)))
        check(L.wa_long_result_segments(h, r, segs, nsg.value, ctypes.byref(nsg)))
        windows = []
        for i in range(nw.value):
            w = wins[i]
            toks, lp, nt = np.zeros(max_tokens, np.int32), np.zeros(max_tokens + 1, np.float32), ctypes.c_int()
            check(L.wa_long_result_window(h, r, i, _as(toks, ctypes.c_int32), max_tokens, ctypes.byref(nt),
                                          _as(lp, ctypes.c_float), max_tokens + 1))
            clip = _scored_clip(toks, nt.value, lp, w.no_speech_prob, w.lang_token, w.lang_prob)
            clip.update(avg_logprob=float(w.avg_logprob), rung=int(w.rung), temperature=float(w.temperature),
                        seek=int(w.seek), size=int(w.size), advance=int(w.advance), skipped=bool(w.skipped))
            if prompted:
                k = ctypes.c_int()
                check(L.wa_long_result_prompt_len(h, r, i, ctypes.byref(k)))
                clip["prompt_len"] = k.value
            windows.append(clip)
        segments = [(float(s.start), float(s.end), windows[s.window]["tokens"][s.tok_begin:s.tok_end])
                    for s in segs[:nsg.value]]
        return {"windows": windows, "segments": segments, "truncated": bool(tr.value)}

    def _scored(self, mels, NB: Optional[int], lang_token, max_tokens: int, eot_stop: bool,
                max_initial: Optional[int] = None, sampling=None, fallback=None, prompts=None):
        torch = _torch()
        mels = mels.contiguous()
        assert mels.dtype == torch.float32 and mels.is_cuda
        B = mels.shape[0] if NB is None else mels.shape[1]
        n = B * (NB or 1)
        toks = np.zeros((n, max_tokens), np.int32)
        nt = np.zeros(n, np.int32)
        lp = np.zeros((n, max_tokens + 1), np.float32)
        ns, lpr, lt = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        sc = Scores(lp.ctypes.data_as(f32p), ns.ctypes.data_as(f32p), lt.ctypes.data_as(i32p),
                    lpr.ctypes.data_as(f32p))
        lang = -1 if lang_token is None else int(lang_token)
        rung = None
        if prompts is not None:  # the prompted entries: the prompt in the language token's place
            assert NB is None
            ptok, pn, pld = _prompt_arrays(prompts, n)
            pr = Prompt(ptok.ctypes.data_as(i32p), pn.ctypes.data_as(i32p), pld)
        if prompts is not None and fallback is not None:
            temps, lp_thr, ns_thr, seed, ts = fallback
            tl = np.ascontiguousarray(np.asarray(temps, np.float32).reshape(-1))
            _, sd = _sampling_arrays(0.0, seed, n)
            nan = float("nan")
            fb = Fallback(tl.ctypes.data_as(f32p), int(tl.size), nan if lp_thr is None else float(lp_thr),
                          nan if ns_thr is None else float(ns_thr), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                          1 if ts else 0, int(max_initial))
            rung = np.zeros(n, np.int32)
            check(lib().wa_transcribe_fallback_prompted(self._h, _ptr(mels), B, ctypes.byref(pr), max_tokens,
                                                        1 if eot_stop else 0, ctypes.byref(fb),
                                                        toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p),
                                                        ctypes.byref(sc), rung.ctypes.data_as(i32p), self._stream()))
        elif prompts is not None:
            sm = None
            if sampling is not None:
                temperature, seed, ts = sampling
                t, sd = _sampling_arrays(temperature, seed, n)
                sm = ctypes.byref(Sampling(t.ctypes.data_as(f32p), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                           1 if ts else 0, int(max_initial)))
            check(lib().wa_transcribe_prompted(self._h, _ptr(mels), B, ctypes.byref(pr), max_tokens,
                                               1 if eot_stop else 0, sm, toks.ctypes.data_as(i32p),
                                               nt.ctypes.data_as(i32p), ctypes.byref(sc), self._stream()))
        elif fallback is not None:
            temps, lp_thr, ns_thr, seed, ts = fallback
            tl = np.ascontiguousarray(np.asarray(temps, np.float32).reshape(-1))
            _, sd = _sampling_arrays(0.0, seed, n)
            nan = float("nan")
            fb = Fallback(tl.ctypes.data_as(f32p), int(tl.size), nan if lp_thr is None else float(lp_thr),
                          nan if ns_thr is None else float(ns_thr), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                          1 if ts else 0, int(max_initial))
            rung = np.zeros(n, np.int32)
            check(lib().wa_transcribe_fallback(self._h, _ptr(mels), B, lang, max_tokens, 1 if eot_stop else 0,
                                               ctypes.byref(fb), toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p),
                                               ctypes.byref(sc), rung.ctypes.data_as(i32p), self._stream()))
        elif sampling is not None:
            temperature, seed, ts = sampling
            flat = lambda a, dt: np.asarray(a, dt).reshape(-1) if np.ndim(a) else a  # [NB, B] arrays: clip-major
            t, sd = _sampling_arrays(flat(temperature, np.float32), flat(seed, np.uint64), n)
            sm = Sampling(t.ctypes.data_as(f32p), sd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1 if ts else 0,
                          int(max_initial))
            f = lib().wa_transcribe_sampled if NB is None else lib().wa_transcribe_batches_sampled
            head = (self._h, _ptr(mels)) + ((B,) if NB is None else (NB, B))
            check(f(*head, lang, max_tokens, 1 if eot_stop else 0, ctypes.byref(sm), toks.ctypes.data_as(i32p),
                    nt.ctypes.data_as(i32p), ctypes.byref(sc), self._stream()))
        elif max_initial is not None:  # the timestamp entries: max_initial before the outputs
            f = lib().wa_transcribe_timestamps if NB is None else lib().wa_transcribe_batches_timestamps
            head = (self._h, _ptr(mels)) + ((B,) if NB is None else (NB, B))
            check(f(*head, lang, max_tokens, 1 if eot_stop else 0, int(max_initial), toks.ctypes.data_as(i32p),
                    nt.ctypes.data_as(i32p), ctypes.byref(sc), self._stream()))
        elif NB is None:
            check(lib().wa_transcribe_scored(self._h, _ptr(mels), B, lang, max_tokens, 1 if eot_stop else 0,
                                             toks.ctypes.data_as(i32p), nt.ctypes.data_as(i32p), ctypes.byref(sc),
                                             self._stream()))
        else:
            check(lib().wa_transcribe_batches_scored(self._h, _ptr(mels), NB, B, lang, max_tokens,
                                                     1 if eot_stop else 0, toks.ctypes.data_as(i32p),
                                                     nt.ctypes.data_as(i32p), ctypes.byref(sc), self._stream()))
        clips = [_scored_clip(toks[i], nt[i], lp[i], ns[i], lt[i], lpr[i]) for i in range(n)]
        if rung is not None:
            for c, r in zip(clips, rung):
                c["rung"], c["temperature"] = int(r), float(tl[r])
        return clips if NB is None else [clips[i * B:(i + 1) * B] for i in range(NB)]

    def transcribe_scored(self, mel, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                          eot_stop: bool = True) -> list[dict]:
        """transcribe with the scores of wa_transcribe_scored.  Per clip a dict:
        tokens (as transcribe), token_logprob (float32, one per token, plus the
        EOT pick's when the clip stopped on EOT), avg_logprob (their mean: the
        sum over len + 1 when the clip ended on EOT), no_speech_prob,
        lang_token, lang_prob, and logprob_slots (the raw max_tokens + 1
        slots, NaN where nothing was stored)."""
        return self._scored(mel, None, lang_token, max_tokens, eot_stop)

    def transcribe_batches_scored(self, mels, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                                  eot_stop: bool = True) -> list[list[dict]]:
        """transcribe_batches with scores (wa_transcribe_batches_scored): mels
        cuda f32 [NB, B, n_mels, 3000] -> NB lists of B dicts as transcribe_scored."""
        assert mels.dim() == 4
        return self._scored(mels, mels.shape[0], lang_token, max_tokens, eot_stop)

    def pipeline_stats(self) -> dict:
        """After transcribe_batches: batches, mean encoder layers run beside a
        decode, mean ms of that CU-masked part, CUs of the masked stream, and
        the units of two and of three batches that decoded together."""
        t = (ctypes.c_float * 4)()
        check(lib().wa_last_pipeline_stats(self._h, t))
        return {"batches": int(t[0]), "overlap_layers": t[1], "masked_ms": t[2], "masked_cus": int(t[3]),
                "pairs": self.pipeline_pairs(), "units3": self.pipeline_units3()}

    def pipeline_pairs(self) -> int:
        """Batch pairs the last transcribe_batches decoded together, one decode
        group per batch (wa_last_pipeline_pairs); 0: every batch on its own."""
        return int(lib().wa_last_pipeline_pairs(self._h))

    def pipeline_units3(self) -> int:
        """Units of three batches the last transcribe_batches decoded together
        (wa_last_pipeline_units3); pipeline_pairs counts those of exactly two."""
        return int(lib().wa_last_pipeline_units3(self._h))

    def decode_graph_key(self, group: int = 0) -> int:
        """Key of decode group `group`'s current step graph (wa_decode_graph_key; -1: none)."""
        return int(lib().wa_decode_graph_key(self._h, group))

    def transcribe_trace(self, mel, trace_ids: np.ndarray, lang_token: Optional[int] = 50259,
                         max_tokens: int = 224, eot_stop: bool = False):
        """transcribe + the decode-step logit trace (wa_transcribe_trace):
        trace_ids int32 [B, max_tokens + 1, K] -> (tokens, logits [B,
        max_tokens + 1, K] float32; slot 0 and slots past a clip's last step
        are NaN)."""
        torch = _torch()
        mel = mel.contiguous()
        B = mel.shape[0]
        K = trace_ids.shape[-1]
        assert trace_ids.shape == (B, max_tokens + 1, K)
        ids = torch.from_numpy(np.ascontiguousarray(trace_ids, np.int32)).to(mel.device)
        out = torch.full((B, max_tokens + 1, K), float("nan"), device=mel.device, dtype=torch.float32)
        toks = np.zeros((B, max_tokens), np.int32)
        nt = np.zeros(B, np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        check(lib().wa_transcribe_trace(self._h, _ptr(mel), B, -1 if lang_token is None else int(lang_token),
                                        max_tokens, 1 if eot_stop else 0, toks.ctypes.data_as(i32p),
                                        nt.ctypes.data_as(i32p), _ptr(ids), K, _ptr(out), self._stream()))
        return [toks[b, : nt[b]].tolist() for b in range(B)], out.cpu().numpy()

    def transcribe_audio(self, audio, lang_token: Optional[int] = 50259, max_tokens: int = 224,
                         eot_stop: bool = True, n_samples: Optional[int] = None):
        """src/transcribe.rs:34-107 from 16 kHz samples (cuda f32 [B, L]) to
        token ids: GPU log-mel (log_mel) then transcribe."""
        mel = log_mel(audio, self.config["n_mels"], n_samples)
        return self.transcribe(mel, lang_token, max_tokens, eot_stop)

    def last_timings(self) -> dict:
        t = (ctypes.c_float * 5)()
        check(lib().wa_last_timings(self._h, t))
        return {"encoder_ms": t[0], "cross_kv_ms": t[1], "prompt_ms": t[2], "decode_ms": t[3], "steps": int(t[4])}

    PROF_NAMES = ("q4_gemm", "encoder_attention", "conv", "layernorm")

    def profile_enable(self, on: bool = True) -> None:
        check(lib().wa_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, reset: bool = True) -> dict:
        """Per category: launches, ms, algorithmic GFLOP and GB (HIP events)."""
        buf = (ctypes.c_double * 16)()
        check(lib().wa_profile_read(self._h, buf, 1 if reset else 0))
        return {n: {"launches": int(buf[4 * i]), "ms": buf[4 * i + 1], "gflop": buf[4 * i + 2], "gb": buf[4 * i + 3]}
                for i, n in enumerate(self.PROF_NAMES)}

    def probe_kernels(self, n_clips: int, iters: int = 20) -> dict:
        """HIP-event timing of single decode-step kernels (after transcribe)."""
        buf = (ctypes.c_double * 6)()
        check(lib().wa_probe_kernels(self._h, n_clips, iters, buf, len(buf)))
        return {"cross_attention": {"us": buf[0], "bytes": buf[1], "kv_cache": buf[5] != 0.0},
                "decode_fc1": {"us": buf[2], "bytes": buf[3], "flops": buf[4]}}

    def encode(self, mel):
        """encoder.rs:87-115 -> encoder_out [B, 1500, D] (also writes the f16 encoder-output planes the decoder cross-attention reads)."""
        torch = _torch()
        B = mel.shape[0]
        out = torch.empty((B, self.config["n_audio_ctx"], self.config["n_audio_state"]), device=mel.device,
                          dtype=torch.float32)
        check(lib().wa_encode(self._h, ctypes.c_void_p(mel.contiguous().data_ptr()), B,
                              ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def prompt_logits(self, prompt):
        """decoder.rs:251-296 after encode(): prompt int32 cuda [B, T<=4] -> last-position logits."""
        torch = _torch()
        B, T = prompt.shape
        out = torch.empty((B, self.config["n_vocab"]), device=prompt.device, dtype=torch.float32)
        check(lib().wa_prompt_logits(self._h, ctypes.c_void_p(prompt.contiguous().data_ptr()), B, T,
                                     ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def close(self):
        if self._h and self._h.value:
            lib().wa_model_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
