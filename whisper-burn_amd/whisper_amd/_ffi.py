"""The ctypes side of libwhisper_amd.so: the library handle, the structs of
include/whisper_amd.h, one table of argument types for every entry of the two
headers (tests/test_ffi_table.py holds it to the prototypes), and the pointer
helpers the wrappers share.  Loud failure if the native libraries are missing.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

import wq4

LIB_PATH = os.path.join(os.path.dirname(wq4.LIB_PATH), "libwhisper_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(wq4.HEADER_PATH), "whisper_amd.h")
CHECKS_HEADER_PATH = os.path.join(os.path.dirname(wq4.HEADER_PATH), "whisper_amd_checks.h")
_lib: Optional[ctypes.CDLL] = None


class Scores(ctypes.Structure):
    """struct wa_scores: host arrays, each nullable."""

    _fields_ = [("token_logprob", ctypes.POINTER(ctypes.c_float)), ("no_speech_prob", ctypes.POINTER(ctypes.c_float)),
                ("lang_token", ctypes.POINTER(ctypes.c_int32)), ("lang_prob", ctypes.POINTER(ctypes.c_float))]


class Beam(ctypes.Structure):
    """struct wa_beam: beams per clip, finished sequences kept per clip, length penalty (NaN: none)."""

    _fields_ = [("beam_size", ctypes.c_int), ("max_candidates", ctypes.c_int), ("length_penalty", ctypes.c_float)]


class BeamOptions(ctypes.Structure):
    """struct wa_beam_options: timestamp rules, their max_initial, one caller prompt per clip (nullable)."""

    _fields_ = [("timestamps", ctypes.c_int), ("max_initial", ctypes.c_int), ("prompt", ctypes.c_void_p)]


class BeamResult(ctypes.Structure):
    """struct wa_beam_result: host arrays, each nullable."""

    _fields_ = [("cand_tokens", ctypes.POINTER(ctypes.c_int32)), ("cand_n_tokens", ctypes.POINTER(ctypes.c_int32)),
                ("cand_sum_logprob", ctypes.POINTER(ctypes.c_float)), ("n_candidates", ctypes.POINTER(ctypes.c_int32)),
                ("best", ctypes.POINTER(ctypes.c_int32))]


class Segment(ctypes.Structure):
    """struct wa_segment: tokens [tok_begin, tok_end) from start_s to end_s."""

    _fields_ = [("start_s", ctypes.c_float), ("end_s", ctypes.c_float), ("tok_begin", ctypes.c_int32),
                ("tok_end", ctypes.c_int32)]


class Sampling(ctypes.Structure):
    """struct wa_sampling: per-clip host temperatures and seeds of a sampled transcribe."""

    _fields_ = [("temperature", ctypes.POINTER(ctypes.c_float)), ("seed", ctypes.POINTER(ctypes.c_uint64)),
                ("timestamps", ctypes.c_int), ("max_initial", ctypes.c_int)]


class Fallback(ctypes.Structure):
    """struct wa_fallback: the temperature ladder, its thresholds and the clips' seeds."""

    _fields_ = [("temperatures", ctypes.POINTER(ctypes.c_float)), ("n_temperatures", ctypes.c_int),
                ("logprob_threshold", ctypes.c_float), ("no_speech_threshold", ctypes.c_float),
                ("seed", ctypes.POINTER(ctypes.c_uint64)), ("timestamps", ctypes.c_int),
                ("max_initial", ctypes.c_int)]


class LongOptions(ctypes.Structure):
    """struct wa_long_options: one transcribe_long call's decode options."""

    _fields_ = [("max_tokens", ctypes.c_int), ("max_windows", ctypes.c_int), ("lang_token", ctypes.c_int),
                ("max_initial", ctypes.c_int), ("temperatures", ctypes.POINTER(ctypes.c_float)),
                ("n_temperatures", ctypes.c_int), ("logprob_threshold", ctypes.c_float),
                ("no_speech_threshold", ctypes.c_float), ("seed", ctypes.POINTER(ctypes.c_uint64))]


class LongWindow(ctypes.Structure):
    """struct wa_long_window: one decoded window of a recording."""

    _fields_ = [(n, ctypes.c_int32) for n in ("stream", "index", "seek", "size", "advance", "skipped", "rung",
                                               "lang_token", "n_tokens")] + \
               [(n, ctypes.c_float) for n in ("temperature", "no_speech_prob", "lang_prob")] + \
               [("avg_logprob", ctypes.c_double)]


class LongSegment(ctypes.Structure):
    """struct wa_long_segment: tokens [tok_begin, tok_end) of a window, in seconds of the recording."""

    _fields_ = [("stream", ctypes.c_int32), ("window", ctypes.c_int32), ("tok_begin", ctypes.c_int32),
                ("tok_end", ctypes.c_int32), ("start", ctypes.c_double), ("end", ctypes.c_double)]


class Prompt(ctypes.Structure):
    """struct wa_prompt: host prompts [n_clips, ld] and their lengths."""

    _fields_ = [("tokens", ctypes.POINTER(ctypes.c_int32)), ("n_tokens", ctypes.POINTER(ctypes.c_int32)),
                ("ld", ctypes.c_int)]


class LongPrompt(ctypes.Structure):
    """struct wa_long_prompt: per-recording initial prompts and the conditioning switch."""

    _fields_ = [("initial", ctypes.POINTER(ctypes.c_int32)), ("n_initial", ctypes.POINTER(ctypes.c_int32)),
                ("ld", ctypes.c_int), ("condition_on_previous_text", ctypes.c_int),
                ("reset_temperature", ctypes.c_float)]


def _table() -> tuple[dict, dict]:
    """(name -> argtypes of every wa_* entry, name -> restype where it is not int)."""
    vp, ci, i64, u64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
    f32, f64, cs = ctypes.c_float, ctypes.c_double, ctypes.c_char_p
    P = ctypes.POINTER
    i32p, f32p, u64p, i64p, cip, vpp = P(ctypes.c_int32), P(f32), P(u64), P(i64), P(ci), P(vp)
    sp, pp, smp, fbp, bmp = P(Scores), P(Prompt), P(Sampling), P(Fallback), P(Beam)
    argtypes = {
        # ---- include/whisper_amd.h
        "wa_last_error": [],
        "wa_model_create_synthetic": [ci, ci, u64, ci, ci, vpp],
        "wa_model_create_synthetic_ex": [ci, ci, u64, ci, ci, ci, vpp],
        "wa_model_weight_type": [vp],
        "wa_model_wide_range": [vp],
        "wa_model_create_from_gguf": [ci, cs, ci, ci, ci, vpp],
        "wa_model_destroy": [vp],
        "wa_gguf_open": [cs, vpp],
        "wa_gguf_close": [vp],
        "wa_gguf_version": [vp],
        "wa_gguf_tensor_count": [vp],
        "wa_gguf_tensor_info": [vp, i64, cs, sz, cip, u64p, cip, u64p, u64p],
        "wa_gguf_tensor_data": [vp, cs, P(ctypes.c_uint8), sz],
        "wa_model_config": [vp, i32p],
        "wa_model_device_bytes": [vp],
        "wa_transcribe": [vp, vp, ci, ci, ci, ci, i32p, i32p, vp],
        "wa_transcribe_batches": [vp, vp, ci, ci, ci, ci, ci, i32p, i32p, vp],
        "wa_transcribe_scored": [vp, vp, ci, ci, ci, ci, i32p, i32p, sp, vp],
        "wa_transcribe_batches_scored": [vp, vp, ci, ci, ci, ci, ci, i32p, i32p, sp, vp],
        "wa_transcribe_timestamps": [vp, vp, ci, ci, ci, ci, ci, i32p, i32p, sp, vp],
        "wa_transcribe_batches_timestamps": [vp, vp, ci, ci, ci, ci, ci, ci, i32p, i32p, sp, vp],
        "wa_segments_from_tokens": [i32p, ci, ci, P(Segment), ci, cip, cip],
        "wa_timestamp_rule": [i32p, ci, ci, ci, ci, i32p],
        "wa_transcribe_sampled": [vp, vp, ci, ci, ci, ci, smp, i32p, i32p, sp, vp],
        "wa_transcribe_batches_sampled": [vp, vp, ci, ci, ci, ci, ci, smp, i32p, i32p, sp, vp],
        "wa_sample_noise": [u64, ci, ci, ci, f32p, f32p],
        "wa_transcribe_fallback": [vp, vp, ci, ci, ci, ci, fbp, i32p, i32p, sp, i32p, vp],
        "wa_prompt_check": [pp, ci, ci, ci, ci],
        "wa_transcribe_prompted": [vp, vp, ci, pp, ci, ci, smp, i32p, i32p, sp, vp],
        "wa_transcribe_fallback_prompted": [vp, vp, ci, pp, ci, ci, fbp, i32p, i32p, sp, i32p, vp],
        "wa_model_set_alignment_heads": [vp, i32p, ci],
        "wa_alignment_heads_check": [i32p, ci, ci, ci],
        "wa_align_check": [pp, ci, i32p, i32p, ci, ci, ci],
        "wa_align": [vp, vp, ci, pp, i32p, i32p, i32p, i32p, vp, vp],
        "wa_last_align_timings": [vp, f32p],
        "wa_align_words": [i32p, ci, i32p, ci, f32p, f32p],
        "wa_transcribe_beam": [vp, vp, ci, ci, ci, ci, bmp, i32p, i32p, sp, P(BeamResult), vp],
        "wa_transcribe_beam_ex": [vp, vp, ci, ci, ci, ci, bmp, P(BeamOptions), i32p, i32p, sp, P(BeamResult), vp],
        "wa_beam_check": [bmp, ci, ci],
        "wa_beam_rank": [f32p, i32p, ci, f32, i32p],
        "wa_last_pipeline_stats": [vp, f32p],
        "wa_last_pipeline_pairs": [vp],
        "wa_last_pipeline_units3": [vp],
        "wa_suppress_check": [i32p, ci, i32p, ci, ci],
        "wa_model_set_suppress": [vp, i32p, ci, i32p, ci],
        "wa_model_suppress_ids": [vp, ci, i32p, ci, cip],
        "wa_log_mel": [ci, vp, ci, i64, i64, ci, vp, vp],
        "wa_mel_filterbank": [ci, f32p, f32p],
        "wa_long_mel_max": [ci, vp, ci, i64p, i64p, ci, vp, vp],
        "wa_long_mel_windows": [ci, vp, ci, i64p, i64p, i32p, i32p, vp, ci, vp, vp],
        "wa_long_advance": [i32p, ci, ci, ci, f32, f64, f32, f32, cip, cip],
        "wa_long_round": [i32p, i32p, i32p, ci, ci, ci, cip, cip],
        "wa_transcribe_long": [vp, vp, ci, i64p, i64p, P(LongOptions), vpp, vp],
        "wa_long_result_free": [vp],
        "wa_long_result_streams": [vp],
        "wa_long_result_max_tokens": [vp],
        "wa_long_result_stream": [vp, ci, cip, cip, cip],
        "wa_long_result_windows": [vp, ci, P(LongWindow), ci, cip],
        "wa_long_result_window": [vp, ci, ci, i32p, ci, cip, f32p, ci],
        "wa_long_result_segments": [vp, ci, P(LongSegment), ci, cip],
        "wa_transcribe_long_prompted": [vp, vp, ci, i64p, i64p, P(LongOptions), P(LongPrompt), vpp, vp],
        "wa_long_result_prompt_len": [vp, ci, ci, cip],
        "wa_long_prompt_window": [i32p, ci, ci, ci, ci, ci, ci, ci, i32p, ci, cip, cip],
        "wa_long_prompt_next": [i32p, cip, cip, i32p, ci, ci, ci, f32, ci, f32],
        "wa_last_timings": [vp, f32p],
        "wa_profile_enable": [vp, ci],
        "wa_profile_read": [vp, P(f64), ci],
        "wa_probe_kernels": [vp, ci, ci, P(f64), ci],
        "wa_decode_group_rows": [ci],
        # ---- include/whisper_amd_checks.h
        "wa_encode": [vp, vp, ci, vp, vp],
        "wa_prompt_logits": [vp, vp, ci, ci, vp, vp],
        "wa_prompt_logits_ragged": [vp, pp, ci, vp, vp],
        "wa_transcribe_trace": [vp, vp, ci, ci, ci, ci, i32p, i32p, vp, ci, vp, vp],
        "wa_decode_graph_key": [vp, ci],
        "wa_synth_uniform": [u64, cs, i64, f32, f32, f32p],
        "wa_decode_graph_key_check": [ci] * 10,
        "wa_xattn_resident_share": [ci, ci, ci, ci, f64],
        "wa_xattn_chunk_resident": [ci, ci],
        "wa_xattn_plan": [ci, cip, cip],
        "wa_xattn_plan_splits": [ci, ci, ci, cip, cip],
        "wa_pipeline_unit_sizes": [ci, ci, cip, cip],
        "wa_xattn_check": [ci, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp],
        "wa_xattn_kv_check": [ci, vp, vp, vp, ci, ci, ci, ci, ci, vp],
        "wa_encoder_attention_check": [ci, vp, ci, ci, ci, ci, vp],
        "wa_self_attention_check": [ci, vp, vp, vp, vp, i32p, ci, ci, ci, ci, ci, ci, ci, vp],
        "wa_self_attention_prefill_check": [ci, vp, vp, vp, ci, ci, i32p, ci, ci, ci, vp],
        "wa_cross_attention_prefill_check": [ci, vp, vp, vp, ci, ci, ci, ci, ci, vp],
        "wa_conv_gelu_check": [ci, vp, i64, i64, i64, ci, ci, ci, ci, vp, vp, vp, ci, vp],
        "wa_embed_check": [ci, i32p, vp, ci, vp, ci, ci, ci, ci, ci, ci, i32p, vp, ci, vp, vp, vp],
        "wa_logits_pick_check": [ci, vp, vp, ci, ci, ci, ci, ci, i32p, ci, f32p, u64p, ci, i32p, vp, vp, vp, vp],
        "wa_row_pick_check": [ci, vp, ci, ci, ci, ci, i32p, ci, f32p, u64p, ci, i32p, vp, vp, vp],
        "wa_row_logprob_check": [ci, vp, ci, ci, ci, ci, ci, vp, ci, vp],
        "wa_timestamp_bookkeep_check": [ci, i32p, ci, ci, ci, ci, ci, i32p],
        "wa_beam_topk_check": [ci, vp, ci, ci, ci, ci, ci, ci, ci, i32p, ci, i32p, vp, vp, vp, i32p],
        "wa_beam_select_check": [ci] + [vp] * 14 + [ci] * 6,
        "wa_align_matrix_check": [ci, vp, vp, ci, ci, i32p, ci, ci, i32p, ci, i32p, ci, ci, vp],
        "wa_dtw_check": [ci, vp, ci, ci, ci, i32p, i32p, vp, vp],
    }
    restype = {
        "wa_last_error": cs,
        "wa_model_destroy": None,
        "wa_gguf_close": None,
        "wa_long_result_free": None,
        "wa_model_device_bytes": sz,
        "wa_gguf_tensor_count": i64,
        "wa_decode_graph_key": ctypes.c_longlong,
        "wa_decode_graph_key_check": ctypes.c_longlong,
    }
    return argtypes, restype


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        wq4.lib()  # libwq4.so first (RTLD_GLOBAL)
        if not os.path.exists(LIB_PATH):
            raise wq4.WQ4Error(6, f"{LIB_PATH} not built")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        argtypes, restype = _table()
        for name, args in argtypes.items():
            getattr(L, name).argtypes = args
        for name, res in restype.items():
            getattr(L, name).restype = res
        _lib = L
    return _lib


def check(st: int) -> None:
    if st != 0:
        raise wq4.WQ4Error(st, lib().wa_last_error().decode(errors="replace"))


def _torch():
    import torch

    return torch


def _dev(t) -> int:
    return t.device.index if t.device.index is not None else 0


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64).reshape(-1))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


def _as(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))
