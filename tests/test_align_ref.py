"""Token alignment, what can be checked without a GPU: align_ref.py's float64
restatement against a torch-CPU transliteration of OpenAI's timing.py lines,
the f32 DTW on the cases where its rule bites, align_words and the argument
checks of the entries, the exported surface, and the precondition of the
planted GPU cases (the reference path survives the bound)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import align_ref as R
import whisper_amd

EINVAL = 1
i32p = ctypes.POINTER(ctypes.c_int32)

NEW = ("wa_model_set_alignment_heads", "wa_align", "wa_align_words", "wa_align_matrix_check", "wa_dtw_check",
       "wa_alignment_heads_check", "wa_align_check", "wa_last_align_timings")


@pytest.mark.parametrize("name", NEW)
def test_symbols_exported_and_declared(name):
    assert hasattr(whisper_amd.lib(), name)
    assert name in open(whisper_amd.HEADER_PATH).read() + open(whisper_amd.CHECKS_HEADER_PATH).read()


def test_python_surface():
    for n in ("set_alignment_heads", "align"):
        assert callable(getattr(whisper_amd.WhisperModel, n))
    for n in ("align_words", "align_matrix_check", "dtw_check"):
        assert callable(getattr(whisper_amd, n))


# ------------------------------------------- OpenAI's lines, transliterated --
def openai_matrix(weights, first_row):
    """timing.py find_alignment from the stacked head weights [heads, n, F]
    (its QKs softmaxed) to the matrix: std_mean(unbiased=False) over the token
    axis, median_filter(7), the head mean, the rows sliced."""
    import torch
    import torch.nn.functional as F

    w = torch.from_numpy(np.asarray(weights, np.float64))
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    w = (w - mean) / std
    pad = F.pad(w[None], (3, 3, 0, 0), mode="reflect")[0]  # median_filter's reflect padding of width // 2
    w = pad.unfold(-1, 7, 1).sort()[0][..., 3]
    return w.mean(dim=0)[first_row:-1].numpy()


def openai_dtw(x):
    """timing.py dtw_cpu + backtrace, and find_alignment's jump_times (in frames)."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.ones((N + 1, M + 1), dtype=np.float32) * np.inf
    trace = -np.ones((N + 1, M + 1), dtype=np.float32)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0 = cost[i - 1, j - 1]
            c1 = cost[i - 1, j]
            c2 = cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = x[i - 1, j - 1] + c
            trace[i, j] = t
    i, j = trace.shape[0] - 1, trace.shape[1] - 1
    trace[0, :] = 2
    trace[:, 0] = 1
    result = []
    while i > 0 or j > 0:
        result.append((i - 1, j - 1))
        if trace[i, j] == 0:
            i -= 1
            j -= 1
        elif trace[i, j] == 1:
            i -= 1
        else:
            j -= 1
    text_indices, time_indices = np.array(result)[::-1, :].T
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    return time_indices[jumps], trace.astype(np.uint8)


@pytest.mark.parametrize("n,F,heads,first_row", [(9, 40, 3, 3), (2, 4, 1, 0), (30, 7, 5, 2)])
def test_matrix_restatement_equals_openai_lines(n, F, heads, first_row):
    rng = np.random.default_rng(n * 100 + F)
    qk = [(rng.standard_normal((n, 64)), rng.standard_normal((F, 64))) for _ in range(heads)]
    w = np.stack([R.weights64(q, k)[0] for q, k in qk])
    got = R.matrix64(qk, first_row)
    want = openai_matrix(w, first_row)
    assert got.shape == (n - 1 - first_row, F)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_zero_std_column_gives_zero_where_openai_gives_nan():
    rng = np.random.default_rng(1)
    q, k = rng.standard_normal((1, 64)).repeat(3, axis=0), rng.standard_normal((9, 64))
    w = R.weights64(q, k)[0]
    assert not R.standardise(w).any() and not R.matrix64([(q, k)], 0).any()
    assert np.isnan(openai_matrix(w[None], 0)).all()


def dtw_cases():
    rng = np.random.default_rng(5)
    yield "ties_integer", rng.integers(-2, 3, (12, 17)).astype(np.float32)
    yield "all_equal", np.zeros((6, 9), np.float32)
    yield "n_gt_f", rng.standard_normal((9, 4)).astype(np.float32)
    yield "n_gt_f_ties", rng.integers(0, 2, (7, 3)).astype(np.float32)
    yield "n_1", rng.standard_normal((1, 11)).astype(np.float32)
    yield "f_4", rng.standard_normal((5, 4)).astype(np.float32)
    yield "n_1_f_4", rng.standard_normal((1, 4)).astype(np.float32)
    yield "normal", rng.standard_normal((23, 57)).astype(np.float32)


@pytest.mark.parametrize("name,x", list(dtw_cases()), ids=[n for n, _ in dtw_cases()])
def test_f32_dtw_equals_openai_lines(name, x):
    want_jump, want_trace = openai_dtw(x)
    for f in (R.dtw, R.dtw_loops):
        jump, trace = f(x)
        assert np.array_equal(jump, want_jump), f.__name__
        assert np.array_equal(trace, want_trace), f.__name__
    assert len(want_jump) == x.shape[0] and (np.diff(want_jump) >= 0).all()


def test_f32_dtw_is_not_the_f64_dtw_on_near_ties():
    """The restatement rounds every cell to f32: costs that differ below f32
    resolution tie (trace 2) where float64 would tell them apart."""
    x = np.array([[1.0, 1.0, 1.0], [1.0, 1.0 + 1e-9, 1.0], [1.0, 1.0, 1.0]])
    assert not np.array_equal(R.dtw(x, np.float32)[1], R.dtw(x, np.float64)[1])


def test_align_words_hand_computed():
    jump = [0, 3, 5, 9, 12, 40]  # 5 tokens + EOT
    start, end = whisper_amd.align_words(jump, [1, 3, 1])
    assert np.array_equal(start, np.array([0.0, 0.06, 0.24], np.float32))
    assert np.array_equal(end, np.array([0.06, 0.24, 0.8], np.float32))
    rs, re = R.align_words(jump, [1, 3, 1])
    np.testing.assert_allclose(start, rs, rtol=1e-7)
    np.testing.assert_allclose(end, re, rtol=1e-7)
    s0, e0 = whisper_amd.align_words([7], [])  # EOT alone: no words
    assert s0.size == 0 and e0.size == 0
    s1, e1 = whisper_amd.align_words([2, 4, 9], [0, 2])  # an empty word starts and ends where the next starts
    assert np.array_equal(s1, np.array([0.04, 0.04], np.float32)) and np.array_equal(e1, np.array([0.04, 0.18], np.float32))
    for bad in ([1, 1], [4], [1, -1, 5]):
        with pytest.raises(whisper_amd.wq4.WQ4Error):
            whisper_amd.align_words(jump, bad)
    L = whisper_amd.lib()
    f = (ctypes.c_float * 4)()
    j = (ctypes.c_int32 * 3)(1, 2, 3)
    assert L.wa_align_words(None, 3, j, 1, f, f) == EINVAL
    assert L.wa_align_words(j, 0, j, 0, f, f) == EINVAL


def prompt_struct(seqs):
    tok, n, ld = whisper_amd._prompt_arrays(seqs)
    return whisper_amd.Prompt(tok.ctypes.data_as(i32p), n.ctypes.data_as(i32p), ld), (tok, n)


V, CTX, T = 51866, 448, 1500
GOOD = [[50258, 50259, 50360, 50364, 11, 12, 50257], [50258, 50259, 50360, 50364, 13, 50257]]


def align_check(seqs, first_row, n_frames, n_clips=None):
    p, keep = prompt_struct(seqs)
    fr, nf = np.asarray(first_row, np.int32), np.asarray(n_frames, np.int32)
    st = whisper_amd.lib().wa_align_check(ctypes.byref(p), len(seqs) if n_clips is None else n_clips,
                                          fr.ctypes.data_as(i32p), nf.ctypes.data_as(i32p), V, CTX, T)
    del keep
    return st


def test_align_check_accepts_and_rejects():
    assert align_check(GOOD, [3, 3], [3000, 8]) == 0
    assert align_check(GOOD, [0, 4], [9, 2999]) == 0  # N = 1 for the second clip
    assert align_check(GOOD, [-1, 3], [3000, 3000]) == EINVAL
    assert align_check(GOOD, [3, 5], [3000, 3000]) == EINVAL  # N = 0
    assert align_check(GOOD, [3, 3], [7, 3000]) == EINVAL
    assert align_check(GOOD, [3, 3], [3000, 3001]) == EINVAL
    assert align_check(GOOD, [3, 3], [3000, 3000], n_clips=0) == EINVAL
    assert align_check([[50258, V]], [0], [3000]) == EINVAL  # an id outside the vocabulary
    assert align_check([[7] * (CTX + 1)], [0], [3000]) == EINVAL  # longer than n_text_ctx
    assert align_check([[7] * CTX], [0], [3000]) == 0
    L = whisper_amd.lib()
    p, keep = prompt_struct(GOOD)
    a = (ctypes.c_int32 * 2)(3, 3)
    assert L.wa_align_check(None, 2, a, a, V, CTX, T) == EINVAL
    assert L.wa_align_check(ctypes.byref(p), 2, None, a, V, CTX, T) == EINVAL
    assert L.wa_align_check(ctypes.byref(p), 2, a, None, V, CTX, T) == EINVAL
    del keep


def test_entries_reject_before_any_device_work():
    L = whisper_amd.lib()
    p, keep = prompt_struct(GOOD)
    a, out = (ctypes.c_int32 * 2)(3, 3), (ctypes.c_int32 * 16)()
    buf = (ctypes.c_float * 16)()
    addr = lambda b: ctypes.c_void_p(ctypes.addressof(b))
    assert L.wa_align(None, addr(buf), 2, ctypes.byref(p), a, a, out, out, None, None) == EINVAL
    assert L.wa_model_set_alignment_heads(None, a, 1) == EINVAL
    assert L.wa_last_align_timings(None, buf) == EINVAL
    # the check entries: null pointers and sizes, before the device is touched
    assert L.wa_align_matrix_check(0, None, addr(buf), 1, 2, a, 8, 1, a, 1, a, 0, 0, addr(buf)) == EINVAL
    assert L.wa_dtw_check(0, None, 1, 2, 2, a, a, addr(buf), None) == EINVAL
    assert L.wa_dtw_check(0, addr(buf), 1, 448, 2, a, a, addr(buf), None) == EINVAL  # N_ld past 447
    del keep


def heads_check(pairs, layers=4, heads=6):
    a = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    return whisper_amd.lib().wa_alignment_heads_check(a.ctypes.data_as(i32p), a.shape[0], layers, heads)


def test_alignment_heads_check():
    assert heads_check([]) == 0  # the default
    assert heads_check([(3, 5), (0, 0), (3, 0)]) == 0
    assert heads_check([(4, 0)]) == EINVAL
    assert heads_check([(0, 6)]) == EINVAL
    assert heads_check([(-1, 0)]) == EINVAL
    assert heads_check([(0, -1)]) == EINVAL
    assert heads_check([(1, 2), (2, 1), (1, 2)]) == EINVAL
    assert whisper_amd.lib().wa_alignment_heads_check(None, 2, 4, 6) == EINVAL
    assert whisper_amd.lib().wa_alignment_heads_check(None, -1, 4, 6) == EINVAL


# ------------------------------------------------------------- the bound --
def test_bound_is_small_where_the_matrix_is_decided_and_has_teeth():
    """On a planted head the bound is far below the matrix's own scale, and a
    softmax that sees one frame past F leaves it."""
    q, k = R.planted_head(33, 65, 80, 3, 0)
    M, bound = R.matrix_ref([(q, k[:65])], 0, "f16x2")
    assert np.isfinite(bound).all() and np.median(bound) < 1e-3 * np.abs(M).max()
    wrong = R.matrix64([(q, k[:66])], 0)[:, :65]
    assert (np.abs(wrong - M) > bound).any()
    # WQ4_PREC_F16 carries the hi halves' worst case: a wider bound
    assert (R.matrix_ref([(q, k[:65])], 0, "f16")[1] >= bound).all()


def test_planted_diagonal_path_survives_the_bound():
    """The precondition of test_align_gpu's planted-diagonal case: the float64
    path over -M is unchanged when M moves by +- its bound under 8 random sign
    patterns, so a device M inside the bound is expected to give that path."""
    _, _, per_clip = R.matrix_case(**R.DIAGONAL_CASE)
    for hs, n, F in zip(per_clip, R.DIAGONAL_CASE["ns"], R.DIAGONAL_CASE["Fs"]):
        M, bound = R.matrix_ref(hs, R.DIAGONAL_FIRST_ROW, "f16x2")
        assert np.isfinite(bound).all()
        assert R.path_is_stable(M, bound)
        jump = R.dtw(-M, np.float64)[0]
        # a diagonal: every row enters within a bump's width of where its bump crosses the one before
        want = (np.arange(R.DIAGONAL_FIRST_ROW, n - 1)) * F / n
        assert jump[0] == 0 and np.abs(jump - want)[1:].max() <= F / n + 3
