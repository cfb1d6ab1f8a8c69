"""Token alignment on the GPU (wa_align): the DTW kernel bit for bit against the
f32 restatement, the weights + filter kernels against the float64 restatement
within align_ref.py's derived bound on planted inputs, and WhisperModel.align
on tiny_test against the float64 oracle, against the host DTW of its own
matrix, and bit-identical across batch compositions.

Worst error / bound seen on an MI355X (the ALIGN_WORST lines of `pytest -s`;
DESIGN.md section 3 "Token alignment against float64"): planted matrices 0.11
at two planes and 0.03 at WQ4_PREC_F16, the planted diagonal 0.02, the model
on tiny_test 0.02; the float64 path survives the bound on two of the model's
three clips, and the GPU's jumps equal it there.
"""
from __future__ import annotations

import numpy as np
import pytest

import align_ref as R
import attn_ref as A
import prompt_ref as PR
import wq4

pytestmark = pytest.mark.gpu

PREC = {"f16x2": wq4.PREC_F16X2, "f16": wq4.PREC_F16}
H, T = 6, 1500
GUARD = -77


@pytest.fixture(scope="module")
def torch():
    import torch as _t

    assert _t.cuda.is_available()
    return _t


def cu(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# --------------------------------------------------------------------- DTW --
DTW_SHAPES = [(1, 4), (1, 1500), (5, 3), (2, 2), (33, 65), (447, 1500), (447, 4)]


def costs(kind, N, F, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.standard_normal((N, F)).astype(np.float32)
    return rng.integers(-2, 3, (N, F)).astype(np.float32)  # dense ties, exact sums


def run_dtw(torch, xs):
    """xs: the clips' cost matrices, ragged, in one launch -> per clip (jump, trace), the guards checked."""
    import whisper_amd

    B, N_ld, F_ld = len(xs), max(x.shape[0] for x in xs), max(x.shape[1] for x in xs)
    x = np.full((B, N_ld, F_ld), np.nan, np.float32)  # what lies past a clip's N x F must not matter
    for b, c in enumerate(xs):
        x[b, :c.shape[0], :c.shape[1]] = c
    buf = torch.full((B * N_ld + 64,), GUARD, device="cuda", dtype=torch.int32)
    jump, trace = whisper_amd.dtw_check(cu(torch, x), [c.shape[0] for c in xs], [c.shape[1] for c in xs], jump=buf)
    buf = buf.cpu().numpy()
    assert (buf[B * N_ld:] == GUARD).all(), "the guard band after jump_out"
    jump, trace = buf[:B * N_ld].reshape(B, N_ld), trace.cpu().numpy()
    out = []
    for b, c in enumerate(xs):
        N, F = c.shape
        assert (jump[b, N:] == GUARD).all(), "entries past N are not written"
        assert (trace[b, N + 1:] == 255).all() and (trace[b, :, F + 1:] == 255).all(), "trace cells past [N][F]"
        out.append((jump[b, :N], trace[b, :N + 1, :F + 1]))
    return out


@pytest.mark.parametrize("kind", ["normal", "integer"])
@pytest.mark.parametrize("N,F", DTW_SHAPES)
def test_dtw_bit_equal_to_the_f32_restatement(torch, N, F, kind):
    x = costs(kind, N, F, 1000 * N + F)
    (jump, trace), = run_dtw(torch, [x])
    want_jump, want_trace = R.dtw(x)
    assert np.array_equal(trace, want_trace)
    assert np.array_equal(jump, want_jump)


@pytest.mark.parametrize("kind", ["normal", "integer"])
def test_dtw_three_ragged_clips_in_one_launch(torch, kind):
    xs = [costs(kind, N, F, 7 + N) for N, F in ((40, 700), (447, 90), (3, 1500))]
    for (jump, trace), x in zip(run_dtw(torch, xs), xs):
        want_jump, want_trace = R.dtw(x)
        assert np.array_equal(trace, want_trace) and np.array_equal(jump, want_jump)


# ------------------------------------------------------------------ matrix --
# P -> (the clips' positions n_b, their frames F_b, the planted heads)
MATRIX_CASES = {
    "P2": dict(P=2, ns=(2, 2), Fs=(4, 1500), heads=(3,)),
    "P33": dict(P=33, ns=(33, 5, 20), Fs=(4, 7, 65), heads=(0, 1, 2, 4, 5)),
    "P129": dict(P=129, ns=(129, 64, 100), Fs=(64, 750, 1500), heads=(2,)),
    "P448": dict(P=448, ns=(448, 300), Fs=(1500, 750), heads=(5, 3, 1, 0, 2)),
}
_cases: dict = {}


def matrix_inputs(name):
    """(q, k, per-clip heads) of a case, once."""
    if name not in _cases:
        case = R.DIAGONAL_CASE if name == "diagonal" else dict(MATRIX_CASES[name], T=T, H=H, seed=len(name) + MATRIX_CASES[name]["P"])
        _cases[name] = (case, R.matrix_case(**case))
    return _cases[name]


def run_matrix(torch, case, q, k, first_row, prec):
    import whisper_amd

    pad = [case["P"] - n for n in case["ns"]]
    return whisper_amd.align_matrix_check(cu(torch, q), cu(torch, k), case["P"], pad, case["heads"], case["Fs"], first_row,
                                          PREC[prec]).cpu().numpy()


def hold(label, prec, got, ref, bound):
    bad, worst = A.violations(got, ref, bound)
    print(f"ALIGN_WORST {prec} {worst:.3f}  {label}")
    assert not bad.any(), f"{label}: {int(bad.sum())} elements outside the bound, worst error / bound {worst:.3g}"


@pytest.mark.parametrize("prec", A.PRECS)
@pytest.mark.parametrize("name", sorted(MATRIX_CASES))
def test_matrix_planted_within_the_bound(torch, name, prec):
    """Ragged pads, F from 4 to 1500, one head and heads-per-pass + 1 heads, the
    frames past F carrying scores the softmax must not see: every element of M
    within the derived bound, everything outside [N][F] zero."""
    case, (q, k, per_clip) = matrix_inputs(name)
    first_row = 0 if case["P"] == 2 else 2
    got = run_matrix(torch, case, q, k, first_row, prec)
    for b, (n, F) in enumerate(zip(case["ns"], case["Fs"])):
        N = n - 1 - first_row
        ref, bound = R.matrix_ref(per_clip[b], first_row, prec)
        hold(f"{name} clip{b} n{n} F{F} heads{len(case['heads'])}", prec, got[b, :N, :F], ref, bound)
        assert not got[b, N:].any() and not got[b, :, F:].any()


@pytest.mark.parametrize("prec", A.PRECS)
def test_matrix_clip_is_independent_of_the_batch(torch, prec):
    """A padded clip beside others and the same clip alone and unpadded: the same bits."""
    case, (q, k, _) = matrix_inputs("P129")
    P = case["P"]
    got = run_matrix(torch, case, q, k, 2, prec)
    for b, (n, F) in enumerate(zip(case["ns"], case["Fs"])):
        one = dict(case, P=n, ns=(n,), Fs=(F,))
        alone = run_matrix(torch, one, q.reshape(-1, P, 64 * H)[b, P - n:], k[b:b + 1], 2, prec)
        assert np.array_equal(alone[0, :, :], got[b, :n, :]), f"clip {b}"


@pytest.mark.parametrize("prec", A.PRECS)
def test_matrix_identical_rows_are_decided_by_the_zero_std_rule(torch, prec):
    """Two identical positions: every column's std is 0, z = 0 by the rule
    (OpenAI's lines give NaN), so M is exactly 0."""
    case = dict(P=3, ns=(2, 3), Fs=(9, 1500), T=T, H=H, heads=(1, 4), seed=5, kind="identical")
    q, k, per_clip = R.matrix_case(**case)
    got = run_matrix(torch, case, q, k, 0, prec)
    for b in range(2):
        ref, bound = R.matrix_ref(per_clip[b], 0, prec)
        assert not ref.any() and not bound.any()
    assert not got.any() and not np.isnan(got).any()


def test_planted_diagonal_path_equals_the_float64_path(torch):
    """M of the planted diagonal through the DTW kernel: the float64 reference's
    jumps (test_align_ref.py shows that path survives the bound)."""
    case, (q, k, per_clip) = matrix_inputs("diagonal")
    fr = R.DIAGONAL_FIRST_ROW
    got = run_matrix(torch, case, q, k, fr, "f16x2")
    xs = []
    for b, (n, F) in enumerate(zip(case["ns"], case["Fs"])):
        ref, bound = R.matrix_ref(per_clip[b], fr, "f16x2")
        hold(f"diagonal clip{b}", "f16x2", got[b, :n - 1 - fr, :F], ref, bound)
        xs.append(-got[b, :n - 1 - fr, :F])
    for (jump, _), hs in zip(run_dtw(torch, xs), per_clip):
        assert np.array_equal(jump, R.dtw(-R.matrix64(hs, fr), np.float64)[0])


# ------------------------------------------------------------------- model --
SEED = PR.SEED
FIRST_ROW = 3
N_TOKENS = (25, 60, 9)
N_FRAMES = (3000, 1000, 640)
CUSTOM_HEADS = [(1, 5), (0, 2), (1, 0)]


def sequence(n, seed):
    rng = np.random.default_rng(seed)
    return [PR.SOT, PR.LANG, PR.TRANSCRIBE, PR.NO_TIMESTAMPS] + rng.integers(0, 50000, n - 5).tolist() + [PR.EOT]


SEQS = [sequence(n, 40 + n) for n in N_TOKENS]


@pytest.fixture(scope="module")
def gpu_model():
    import whisper_amd

    m = whisper_amd.WhisperModel("tiny_test", SEED, max_batch=17)
    yield m
    m.close()


@pytest.fixture(scope="module")
def mel(torch):
    return torch.from_numpy(PR.mels(3)).cuda()


@pytest.fixture(scope="module")
def runs(gpu_model, mel):
    """Everything the model tests look at, run once: the transcribes before
    the first align, the batch of three, and the transcribes after it."""
    prompts = [s[:4] for s in SEQS]
    out = dict(before=(gpu_model.transcribe(mel, PR.LANG, max_tokens=12),
                       [c["tokens"] for c in gpu_model.transcribe_prompted(mel, prompts, max_tokens=12)]))
    bytes0 = gpu_model.device_bytes()
    out["batch"] = gpu_model.align(mel, SEQS, FIRST_ROW, N_FRAMES, return_matrix=True)
    out["grown"] = gpu_model.device_bytes() - bytes0
    out["after"] = (gpu_model.transcribe(mel, PR.LANG, max_tokens=12),
                    [c["tokens"] for c in gpu_model.transcribe_prompted(mel, prompts, max_tokens=12)])
    return out


@pytest.fixture(scope="module")
def oracle():
    """The float64 oracle's cross-attention operands of the three clips."""
    om = R.AlignOracle("tiny_test", SEED, dtype=np.float64)
    enc = om.encode(PR.mels(3).astype(np.float64))
    return om, [om.align_operands(enc[b:b + 1], SEQS[b]) for b in range(3)]


def oracle_ref(oracle, b, pairs, prec="f16x2"):
    _, ops = oracle
    F = N_FRAMES[b] // 2
    pairs = sorted(pairs, key=lambda p: p[0])
    return R.matrix_ref([(ops[b][l][0][0, h], ops[b][l][1][0, h, :F]) for l, h in pairs], FIRST_ROW, prec)


DEFAULT_HEADS = [(1, h) for h in range(6)]  # tiny_test: 2 layers, the upper half is layer 1


def test_align_matrix_against_the_float64_oracle(runs, oracle):
    """M of every clip of the batch within the bound derived from the oracle's
    own cross-attention operands."""
    for b, clip in enumerate(runs["batch"]):
        ref, bound = oracle_ref(oracle, b, DEFAULT_HEADS)
        got = clip["matrix"].cpu().numpy()
        assert got.shape == ref.shape == (N_TOKENS[b] - 1 - FIRST_ROW, N_FRAMES[b] // 2)
        hold(f"model clip{b}", "f16x2", got, ref, bound)


def test_align_jump_is_the_host_dtw_of_the_gpu_matrix(runs):
    for b, clip in enumerate(runs["batch"]):
        M = clip["matrix"].cpu().numpy()
        assert np.array_equal(clip["jump"], R.dtw(-M)[0]), f"clip {b}"
        assert clip["jump"][0] == 0 and (np.diff(clip["jump"]) >= 0).all()
        assert np.array_equal(clip["start_s"], clip["jump"].astype(np.float32) / np.float32(50.0))
        assert np.array_equal(clip["end_s"], clip["start_s"][1:])


def test_align_jump_equals_the_float64_path_where_the_bound_decides_it(runs, oracle):
    """Where the float64 path survives +- the bound (align_ref.path_is_stable),
    the GPU's jumps are the float64 reference's."""
    decided = 0
    for b, clip in enumerate(runs["batch"]):
        ref, bound = oracle_ref(oracle, b, DEFAULT_HEADS)
        stable = R.path_is_stable(ref, bound)
        print(f"ALIGN_PATH clip{b} stable under the bound: {stable}")
        if stable:
            decided += 1
            assert np.array_equal(clip["jump"], R.dtw(-ref, np.float64)[0]), f"clip {b}"
    print(f"ALIGN_PATH decided clips: {decided} of 3")


def same_clip(a, b):
    assert np.array_equal(a["jump"], b["jump"])
    assert a["matrix"].cpu().numpy().tobytes() == b["matrix"].cpu().numpy().tobytes()


def test_align_clip_is_bit_identical_alone_in_a_batch_and_in_the_second_group(gpu_model, mel, runs):
    """Clip 1 (60 tokens, 1000 frames): alone, inside the batch of three with
    other lengths and n_frames, and at clip 16 of 17 (the second decode group)."""
    alone = gpu_model.align(mel[1:2], [SEQS[1]], FIRST_ROW, N_FRAMES[1], return_matrix=True)
    same_clip(alone[0], runs["batch"][1])
    idx = [0, 2] * 8 + [1]
    seqs = [sequence(6 + 7 * i, 300 + i) for i in range(16)] + [SEQS[1]]
    frames = [8 + 180 * i for i in range(16)] + [N_FRAMES[1]]
    big = gpu_model.align(mel[idx], seqs, FIRST_ROW, frames, return_matrix=True)
    same_clip(big[16], runs["batch"][1])
    assert [len(c["jump"]) for c in big] == [len(s) - 1 - FIRST_ROW for s in seqs]


def test_transcribes_are_unchanged_by_an_align(runs):
    assert runs["after"] == runs["before"]
    assert runs["grown"] > 0  # the first align allocates, and counts, its buffers


def test_custom_heads_over_two_layers_and_back_to_the_default(gpu_model, mel, runs, oracle):
    gpu_model.set_alignment_heads(CUSTOM_HEADS)
    try:
        got = gpu_model.align(mel, SEQS, FIRST_ROW, N_FRAMES, return_matrix=True)
    finally:
        gpu_model.set_alignment_heads([])
    for b, clip in enumerate(got):
        ref, bound = oracle_ref(oracle, b, CUSTOM_HEADS)
        hold(f"model custom heads clip{b}", "f16x2", clip["matrix"].cpu().numpy(), ref, bound)
    again = gpu_model.align(mel[:1], [SEQS[0]], FIRST_ROW, N_FRAMES[0], return_matrix=True)
    same_clip(again[0], runs["batch"][0])
    with pytest.raises(wq4.WQ4Error):
        gpu_model.set_alignment_heads([(2, 0)])
    with pytest.raises(wq4.WQ4Error):
        gpu_model.align(mel[:1], [SEQS[0]], FIRST_ROW, 7)
