"""bench.py end to end on the GPU at the tiny_test size: the plain run's
result line and `--dump-outputs`, and what `--full` adds to it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--variant", "tiny_test", "--clips-per-gpu", "3",
        "--max-tokens", "12", "--fixed-length"]
FULL_ONLY = ("roofline", "roofline_q4_gemm", "roofline_cross_attention", "roofline_decode_gemm",
             "roofline_decode_step", "value_sequential", "value_pcie_inclusive", "input_h2d_ms_per_step",
             "cpu_baseline")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + ARGS + list(extra), env=env,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(s) for s in out.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_plain_run_line_and_dump_are_reproducible(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench("--dump-outputs", a)
    _bench("--dump-outputs", b)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "audio-s/wall-s" and line["higher_is_better"] is True and line["dtype"] == "fp16x2"
    # value and ms_per_step are the same measurement: 3 clips x 30 s per step
    assert line["value"] == pytest.approx(3 * 30.0 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["pipeline"]["batches"] == 2  # --steps sets the timed batches
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(a)) == ["n_tokens.npy", "tokens.npy"]
    tok, n = np.load(os.path.join(a, "tokens.npy")), np.load(os.path.join(a, "n_tokens.npy"))
    assert tok.dtype == np.float32 and tok.shape == (3, 12) and n.dtype == np.float32
    assert n.shape == (3,) and np.all((n >= 1) & (n <= 12))
    for i in range(3):  # ids up to the clip's count, -1 padding after it
        k = int(n[i])
        assert np.all(tok[i, :k] >= 0) and np.all(tok[i, :k] == np.round(tok[i, :k])) and np.all(tok[i, k:] == -1)
    for name in ("tokens.npy", "n_tokens.npy"):
        assert np.array_equal(np.load(os.path.join(a, name)), np.load(os.path.join(b, name))), name


def test_full_run_adds_the_other_measurements():
    line = _bench("--full", "--cpu-rows", "8")
    assert line["full"] is True
    assert not [k for k in FULL_ONLY if k not in line]
    assert line["value_sequential"] > 0 and line["cpu_baseline"]["value"] > 0
    assert line["roofline"] in (line["roofline_q4_gemm"], line["roofline_cross_attention"])
