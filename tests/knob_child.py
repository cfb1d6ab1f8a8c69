"""Child process of test_tuning_knobs_gpu.py: the environment knobs are read
once per process (static initialisers), so every setting runs in its own
interpreter.  Prints the greedy tokens of 16 synthetic tiny_test clips as
one JSON line.

With a GGUF path as its argument (test_range_guard.py) it loads that model
with max_batch=2 instead, transcribes the range-guard module's two mels
(24 steps, EOT ignored) and prints {"tokens": ..., "range_tier": ...}."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "whisper-burn_amd"),
                os.path.join(REPO, "whisper-burn_amd", "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import whisper_amd  # noqa: E402
import whisper_oracle as wo  # noqa: E402

if len(sys.argv) > 1:
    m = whisper_amd.WhisperModel.from_gguf(sys.argv[1], "tiny_test", max_batch=2)
    mel = np.stack([wo.synthetic_mel(c, m.config["n_mels"]) for c in (0, 1)])
    tok = m.transcribe(torch.from_numpy(mel).cuda(), 50259, 24, eot_stop=False)
    out = {"tokens": tok, "range_tier": m.range_tier}
    m.close()
    print(json.dumps(out))
    sys.exit(0)

mel = np.stack([wo.synthetic_mel(20 + c, 80) for c in range(16)]).astype(np.float32)
m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=16)
tok = m.transcribe(torch.from_numpy(mel).cuda(), 50259, max_tokens=24)
m.close()
print(json.dumps(tok))
