"""Child process of test_pipeline_pairs_gpu.py: WA_PAIR_BATCHES is read once
per process, so the knob's off setting runs in its own interpreter.  Runs
transcribe_batches over the module's first four 16-clip batches (fixed
length, 24 steps) and prints {"tokens": ..., "pairs": ...} as one JSON line."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "oracle"), os.path.join(REPO, "whisper-burn_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import whisper_amd  # noqa: E402
import whisper_oracle as wo  # noqa: E402

FIRST, NB, B = 300, 4, 16
mel = np.stack([np.stack([wo.synthetic_mel(FIRST + i * B + c, 80) for c in range(B)]) for i in range(NB)])
m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
tok = m.transcribe_batches(torch.from_numpy(mel).cuda(), 50259, max_tokens=24, eot_stop=False)
out = {"tokens": tok, "pairs": m.pipeline_pairs()}
m.close()
print(json.dumps(out))
