"""Child process of test_pipeline_lanes_gpu.py: WA_LANES is read once per
process, so each setting of the knob runs in its own interpreter.  Runs
transcribe_batches over the module's first five 17-clip batches (fixed
length, 24 steps) and prints {"tokens": ..., "pairs": ..., "units3": ...,
"lanes": ...} as one JSON line; "lanes" is what the call allocated, in lanes."""
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

FIRST, NB, B = 500, 5, 17
mel = np.stack([np.stack([wo.synthetic_mel(FIRST + i * B + c, 80) for c in range(B)]) for i in range(NB)])
m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
cfg = m.config
lane = B * (cfg["n_audio_ctx"] * 2 * cfg["n_audio_state"] * 2
            + cfg["n_text_layer"] * 2 * cfg["n_text_ctx"] * cfg["n_text_state"] * 4)
n0 = m.device_bytes()
tok = m.transcribe_batches(torch.from_numpy(mel).cuda(), 50259, max_tokens=24, eot_stop=False)
out = {"tokens": tok, "pairs": m.pipeline_pairs(), "units3": m.pipeline_units3(),
       "lanes": (m.device_bytes() - n0) / lane}
m.close()
print(json.dumps(out))
