"""Child process of test_xattn_plan_gpu.py (a model and pipeline of its own,
like tests/pairs_child.py): two and three 16-clip batches of the small test
model through transcribe_batches with the cross-attention's frame split
forced to 5 and to 7 (WA_XATTN_SPLITS_RT), against one transcribe per batch
under the default plan; after every paired call a plain transcribe without
the override must be back on the default plan (the graph key's split digit).
Prints one JSON line."""
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

ENV = "WA_XATTN_SPLITS_RT"
FIRST, NB, B, STEPS = 300, 3, 16, 12


def splits(m):
    return [m.decode_graph_key(g) // (whisper_amd.XATTN_SHARE_DEN + 1) % 16 for g in (0, 1)]


mel = np.stack([np.stack([wo.synthetic_mel(FIRST + i * B + c, 80) for c in range(B)]) for i in range(NB)])
x = torch.from_numpy(mel).cuda()
m = whisper_amd.WhisperModel("tiny_test", 1234, max_batch=B)
os.environ.pop(ENV, None)
seq = [m.transcribe(x[i], 50259, max_tokens=STEPS, eot_stop=False) for i in range(NB)]
out = {"sequential_splits": splits(m), "runs": []}
for nb in (2, 3):
    for forced in (5, 7):
        os.environ[ENV] = str(forced)
        tok = m.transcribe_batches(x[:nb], 50259, max_tokens=STEPS, eot_stop=False)
        run = {"batches": nb, "forced": forced, "pairs": m.pipeline_pairs(), "splits": splits(m),
               "equal": tok == seq[:nb]}
        del os.environ[ENV]
        plain = m.transcribe(x[0], 50259, max_tokens=STEPS, eot_stop=False)
        run["plain_after_splits"] = splits(m)
        run["plain_after_equal"] = plain == seq[0]
        out["runs"].append(run)
m.close()
print(json.dumps(out))
