"""Cost of caller prompts: wa_transcribe_prompted at prompt lengths 4, 64 and 227
against wa_transcribe (the fixed 4-token prompt through the Tq <= 4 path) on
the same model and clips, fixed-length decode.

  python whisper-burn_amd/tools/prompt_bench.py [--variant large_v3] [--clips 32]
      [--max-tokens 64] [--runs 3] [--json-out profiles/prompted_overhead.json]

Per run the forms alternate (plain, P = 4, 64, 227), each after one warm-up
call that captures its step graphs and allocates its buffers; reported per
form: wall ms per call, the prompt phase and the decode phase (wa_last_timings:
device events) and the decode us per step.  Every clip of a prompted form has
the same length, so P is also the group's.  The condition the prefill kernels
have to meet: the 227-token prefill costs less than ceil(227 / 4) = 57 times
the plain form's 4-token prompt -- the existing path run in 4-token chunks is
the cheapest alternative.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

LENGTHS = (4, 64, 227)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--max-tokens", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import whisper_amd

    m = whisper_amd.WhisperModel(args.variant, args.seed, max_batch=args.clips)
    n_mels, n_lang = m.config["n_mels"], m.config["n_lang"]
    arr = np.stack([whisper_amd.synth_uniform(0x5EED0000 + c, "mel", n_mels * 3000, -1.5, 1.0)
                    for c in range(args.clips)])
    mel = torch.from_numpy(arr.reshape(args.clips, n_mels, 3000)).cuda()
    transcribe, no_ts = 50260 + n_lang, 50260 + n_lang + 4
    tail = [50258, 50259, transcribe, no_ts]
    rng = np.random.default_rng(args.seed)

    def prompts(P):  # <|startofprev|> + text ids + the default prompt
        return [tail if P == 4 else [no_ts - 2] + rng.integers(0, 50257, P - 5).tolist() + tail
                for _ in range(args.clips)]

    forms = {"plain": lambda: m.transcribe(mel, 50259, args.max_tokens, eot_stop=False)}
    for P in LENGTHS:
        forms[f"P{P}"] = (lambda pr: lambda: [c["tokens"] for c in m.transcribe_prompted(
            mel, pr, args.max_tokens, eot_stop=False)])(prompts(P))
    bytes0 = m.device_bytes()
    tokens = {k: f() for k, f in forms.items()}  # warm-up
    assert tokens["P4"] == tokens["plain"], "the default prompt through the prefill gives other tokens"
    runs = []
    for _ in range(args.runs):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t = m.last_timings()
            runs.append({"form": name, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                         "prompt_ms": round(t["prompt_ms"], 3), "decode_ms": round(t["decode_ms"], 3),
                         "steps": t["steps"]})
    mean = lambda form, key: float(np.mean([r[key] for r in runs if r["form"] == form]))
    out = {"what": "wa_transcribe_prompted at P = 4, 64, 227 against wa_transcribe, fixed-length decode, forms interleaved",
           "variant": args.variant, "clips": args.clips, "max_tokens": args.max_tokens,
           "prefill_device_bytes": int(m.device_bytes() - bytes0), "runs": runs}
    for key in ("wall_ms", "prompt_ms", "decode_ms"):
        out[key + "_mean"] = {f: round(mean(f, key), 3) for f in forms}
    out["decode_us_per_step"] = {f: round(mean(f, "decode_ms") / args.max_tokens * 1e3, 2) for f in forms}
    chunks = -(-LENGTHS[-1] // 4)
    out["chunked_alternative_ms"] = round(chunks * mean("plain", "prompt_ms"), 3)  # 57 x the 4-token prompt
    out["prefill_227_ms"] = round(mean(f"P{LENGTHS[-1]}", "prompt_ms"), 3)
    out["prefill_beats_chunks"] = bool(out["prefill_227_ms"] < out["chunked_alternative_ms"])
    s = json.dumps(out)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
