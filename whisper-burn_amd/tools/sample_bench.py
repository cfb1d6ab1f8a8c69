"""Cost of temperature sampling: wa_transcribe_sampled at T = 0 and at T = 0.6
against wa_transcribe_scored on the same model and clips, fixed-length decode,
so every form runs the same number of steps.

  python whisper-burn_amd/tools/sample_bench.py [--variant large_v3] [--clips 32]
      [--max-tokens 224] [--runs 3] [--temperature 0.6] [--json-out FILE]

Per run the forms alternate, in an order that reverses from run to run, each
after one warm-up call that captures its step graphs; reported: wall ms per
call, the prompt and decode phases (wa_last_timings) and the ratios of their
means to the scored form's.  The T = 0 form runs the sampled kernel without
evaluating noise (the cost of the wider reduction alone); at T > 0 every
thread also hashes its 16 ids and takes two logarithms each, and the tokens
differ from the greedy ones, so the forms decode different sequences of the
same length: the step cost is what is compared.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--max-tokens", type=int, default=224)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import whisper_amd

    m = whisper_amd.WhisperModel(args.variant, args.seed, max_batch=args.clips)
    n_mels = m.config["n_mels"]
    arr = np.stack([whisper_amd.synth_uniform(0x5EED0000 + c, "mel", n_mels * 3000, -1.5, 1.0)
                    for c in range(args.clips)])
    mel = torch.from_numpy(arr.reshape(args.clips, n_mels, 3000)).cuda()
    seeds = np.arange(args.clips, dtype=np.uint64) + np.uint64(args.seed)
    hot = f"sampled_T{args.temperature:g}"

    def sampled(T):
        return lambda: [c["tokens"] for c in
                        m.transcribe_sampled(mel, T, seeds, 50259, args.max_tokens, eot_stop=False)]

    forms = {
        "scored": lambda: [c["tokens"] for c in m.transcribe_scored(mel, 50259, args.max_tokens, eot_stop=False)],
        "sampled_T0": sampled(0.0),
        hot: sampled(args.temperature),
    }
    tokens = {k: f() for k, f in forms.items()}  # warm-up: graphs captured, buffers allocated
    assert tokens["scored"] == tokens["sampled_T0"]
    picks = args.clips * args.max_tokens
    off_greedy = sum(a != b for ca, cb in zip(tokens[hot], tokens["scored"]) for a, b in zip(ca, cb))
    runs = []
    for r in range(args.runs):
        order = list(forms) if r % 2 == 0 else list(forms)[::-1]
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            forms[name]()
            torch.cuda.synchronize()
            t = m.last_timings()
            runs.append({"form": name, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                         "decode_ms": round(t["decode_ms"], 3), "prompt_ms": round(t["prompt_ms"], 3),
                         "steps": t["steps"]})
    mean = lambda form, key: float(np.mean([x[key] for x in runs if x["form"] == form]))
    out = {"what": "wa_transcribe_sampled at T = 0 and T > 0 against wa_transcribe_scored, fixed-length decode, "
                   "forms interleaved in alternating order",
           "variant": args.variant, "clips": args.clips, "max_tokens": args.max_tokens,
           "temperature": args.temperature, "picks": int(picks), "picks_off_the_scored_token": int(off_greedy),
           "runs": runs}
    for key in ("wall_ms", "decode_ms", "prompt_ms"):
        out[key + "_mean"] = {f: round(mean(f, key), 3) for f in forms}
        out[key + "_ratio_to_scored"] = {f: round(mean(f, key) / mean("scored", key), 5) for f in forms}
    out["decode_us_per_step"] = {f: round(mean(f, "decode_ms") / args.max_tokens * 1e3, 2) for f in forms}
    s = json.dumps(out)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
