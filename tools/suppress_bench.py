"""Cost of the suppress-token lists in the decode step: Large-V3 Q4_0 synthetic,
32 clips, 224 tokens, fixed-length decode (eot_stop = 0), decode ms per step, in
three forms --
  a  the parent commit (a built checkout of it: --parent-tree),
  b  this tree with no list set (the kernels of a list-free model),
  c  this tree with an 88-id `always` list (82 text ids spread over the
     vocabulary plus SOT, TRANSLATE, TRANSCRIBE, <|startoflm|>, <|startofprev|>,
     <|nospeech|>) and first = [220, EOT]
-- for the greedy decode (wa_transcribe), the timestamp decode
(wa_transcribe_timestamps) and a 6 x 5 beam call (wa_transcribe_beam).

  python tools/suppress_bench.py --parent-tree DIR [--procs 3] [--runs 3]
      [--json-out profiles/suppress_overhead.json]

Every form runs in --procs fresh processes, the forms interleaved (a, b, c, a,
...); a process builds the model, warms each mode up once (buffers, step
graphs) and times --runs calls per mode (wa_last_timings: device events).  A
process's figure is the mean of its calls.  b runs the same kernels as a, so
its figures must fall inside or overlap a's range; c is reported against a.

  python tools/suppress_bench.py --worker --tree DIR --list none|set
is one such process (prints one JSON line).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT = 50257
MODES = ("greedy", "timestamps", "beam")


def lists(n_lang: int):
    tr = 50260 + n_lang  # TRANSCRIBE
    specials = [50258, tr - 1, tr, tr + 1, tr + 2, tr + 3]
    text = sorted({int(round(i * (EOT - 1) / 81)) for i in range(82)})
    return text + specials, [220, EOT]


def worker(args) -> None:
    sys.path.insert(0, os.path.join(args.tree, "whisper-burn_amd"))
    import numpy as np
    import torch

    import whisper_amd

    m = whisper_amd.WhisperModel(args.variant, args.seed, max_batch=args.clips)
    n_mels = m.config["n_mels"]
    arr = np.stack([whisper_amd.synth_uniform(0x5EED0000 + c, "mel", n_mels * 3000, -1.5, 1.0)
                    for c in range(args.clips)])
    mel = torch.from_numpy(arr.reshape(args.clips, n_mels, 3000)).cuda()
    n_always = n_first = 0
    if args.list == "set":
        always, first = lists(m.config["n_lang"])
        m.set_suppress_tokens(always, first)
        n_always, n_first = len(always), len(first)
    K, C = args.beam, args.beam_clips
    forms = {
        "greedy": lambda: m.transcribe(mel, 50259, args.max_tokens, eot_stop=False),
        "timestamps": lambda: m.transcribe_timestamps(mel, 50259, args.max_tokens, eot_stop=False),
        "beam": lambda: m.transcribe_beam(mel[:C], K, 1.0, None, 50259, args.max_tokens, False),
    }
    out = {"list": args.list, "n_always": n_always, "n_first": n_first,
           "range_tier": None, "modes": {}}
    for name in MODES:
        forms[name]()  # warm-up: buffers and step graphs
    for _ in range(args.runs):
        for name in MODES:
            torch.cuda.synchronize()
            forms[name]()
            torch.cuda.synchronize()
            t = m.last_timings()
            out["modes"].setdefault(name, []).append({"decode_ms": round(t["decode_ms"], 3), "steps": t["steps"]})
    out["range_tier"] = m.range_tier
    for name in MODES:
        r = out["modes"][name]
        out["modes"][name] = {"runs": r, "ms_per_step": round(sum(x["decode_ms"] for x in r) /
                                                             max(1, sum(x["steps"] for x in r)), 5)}
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--list", default="none", choices=["none", "set"])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--beam-clips", type=int, default=6)
    ap.add_argument("--max-tokens", type=int, default=224)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_tree:
        ap.error("--parent-tree: a built checkout of the parent commit")
    forms = {"a": (args.parent_tree, "none"), "b": (REPO, "none"), "c": (REPO, "set")}
    procs = {f: [] for f in forms}
    for _ in range(args.procs):
        for f, (tree, lst) in forms.items():  # a fresh process each, the forms interleaved
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--list", lst, "--variant",
                   args.variant, "--clips", str(args.clips), "--beam", str(args.beam), "--beam-clips",
                   str(args.beam_clips), "--max-tokens", str(args.max_tokens), "--runs", str(args.runs), "--seed",
                   str(args.seed)]
            res = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
            procs[f].append(json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]))
            print(f"form {f}: " + ", ".join(f"{k} {v['ms_per_step']}" for k, v in procs[f][-1]["modes"].items()),
                  file=sys.stderr, flush=True)
    out = {"what": "decode ms per step of the parent commit (a), this tree without lists (b) and with an 88-id "
                   "`always` list and first = [220, EOT] (c); fresh processes, forms interleaved",
           "variant": args.variant, "clips": args.clips, "beam": [args.beam_clips, args.beam],
           "max_tokens": args.max_tokens, "runs_per_process": args.runs, "processes": procs, "summary": {}}
    for mode in MODES:
        v = {f: [p["modes"][mode]["ms_per_step"] for p in procs[f]] for f in forms}
        a_lo, a_hi = min(v["a"]), max(v["a"])
        out["summary"][mode] = {
            "ms_per_step": v,
            "a_range": [a_lo, a_hi],
            "a_spread": round(a_hi - a_lo, 5),
            "b_overlaps_a": bool(min(v["b"]) <= a_hi and max(v["b"]) >= a_lo),
            "c_max_over_a_max": round(max(v["c"]) - a_hi, 5),
            "c_mean_over_a_mean_pct": round(100.0 * (sum(v["c"]) / len(v["c"]) / (sum(v["a"]) / len(v["a"])) - 1.0), 3),
            "c_beyond_a_spread": bool(max(v["c"]) - a_hi > a_hi - a_lo),
        }
    s = json.dumps(out, indent=1)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
