"""Cost of beam search: wa_transcribe_beam at 6 clips x beam_size 5 (30 rows)
against wa_transcribe at 30 clips and at 6 clips, Large-V3 Q4_0, fixed-length
decode (eot_stop = 0), same model, same process.

  python tools/beam_bench.py [--variant large_v3] [--clips 6] [--beam 5]
      [--max-tokens 224] [--runs 3] [--only beam] [--kernel-stats CSV]
      [--timestamps] [--prompt-len N]
      [--bench-parent JSON --bench-new JSON] [--json-out profiles/beam_overhead.json]

Per run the forms alternate (beam, greedy at clips * beam clips, greedy at
`clips` clips), each after one warm-up call that allocates its buffers and
captures its step graph; reported per form: wall ms per call, the decode phase
(wa_last_timings: device events) and ms per step.  The 30-clip greedy call is
two 15-row decode groups on two streams (the product's layout for a sequential
call of 30 clips); the beam call is one 30-row group.

--timestamps: the beam form under the timestamp rules (wa_transcribe_beam_ex).
--prompt-len N: the beam form after a caller prompt of N tokens per clip
  (<|startofprev|>, text, then the default prompt; N = 223 with 224 tokens
  fills the context).
--only beam: the beam form alone (the run to put under
  rocprofv3 --kernel-trace --stats -- python tools/beam_bench.py --only beam --runs 1).
--kernel-stats CSV: that run's *_kernel_stats.csv; the three beam kernels' rows
  are added to the result, with the bytes beam_topk moves against its time.
--bench-parent / --bench-new: files holding the JSON lines of `python bench.py`
  runs of the parent build and of this one, recorded as they are.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper-burn_amd"))

BEAM_KERNELS = ("beam_topk_kernel", "beam_topk_rules_kernel", "beam_select_kernel", "dec_self_attn_beam_kernel")


def kernel_rows(path: str) -> dict:
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in BEAM_KERNELS:
                if k in name:
                    out[k] = {"calls": int(float(row["Calls"])),
                              "avg_us": round(float(row["AverageNs"]) / 1e3, 3),
                              "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3),
                              "percent": round(float(row["Percentage"]), 3)}
    return out


def bench_lines(path: str) -> list:
    with open(path) as fh:
        lines = [json.loads(ln) for ln in fh if ln.startswith("{")]
    return [{"rtf": ln["value"], "ms_per_step": ln.get("ms_per_step")} for ln in lines]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--clips", type=int, default=6)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--max-tokens", type=int, default=224)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--only", default=None, choices=["beam"])
    ap.add_argument("--timestamps", action="store_true")
    ap.add_argument("--prompt-len", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--bench-parent", default=None)
    ap.add_argument("--bench-new", default=None)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import whisper_amd

    rows = args.clips * args.beam
    m = whisper_amd.WhisperModel(args.variant, args.seed, max_batch=rows)
    n_mels, V = m.config["n_mels"], m.config["n_vocab"]
    arr = np.stack([whisper_amd.synth_uniform(0x5EED0000 + c, "mel", n_mels * 3000, -1.5, 1.0) for c in range(rows)])
    mel = torch.from_numpy(arr.reshape(rows, n_mels, 3000)).cuda()
    prompts = None
    if args.prompt_len:
        tr = 50260 + m.config["n_lang"]
        tail = [50258, 50259, tr] + ([] if args.timestamps else [tr + 4])
        n_text = args.prompt_len - len(tail) - 1
        assert n_text >= 0, "--prompt-len is too short for <|startofprev|> and the default prompt"
        rng = np.random.default_rng(args.seed)
        prompts = [[tr + 2] + rng.integers(0, 50257, n_text).tolist() + tail for _ in range(args.clips)]
    forms = {"beam": lambda: m.transcribe_beam(mel[:args.clips], args.beam, 1.0, None, 50259, args.max_tokens, False,
                                               timestamps=args.timestamps, prompts=prompts)}
    if args.only is None:
        forms[f"greedy{rows}"] = lambda: m.transcribe(mel, 50259, args.max_tokens, eot_stop=False)
        forms[f"greedy{args.clips}"] = lambda: m.transcribe(mel[:args.clips], 50259, args.max_tokens, eot_stop=False)
    bytes0 = m.device_bytes()
    forms["beam"]()  # warm-up: buffers and step graphs
    beam_bytes = int(m.device_bytes() - bytes0)  # the beam buffers and the score buffers of the SOT scores
    for name, f in forms.items():
        if name != "beam":
            f()
    runs = []
    for _ in range(args.runs):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t = m.last_timings()
            runs.append({"form": name, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                         "encoder_ms": round(t["encoder_ms"], 3), "prompt_ms": round(t["prompt_ms"], 3),
                         "decode_ms": round(t["decode_ms"], 3), "steps": t["steps"]})
    mean = lambda form, key: float(np.mean([r[key] for r in runs if r["form"] == form]))
    out = {"what": "wa_transcribe_beam (clips x beam rows, one decode group) against wa_transcribe at as many clips "
                   "as rows and at `clips` clips; fixed-length decode, forms interleaved",
           "variant": args.variant, "clips": args.clips, "beam_size": args.beam, "rows": rows,
           "max_tokens": args.max_tokens, "timestamps": args.timestamps, "prompt_len": args.prompt_len, "range_tier": m.range_tier, "beam_device_bytes": beam_bytes, "runs": runs}
    for key in ("wall_ms", "decode_ms"):
        out[key + "_mean"] = {f: round(mean(f, key), 3) for f in forms}
    out["ms_per_step"] = {f: round(mean(f, "decode_ms") / max(1.0, mean(f, "steps")), 4) for f in forms}
    if args.only is None:
        out["beam_over_greedy_rows_decode"] = round(mean("beam", "decode_ms") / mean(f"greedy{rows}", "decode_ms"), 4)
        out["beam_over_greedy_clips_decode"] = round(mean("beam", "decode_ms") / mean(f"greedy{args.clips}",
                                                                                    "decode_ms"), 4)
    if args.kernel_stats:
        ks = kernel_rows(args.kernel_stats)
        out["kernels"] = ks
        topk = "beam_topk_rules_kernel" if args.timestamps else "beam_topk_kernel"
        if topk in ks:
            nbytes = rows * V * 4  # the rules form reads the row twice; the second walk comes from L2
            out["beam_topk_bytes"] = nbytes
            out["beam_topk_gb_per_s"] = round(nbytes / (ks[topk]["avg_us"] * 1e-6) / 1e9, 1)
    if args.bench_parent and args.bench_new:
        out["bench_py"] = {"parent": bench_lines(args.bench_parent), "new": bench_lines(args.bench_new)}
    s = json.dumps(out)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
