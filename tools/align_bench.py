"""Cost of token alignment: wa_align on Large-V3 Q4_0 at 32 clips for id
sequences of 64 and 224 tokens, with the default alignment heads (every head of
the upper half of the layers) and with a 10-head set, beside the prompt phase
of wa_transcribe_prompted at the same length (the prefill without the capture).

  python tools/align_bench.py [--variant large_v3] [--clips 32] [--runs 3]
      [--json-out profiles/align_overhead.json] [--parent-tree DIR]

Per run the forms alternate, each after one warm-up call; reported per form:
wall ms per call and wa_last_align_timings' device-event parts (encoder,
prefill with the capture, DTW, total), or wa_last_timings' prompt phase for the
prompted forms; capture_ms = the align form's prefill less the prompted form's
prompt phase at the same length (the weights + filter kernels; the align
prefill stops after the last layer with alignment heads and skips the logits,
so with few heads it can come out negative).

--parent-tree DIR (a checkout of the parent commit with its libraries built):
first runs `python bench.py --steps 2 --warmup 1` of that tree and of this one,
interleaved, twice each, and reports whether the token dumps are identical and
whether this build's RTF lies inside the parent's own spread.  Prints one JSON
line.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "whisper-burn_amd"))

LENGTHS = (64, 224)
# ten (layer, head) pairs spread over the decoder (valid for Large-V3: 32 layers, 20 heads)
TEN_HEADS = [(7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4), (24, 1), (25, 6)]


def bench_ab(parent_tree: str) -> dict:
    """The parent tree's bench.py and this tree's, interleaved, twice each."""
    import numpy as np

    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(2):
            for build in ("parent", "new"):
                env = dict(os.environ)
                env.pop("WQ4_LIB_DIR", None)
                root = os.path.abspath(parent_tree) if build == "parent" else REPO
                dump = os.path.join(tmp, f"{build}{i}")
                run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1",
                                      "--dump-outputs", dump], env=env, cwd=root, capture_output=True, text=True)
                if run.returncode != 0:
                    raise RuntimeError(f"{build} bench.py failed: {run.stderr[-2000:]}")
                out = run.stdout
                line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
                runs.append({"build": build, "rtf": line["value"],
                             "tokens": np.load(os.path.join(dump, "tokens.npy")).tobytes().hex()})
    parent = [r["rtf"] for r in runs if r["build"] == "parent"]
    new = [r["rtf"] for r in runs if r["build"] == "new"]
    return {"rtf_parent": parent, "rtf_new": new, "tokens_identical": len({r["tokens"] for r in runs}) == 1,
            "new_inside_parent_spread": bool(max(new) >= min(parent))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import whisper_amd

    bench = bench_ab(args.parent_tree) if args.parent_tree else None  # before this process holds a model
    m = whisper_amd.WhisperModel(args.variant, args.seed, max_batch=args.clips)
    n_mels, n_lang = m.config["n_mels"], m.config["n_lang"]
    arr = np.stack([whisper_amd.synth_uniform(0x5EED0000 + c, "mel", n_mels * 3000, -1.5, 1.0)
                    for c in range(args.clips)])
    mel = torch.from_numpy(arr.reshape(args.clips, n_mels, 3000)).cuda()
    transcribe, no_ts = 50260 + n_lang, 50260 + n_lang + 4
    rng = np.random.default_rng(args.seed)
    ten = [p for p in TEN_HEADS if p[0] < m.config["n_text_layer"] and p[1] < m.config["n_text_head"]]

    def sequences(n):
        return [[50258, 50259, transcribe, no_ts] + rng.integers(0, 50257, n - 5).tolist() + [50257]
                for _ in range(args.clips)]

    def align_form(seqs, heads):
        def run():
            m.set_alignment_heads(heads)
            m.align(mel, seqs, 3, 3000)
            return m.align_timings()
        return run

    def prompt_form(seqs):
        def run():
            m.transcribe_prompted(mel, seqs, max_tokens=1, eot_stop=False)
            t = m.last_timings()
            return {"encoder_ms": t["encoder_ms"] + t["cross_kv_ms"], "prefill_ms": t["prompt_ms"]}
        return run

    forms = {}
    for n in LENGTHS:
        seqs = sequences(n)
        forms[f"align_n{n}_default"] = align_form(seqs, [])
        forms[f"align_n{n}_ten"] = align_form(seqs, ten)
        forms[f"prompted_P{n - 1}"] = prompt_form([s[:-1] for s in seqs])  # P + the one decoded token <= n_text_ctx
    bytes0 = m.device_bytes()
    for f in forms.values():  # warm-up: buffers, step graphs
        f()
    runs = []
    for _ in range(args.runs):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts = f()
            torch.cuda.synchronize()
            runs.append(dict({"form": name, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3)},
                             **{k: round(v, 3) for k, v in parts.items()}))
    m.set_alignment_heads([])
    mean = lambda form, key: round(float(np.mean([r[key] for r in runs if r["form"] == form])), 3)
    out = {"what": "wa_align against the prompt phase of wa_transcribe_prompted, forms interleaved",
           "variant": args.variant, "clips": args.clips, "heads_per_pass": 4, "ten_heads": ten,
           "align_device_bytes": int(m.device_bytes() - bytes0), "runs": runs, "mean": {}}
    for name in forms:
        keys = [k for k in runs[0] if k != "form"] if name.startswith("align") else ["wall_ms", "encoder_ms", "prefill_ms"]
        out["mean"][name] = {k: mean(name, k) for k in keys if any(k in r for r in runs if r["form"] == name)}
    for n in LENGTHS:
        for hs in ("default", "ten"):
            out["mean"][f"align_n{n}_{hs}"]["capture_ms"] = round(
                out["mean"][f"align_n{n}_{hs}"]["prefill_ms"] - out["mean"][f"prompted_P{n - 1}"]["prefill_ms"], 3)
    if bench is not None:
        out["bench"] = bench
    s = json.dumps(out)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
