"""Every output of the token pick on fixed seeded inputs, for a bit-for-bit
comparison of two builds of the libraries (a refactor of the pick against its
parent commit).

  WQ4_LIB_DIR=<build A> python whisper-burn_amd/tools/pick_bits.py --out a.npz
  WQ4_LIB_DIR=<build B> python whisper-burn_amd/tools/pick_bits.py --out b.npz
  python whisper-burn_amd/tools/pick_bits.py --compare a.npz b.npz [--json-out FILE]

One run per build, each in a fresh process; --compare needs no GPU and asks
that both files hold the same arrays, byte for byte (NaN payloads included).

The kernel cases drive the wa_*_check entry points at the smallest shapes at
which the reduction can go wrong, plus the real vocabulary: D = 128, both
precisions, B in {1, 17, 32}, steps 0 and 5 (EOT suppressed / not), and
  V = 300, ts0 = 200     3 workgroups (fewer than the 8 reduction parts), a
                         padded tail, ts0 inside a workgroup (it holds both sides)
  V = 300, ts0 = 256     ts0 on a workgroup boundary (no workgroup holds both)
  V = 1100, ts0 = 1000   9 workgroups: the parts hold uneven counts
  V = 51866, ts0 = 50365 the real vocabulary
Five embedding rows are one vector, so their logits tie exactly at the row
maximum: inside a workgroup (5, 77), across workgroups (133) and across ts0
(ts0 - 1, ts0 + 3; ts0 + 9 ties inside the timestamps).  The rule records cover
the first pick and all four (last, penult) states, so whole sides are masked;
temperatures 0, 0.2, 1 with distinct seeds.  All five fused forms, the row
kernels with and without records at pick 0 (EOT suppressed) and pick 6, and
the timestamp bookkeeping.  The returned masked logits are kept whole up to
V = 1100 and as a SHA-256 digest at the real vocabulary.

The model cases run every transcribe form of `tiny_test` at 3 clips, at 66
clips (two groups of 33 rows: the stored-row picks) and one pipelined sampled
call of that width.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

D = 128
GRID = [(300, 200), (300, 256), (1100, 1000), (51866, 50365)]
TEMPS = (0.0, 0.2, 1.0)
TEXT = 7


def histories(ts0):
    t = lambda k: ts0 + k
    return [[], [t(10), TEXT], [t(10), TEXT, t(20)], [t(10), TEXT, t(20), t(20)], [TEXT]]


def tie_ids(ts0):
    return [5, 77, 133, ts0 - 1, ts0 + 3, ts0 + 9]


def inputs(V, ts0):
    rng = np.random.default_rng(9000 + V + ts0)
    emb = (rng.uniform(-1, 1, (V, D)) * 0.03).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((D, 32)))
    hid = (q.T * 16.0).astype(np.float32)
    emb[tie_ids(ts0)] = (q.T.sum(axis=0) * (2.0 / 16.0)).astype(np.float32)
    rows = rng.standard_normal((32, V)).astype(np.float32)
    rows[:, tie_ids(ts0)] = 4.5
    return hid, emb, rows


def keep(out, key, t, V=0):
    a = np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t))
    if V > 1100 and a.size >= V:
        a = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
    assert key not in out, key
    out[key] = a


def kernel_cases(out):
    import torch

    import whisper_amd as wa
    import wq4

    for V, ts0 in GRID:
        hid_h, emb_h, rows_h = inputs(V, ts0)
        emb = torch.from_numpy(emb_h).cuda()
        hist = [histories(ts0)[r % 5] for r in range(32)]
        temps = np.array([TEMPS[r % 3] for r in range(32)], np.float32)
        seeds = np.arange(32, dtype=np.uint64) * np.uint64(977) + np.uint64(V)
        for prec in (wq4.PREC_F16X2, wq4.PREC_F16):
            for B in (1, 17, 32):
                hid = torch.from_numpy(hid_h[:B]).cuda()
                for step in (0, 5):
                    tag = f"V{V}_ts{ts0}_p{prec}_B{B}_s{step}"
                    tok, lg = wa.logits_argmax_check(hid, emb, step, prec)
                    keep(out, f"plain/{tag}/tok", tok)
                    keep(out, f"plain/{tag}/logits", lg, V)
                    tok, lp, lg = wa.logits_logprob_check(hid, emb, step, prec)
                    keep(out, f"scored/{tag}/tok", tok)
                    keep(out, f"scored/{tag}/lp", lp)
                    keep(out, f"scored/{tag}/logits", lg, V)
                    tok, lp, lg, mass = wa.logits_timestamp_check(hid, emb, hist[:B], step, ts0, precision=prec)
                    keep(out, f"ts/{tag}/tok", tok)
                    keep(out, f"ts/{tag}/lp", lp)
                    keep(out, f"ts/{tag}/mass", mass)
                    keep(out, f"ts/{tag}/logits", lg, V)
                    for name, h in (("sampled", None), ("sampled_ts", hist[:B])):
                        tok, lp, lg, mass = wa.logits_sample_check(hid, emb, temps[:B], seeds[:B], step, h, ts0,
                                                                   precision=prec)
                        keep(out, f"{name}/{tag}/tok", tok)
                        keep(out, f"{name}/{tag}/lp", lp)
                        keep(out, f"{name}/{tag}/logits", lg, V)
                        if mass is not None:
                            keep(out, f"{name}/{tag}/mass", mass)
        # the row kernels: pick 0 with EOT suppressed, pick 6 without
        rows = torch.from_numpy(rows_h).cuda()
        idx = torch.from_numpy(rows_h.argmax(axis=1).astype(np.int32)).cuda()
        for pick, sup in ((0, True), (6, False)):
            tag = f"V{V}_ts{ts0}_pick{pick}"
            keep(out, f"row_logprob/{tag}", wa.row_logprob_check(rows, 0, V, sup, idx))
            keep(out, f"row_logprob_fixed/{tag}", wa.row_logprob_check(rows, 3, V - 2, sup, None, TEXT))
            for k, a in zip(("tok", "lp", "mass"), wa.row_timestamp_check(rows, hist, ts0, sup)):
                keep(out, f"row_ts/{tag}/{k}", a)
            for name, h in (("row_sample", None), ("row_sample_ts", hist)):
                for k, a in zip(("tok", "lp", "mass"), wa.row_sample_check(rows, temps, seeds, pick, sup, h, ts0)):
                    keep(out, f"{name}/{tag}/{k}", a)
        rng = np.random.default_rng(V + ts0)
        seq = np.where(rng.random((40, 12)) < 0.4, rng.integers(ts0, V, (40, 12)), rng.integers(0, ts0, (40, 12)))
        keep(out, f"bookkeep/V{V}_ts{ts0}", wa.timestamp_bookkeep_check(seq.astype(np.int32), ts0, V))


def keep_clips(out, key, clips):
    n = max(len(c["tokens"]) for c in clips)
    toks = np.full((len(clips), n + 1), -1, np.int32)
    for i, c in enumerate(clips):
        toks[i, :len(c["tokens"])] = c["tokens"]
    keep(out, key + "/tokens", toks)
    if "logprob_slots" not in clips[0]:  # a plain transcribe: tokens only
        return
    keep(out, key + "/logprob_slots", np.stack([c["logprob_slots"] for c in clips]))
    for k in ("no_speech_prob", "lang_prob", "avg_logprob"):
        keep(out, f"{key}/{k}", np.array([c[k] for c in clips], np.float32))
    keep(out, key + "/lang_token", np.array([c["lang_token"] for c in clips], np.int32))
    if "segments" in clips[0]:
        segs = [[i, s, e, len(t)] for i, c in enumerate(clips) for s, e, t in c["segments"]]
        keep(out, key + "/segments", np.array(segs, np.float32).reshape(-1, 4))
        keep(out, key + "/seek_frames", np.array([c["seek_frames"] for c in clips], np.int32))
    if "rung" in clips[0]:
        keep(out, key + "/rung", np.array([c["rung"] for c in clips], np.int32))


def model_cases(out):
    import torch

    import whisper_amd as wa

    wide = 66
    m = wa.WhisperModel("tiny_test", 1234, max_batch=wide)
    n_mels = m.config["n_mels"]
    arr = np.stack([wa.synth_uniform(0x51C50000 + c, "mel", n_mels * 3000, -1.5, 1.0) for c in range(2 * wide)])
    mel = torch.from_numpy(arr.reshape(2, wide, n_mels, 3000)).cuda()
    assert wa.decode_group_rows(wide) > 32 >= wa.decode_group_rows(3)
    for name, B, n in (("3", 3, 12), ("wide", wide, 6)):
        x = mel[0, :B].contiguous()
        temps = np.array([(0.0, 0.5, 1.0)[c % 3] for c in range(B)], np.float32)
        seeds = np.arange(B, dtype=np.uint64) * np.uint64(131) + np.uint64(9)
        keep_clips(out, f"model{name}/plain", [dict(tokens=t) for t in m.transcribe(x, 50259, n)])
        keep_clips(out, f"model{name}/plain_auto", [dict(tokens=t) for t in m.transcribe(x, None, n)])
        keep_clips(out, f"model{name}/scored", m.transcribe_scored(x, 50259, n))
        keep_clips(out, f"model{name}/scored_auto", m.transcribe_scored(x, None, n))
        keep_clips(out, f"model{name}/ts", m.transcribe_timestamps(x, 50259, n))
        keep_clips(out, f"model{name}/sampled", m.transcribe_sampled(x, temps, seeds, 50259, n))
        keep_clips(out, f"model{name}/sampled_ts", m.transcribe_sampled(x, temps, seeds, 50259, n, timestamps=True))
        keep_clips(out, f"model{name}/fallback", m.transcribe_fallback(x, seeds, (0.0, 0.5, 1.0), -0.5, None, 50259, n))
    temps = np.array([(0.0, 0.5, 1.0)[c % 3] for c in range(2 * wide)], np.float32).reshape(2, wide)
    seeds = (np.arange(2 * wide, dtype=np.uint64) * np.uint64(131) + np.uint64(9)).reshape(2, wide)
    for i, b in enumerate(m.transcribe_batches_sampled(mel, temps, seeds, 50259, 6, timestamps=True)):
        keep_clips(out, f"modelwide/pipelined_sampled_ts/{i}", b)
    m.close()


def compare(a_path, b_path, json_out):
    a, b = np.load(a_path), np.load(b_path)
    differing = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            differing.append(k)
    groups = sorted({k.split("/")[0] for k in a.files})
    res = {"what": "pick_bits.py --compare: every array of both builds' outputs, byte for byte",
           "a": os.path.basename(a_path), "b": os.path.basename(b_path), "arrays": len(a.files),
           "cases": {g: sum(k.startswith(g + "/") for k in a.files) for g in groups},
           "result": "equal" if not differing else "different", "differing": differing[:50]}
    s = json.dumps(res)
    print(s)
    if json_out:
        with open(json_out, "w") as fh:
            fh.write(s + "\n")
    sys.exit(0 if not differing else 1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare, args.json_out)
    out = {}
    kernel_cases(out)
    model_cases(out)
    np.savez(args.out, **out)
    print(json.dumps({"wrote": args.out, "arrays": len(out)}))


if __name__ == "__main__":
    main()
