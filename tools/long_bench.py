"""Long-form transcription throughput: WhisperModel.transcribe_long over many
synthetic recordings of mixed lengths, and the cost of its two mel kernels.

    python tools/long_bench.py [--variant large_v3] [--recordings 40] [--max-batch 32]
        [--min-minutes 1] [--max-minutes 10] [--max-tokens 224] [--json-out profiles/long_form.json]

Recorded, not gated:
  audio_s_per_wall_s   seconds of audio per wall second of one transcribe_long call
                       (after a warm-up call on a short prefix of every recording)
  rounds, mean_fill    the scheduling rule's rounds and their mean batch fill B / max_batch
  mel_stream_max       ms of long_mel_max over all recordings, and per recording-hour
  mel_window           ms of one long_mel_windows launch of max_batch windows (a full round)
  graph_key_changes    decode-step graph keys that changed from one round to the next while
                       the loop is composed from the public pieces (a new B captures step
                       graphs unless a kept graph serves it), and the distinct B seen

The thresholds are off by default (one rung per round): synthetic weights score
every window far below OpenAI's -1.0, so the ladder would run every rung on
every round and the figure would measure the rung count.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "whisper-burn_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))


def event_ms(torch, fn, reps: int) -> float:
    fn()  # allocates on first use
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="large_v3", choices=["large_v3", "medium", "tiny_test"])
    ap.add_argument("--recordings", type=int, default=40)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--min-minutes", type=float, default=1.0)
    ap.add_argument("--max-minutes", type=float, default=10.0)
    ap.add_argument("--max-tokens", type=int, default=224)
    ap.add_argument("--temperatures", default="0,0.2,0.4,0.6,0.8,1")
    ap.add_argument("--logprob-threshold", type=float, default=None)
    ap.add_argument("--no-speech-threshold", type=float, default=None)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--json-out", default=os.path.join(HERE, "..", "profiles", "long_form.json"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import mel_oracle as mo
    import whisper_amd as wa

    S, mb = args.recordings, args.max_batch
    ladder = tuple(float(t) for t in args.temperatures.split(","))
    rng = np.random.default_rng(args.seed)
    n = (rng.uniform(args.min_minutes, args.max_minutes, S) * 60 * 16000).astype(np.int64)
    # one minute of speech-like audio per voice, tiled to each recording's length
    voices = mo.synthetic_audio(8, 60 * 16000, seed=args.seed)
    audio = [torch.from_numpy(np.tile(voices[r % 8], int(n[r]) // voices.shape[1] + 1)[: int(n[r])]).cuda()
             for r in range(S)]
    off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    buf = torch.cat(audio)
    seeds = np.arange(S, dtype=np.uint64) + np.uint64(args.seed)
    hours = float(n.sum()) / 16000 / 3600

    m = wa.WhisperModel(args.variant, args.seed, max_batch=mb)
    n_mels = m.config["n_mels"]
    kw = dict(seed=seeds, temperatures=ladder, logprob_threshold=args.logprob_threshold,
              no_speech_threshold=args.no_speech_threshold, max_tokens=args.max_tokens)

    # the mel kernels on their own
    max_dev = wa.long_mel_max(buf, off, n, n_mels)
    t_max = event_ms(torch, lambda: wa.long_mel_max(buf, off, n, n_mels, out=max_dev), 3)
    pick = np.arange(mb) % S
    seek0 = [int(n[r]) // 160 // 2 for r in pick]
    win = wa.long_mel_windows(buf, off[pick], n[pick], seek0, pick, max_dev, n_mels)
    t_win = event_ms(torch, lambda: wa.long_mel_windows(buf, off[pick], n[pick], seek0, pick, max_dev, n_mels,
                                                        out=win), 10)

    # warm-up: one window of every recording (buffers, the full-batch step graphs)
    m.transcribe_long(audio, max_windows=1, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = m.transcribe_long(audio, **kw)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    timings = m.last_timings()

    # the rounds, replayed from the recorded advances by the scheduling rule
    C = [int(x) // 160 for x in n]
    seek, w, fills = [0] * S, [0] * S, []
    while True:
        rec = wa.long_round(C, seek, w, mb, 1 << 20)
        if not rec:
            break
        fills.append(len(rec))
        for r in rec:
            seek[r] += res[r]["windows"][w[r]]["advance"]
            w[r] += 1
    assert w == [len(x["windows"]) for x in res]

    # the same rounds composed from the public pieces, watching the step-graph keys
    groups = 2
    keys = [m.decode_graph_key(g) for g in range(groups)]
    changes, seek, w = 0, [0] * S, [0] * S
    for B in fills:
        rec = wa.long_round(C, seek, w, mb, 1 << 20)
        mel = wa.long_mel_windows(buf, off[rec], n[rec], [seek[r] for r in rec], rec, max_dev, n_mels)
        m.transcribe_fallback(mel, np.array([int(seeds[r]) + 8 * w[r] for r in rec], np.uint64), ladder,
                              args.logprob_threshold, args.no_speech_threshold, 50259, max_tokens=args.max_tokens,
                              timestamps=True)
        now = [m.decode_graph_key(g) for g in range(groups)]
        changes += sum(a != b for a, b in zip(keys, now))
        keys = now
        for r in rec:
            seek[r] += res[r]["windows"][w[r]]["advance"]
            w[r] += 1

    windows = [x for r in res for x in r["windows"]]
    out = {
        "what": "transcribe_long over synthetic recordings of mixed lengths; thresholds "
                + ("off (one rung per round)" if args.logprob_threshold is None else "on"),
        "variant": args.variant, "weights": m.weights, "recordings": S, "max_batch": mb,
        "minutes": [round(float(x) / 16000 / 60, 2) for x in n], "audio_hours": round(hours, 4),
        "max_tokens": args.max_tokens, "temperatures": ladder, "logprob_threshold": args.logprob_threshold,
        "no_speech_threshold": args.no_speech_threshold,
        "wall_s": round(wall, 3), "audio_s_per_wall_s": round(hours * 3600 / wall, 1),
        "windows": len(windows), "segments": sum(len(r["segments"]) for r in res),
        "skipped": sum(x["skipped"] for x in windows),
        "mean_advance_frames": round(float(np.mean([x["advance"] for x in windows])), 1),
        "rounds": len(fills), "batch_sizes": fills, "mean_fill": round(float(np.mean(fills)) / mb, 4),
        "phase_ms_summed": {k: round(float(v), 1) for k, v in timings.items()},
        "mel_stream_max_ms": round(t_max, 3), "mel_stream_max_ms_per_recording_hour": round(t_max / hours, 3),
        "mel_window_ms_per_round": round(t_win, 3), "mel_window_clips": mb,
        "graph_key_changes": changes, "distinct_batch_sizes": len(set(fills)),
    }
    s = json.dumps(out)
    print(s, flush=True)
    if args.json_out:
        with open(args.json_out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
