"""References for the prompted entries (wa_transcribe_prompted and the
long-form prompt handling), shared by test_prompted.py (CPU) and the GPU tests.

  * long_prompt_window / long_prompt_next: OpenAI transcribe.py's prompt
    handling as include/whisper_amd.h states it, restated in Python.
  * prompted_transcribe: a prompted greedy transcribe composed from the
    unmodified oracle -- SynthWhisper.decoder_pass(tokens, arange(n), cache,
    fresh=True) per clip, then whisper.rs:104-125's step loop.
  * reference(): the fixture of the model tests, computed once per process:
    four synthetic clips under prompts of 4, 5, 37 and 130 tokens and clip 0
    under one of 227, in float32 and in float64.
"""
from __future__ import annotations

import functools

import numpy as np

import whisper_oracle as wo

SEED = 1234
SOT, EOT = 50258, 50257
LANG, TRANSCRIBE, NO_TIMESTAMPS = 50259, 50360, 50364  # tiny_test / Large-V3 (n_lang = 100)
STARTOFPREV = NO_TIMESTAMPS - 2
TS0 = NO_TIMESTAMPS + 1
STEPS = 32
LENGTHS = (4, 5, 37, 130)
LONG = 227


# ------------------------------------------------- the long-form prompt rule --
def long_prompt_window(prev, reset, n_text_ctx, max_tokens, lang=LANG, task=TRANSCRIBE, startofprev=STARTOFPREV):
    """(prompt, k): the last k of prev[reset:], k = min(len, ctx / 2 - 1, ctx - 4 - max_tokens)."""
    tail = list(prev[reset:])
    k = max(0, min(len(tail), n_text_ctx // 2 - 1, n_text_ctx - 4 - max_tokens))
    head = [startofprev] + tail[len(tail) - k:] if k > 0 else []
    return head + [SOT, lang, task], k


def segments(tokens, ts0=TS0):
    """OpenAI's slicing at consecutive timestamp pairs: [(tok_begin, tok_end)]."""
    n = len(tokens)
    if n == 0:
        return []
    is_ts = [t >= ts0 for t in tokens]
    single_end = n >= 2 and not is_ts[n - 2] and is_ts[n - 1]
    cuts = [i for i in range(1, n) if is_ts[i - 1] and is_ts[i]]
    if not cuts:
        return [(0, n)]
    if single_end:
        cuts.append(n)
    out, last = [], 0
    for c in cuts:
        out.append((last, c))
        last = c
    return out


def long_prompt_next(prev, reset, tokens, skipped, temperature, condition, reset_temperature=0.5, ts0=TS0):
    """(prev, reset) after a window: the emitted segments' tokens appended, the
    reset mark moved when conditioning is off or the kept rung ran hot."""
    if skipped:
        return list(prev), reset
    prev = list(prev)
    for a, b in segments(list(tokens), ts0):
        prev += list(tokens[a:b])
    if not condition or temperature > reset_temperature:
        reset = len(prev)
    return prev, reset


# ------------------------------------------------------ prompted transcribe --
def make_prompt(n, seed):
    """n ids: the default prompt (n = 4), or <|startofprev|> + n - 5 text ids + the default prompt."""
    tail = [SOT, LANG, TRANSCRIBE, NO_TIMESTAMPS]
    if n == 4:
        return tail
    rng = np.random.default_rng(seed)
    return [STARTOFPREV] + rng.integers(0, EOT, n - 5).tolist() + tail


def prompted_transcribe(om, enc, prompts, max_tokens=STEPS, eot_stop=True):
    """Per clip: tokens, the prompt's last-position logits, the logit rows the
    picks were taken from (EOT suppressed where whisper.rs suppresses it) and
    the logits at the prompt's last SOT.  enc: the oracle's encoder output [B, T, D]."""
    out = []
    for b, prompt in enumerate(prompts):
        cache = om.init_cache(enc[b:b + 1])
        n = len(prompt)
        logits = om.decoder_pass(np.array([prompt]), np.arange(n), cache, fresh=True)[0]
        first = logits.copy()
        row = logits.copy()
        row[EOT] = -np.inf
        picked = [row]
        nxt = om.argmax_last(row)
        toks, position = [], n
        for step in range(max_tokens):
            if eot_stop and nxt == EOT:
                break
            toks.append(nxt)
            row = om.decoder_pass(np.array([[nxt]]), np.array([position]), cache, fresh=False)[0].copy()
            position += 1
            if step + 1 < wo.MIN_TOKENS:
                row[EOT] = -np.inf
            picked.append(row)
            nxt = om.argmax_last(row)
        sot = max(i for i, t in enumerate(prompt) if t == SOT)
        z0 = om.decoder_pass(np.array([prompt[:sot + 1]]), np.arange(sot + 1), om.init_cache(enc[b:b + 1]), fresh=True)[0]
        out.append({"tokens": toks, "first": first, "picked": picked, "z0": z0})
    return out


def mels(n, n_mels=80, first=0):
    return np.stack([wo.synthetic_mel(first + c, n_mels) for c in range(n)]).astype(np.float32)


def prompts():
    return [make_prompt(n, 100 + n) for n in LENGTHS], make_prompt(LONG, 100 + LONG)


@functools.lru_cache(maxsize=None)
def reference(dtype_name="float32"):
    """{"batch": per-clip results of the four prompts, "long": clip 0 under the 227-token prompt}."""
    om = wo.SynthWhisper("tiny_test", SEED, dtype=np.dtype(dtype_name).type)
    enc = om.encode(mels(len(LENGTHS)).astype(om.dt))
    batch, long = prompts()
    return {"batch": prompted_transcribe(om, enc, batch), "long": prompted_transcribe(om, enc[:1], [long])[0]}
