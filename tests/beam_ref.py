"""Numpy reference of the beam search of wa_transcribe_beam (include/
whisper_amd.h, "Beam search"): the per-row top-(K + 1), one merge step, finalize
and rank, and a driver that runs a whole beam decode around a function giving
the rows' log-probabilities -- over random tables (test_beam_ref.py) or over
whisper_oracle.SynthWhisper.decoder_pass with the per-beam caches gathered
physically, as OpenAI's rearrange_kv_cache does.

Scores are float32 and every score is one float32 addition S[j] + lp, as on
the device, so a merge step is comparable bit for bit.
"""
from __future__ import annotations

import numpy as np

EOT = 50257
NEG = np.float32(-np.inf)


def log_softmax(z):
    """float64 log-softmax of one row (-inf entries stay -inf)."""
    z = np.asarray(z, np.float64)
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))


def topk_row(lp, kp):
    """The kp largest entries of a row: larger value first, equal values: larger
    id first.  Returns (ids int32 [kp], values in lp's dtype [kp])."""
    lp = np.asarray(lp)
    ids = np.arange(lp.size)
    order = np.lexsort((-ids, -lp.astype(np.float64)))[:kp]
    return order.astype(np.int32), lp[order]


def select(S, top_tok, top_lp, K, C, fin_n, complete, eot=EOT):
    """One merge step of one clip.  S float32 [K]; top_tok / top_lp [K][K + 1].
    Returns a dict: next_tok, parent (source beam), S (new, float32) [K] -- a
    beam no candidate fills is (0, itself, -inf) --, filed: [(source beam, sum)]
    newly finished sequences in list order (none when the clip is complete),
    fin_n and complete afterwards, order: the walked candidates [(score, j, i,
    tok)] up to the K-th non-EOT one, and behind: the first one after them."""
    cands = []
    for j in range(K):
        for i in range(K + 1):
            s = np.float32(np.float32(S[j]) + np.float32(top_lp[j][i]))
            if s > NEG:
                cands.append((s, j, i, int(top_tok[j][i])))
    cands.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
    next_tok, parent, S_new = [0] * K, list(range(K)), [NEG] * K
    filed, n_live, n_met, walked, behind = [], 0, 0, [], None
    for c in cands:
        if n_live == K:
            behind = c  # the first candidate behind the walk (margins only)
            break
        walked.append(c)
        s, j, _, tok = c
        if tok == eot:
            n_met += 1
            if not complete and fin_n + len(filed) < C:
                filed.append((j, s))
        else:
            next_tok[n_live], parent[n_live], S_new[n_live] = tok, j, s
            n_live += 1
    if not complete:
        fin_n = min(C, fin_n + n_met)
        complete = fin_n >= C
    return {"next_tok": next_tok, "parent": parent, "S": np.asarray(S_new, np.float32), "filed": filed,
            "fin_n": fin_n, "complete": bool(complete), "order": walked, "behind": behind, "n_kept": n_live}


def finalize(finished, live_tokens, live_S, K):
    """finished: [(tokens, sum)]; a list shorter than K gets live beams (finite
    S), S descending then beam index ascending, until it has K."""
    out = list(finished)
    order = sorted((j for j in range(len(live_S)) if live_S[j] > NEG), key=lambda j: (-float(live_S[j]), j))
    for j in order:
        if len(out) >= K:
            break
        out.append((list(live_tokens[j]), np.float32(live_S[j])))
    return out


def rank_scores(sums, lens, length_penalty=None):
    lens = np.maximum(np.asarray(lens, np.float64), 1.0)
    sums = np.asarray(sums, np.float32).astype(np.float64)
    if length_penalty is None or np.isnan(length_penalty):
        return sums / lens
    return sums / ((5.0 + lens) / 6.0) ** float(length_penalty)


def rank(sums, lens, length_penalty=None):
    """The best candidate: the largest score, the first among equals."""
    return int(np.argmax(rank_scores(sums, lens, length_penalty)))


def step_margin(sel, K, C, fin_before, complete_before):
    """The smallest score gap of one merge step whose flip would change the
    kept set or the finished list: the K-th kept candidate against the first
    one behind the walk, an EOT candidate inside the walk against the K-th
    kept one, and -- when the list overflows -- EOT candidates against each
    other."""
    inside, behind = sel["order"], sel["behind"]
    if sel["n_kept"] < K:
        return np.inf  # every candidate was walked: nothing to flip
    last = float(inside[-1][0])
    m = np.inf
    if behind is not None:
        m = min(m, last - float(behind[0]))
    eots = [float(c[0]) for c in inside if c[3] == EOT]
    if eots and not complete_before:
        m = min(m, min(eots) - last)
        if fin_before + len(eots) > C:
            m = min([m] + [a - b for a, b in zip(eots, eots[1:])])
    return m


class BeamRun:
    """A beam decode of n_clips clips over rows clip * K + beam.  advance(lp)
    takes the rows' masked log-probabilities [rows][V] (pick 0 first) and
    returns (next tokens [rows], parent rows [rows]); result() finalizes."""

    def __init__(self, n_clips, K, C, eot=EOT):
        self.n, self.K, self.C, self.eot = n_clips, K, C, eot
        self.S = np.full((n_clips, K), NEG, np.float32)
        self.S[:, 0] = 0.0
        self.tokens = [[[] for _ in range(K)] for _ in range(n_clips)]
        self.finished = [[] for _ in range(n_clips)]
        self.complete = [False] * n_clips
        self.margin = [np.inf] * n_clips  # over the steps before the clip completed
        self.picks = 0

    def advance(self, lp):
        K, nxt, par = self.K, [], []
        for c in range(self.n):
            pairs = [topk_row(np.asarray(lp[c * K + j], np.float32), K + 1) for j in range(K)]
            before = (len(self.finished[c]), self.complete[c])
            sel = select(self.S[c], [p[0] for p in pairs], [p[1] for p in pairs], K, self.C, before[0], before[1],
                         self.eot)
            if not before[1]:
                self.margin[c] = min(self.margin[c], step_margin(sel, K, self.C, *before))
            for j, s in sel["filed"]:
                self.finished[c].append((list(self.tokens[c][j]), s))
            self.tokens[c] = [self.tokens[c][sel["parent"][b]] + [sel["next_tok"][b]] for b in range(K)]
            self.S[c] = sel["S"]
            self.complete[c] = sel["complete"]
            nxt += sel["next_tok"]
            par += [c * K + p for p in sel["parent"]]
        self.picks += 1
        return np.asarray(nxt), np.asarray(par)

    def all_complete(self):
        return all(self.complete)

    def result(self, length_penalty=None):
        """Per clip: candidates [(tokens, sum)] in list order, the best index,
        and the final margins: of the live beams finalize cuts between and of
        the rank's winner over the runner-up."""
        out = []
        for c in range(self.n):
            cands = finalize(self.finished[c], self.tokens[c], self.S[c], self.K)
            sc = rank_scores([s for _, s in cands], [len(t) for t, _ in cands], length_penalty)
            m = self.margin[c]
            nf = len(self.finished[c])
            if 0 < nf < self.K:  # finalize takes the K - nf best live beams
                live = sorted((float(s) for s in self.S[c] if s > NEG), reverse=True)
                if len(live) > self.K - nf:
                    m = min(m, live[self.K - nf - 1] - live[self.K - nf])
            if len(sc) > 1:
                top = np.sort(sc)[::-1]
                m = min(m, float(top[0] - top[1]))
            out.append({"candidates": cands, "best": int(np.argmax(sc)), "margin": m})
        return out


def oracle_beam(model, mel, K, C, lang_token=50259, max_tokens=12, eot_stop=True, length_penalty=None, enc=None):
    """wa_transcribe_beam over the numpy oracle: the prompt on every row, then
    decode steps whose per-beam self-attention caches are gathered by parent.
    Returns (BeamRun.result(), max |finite picked logit|, finished sequences)."""
    import whisper_oracle as wo

    c = model.cfg
    n = mel.shape[0]
    enc = model.encode(mel) if enc is None else enc
    cache = model.init_cache(np.repeat(enc, K, axis=0))
    rows = n * K
    tr = 50260 + c["n_lang"]
    if lang_token is not None:
        prompt = np.array([[wo.SOT, lang_token, tr, tr + 4]] * rows)
        logits = model.decoder_pass(prompt, np.arange(4), cache, fresh=True)
        position = 4
    else:
        logits = model.decoder_pass(np.full((rows, 1), wo.SOT), np.arange(1), cache, fresh=True)
        lo, hi = 50259, 50259 + c["n_lang"]
        langs = [lo + model.argmax_last(logits[b, lo:hi]) for b in range(rows)]
        prompt = np.array([[lg, tr, tr + 4] for lg in langs])
        logits = model.decoder_pass(prompt, np.arange(3), cache, fresh=True)
        position = 4
    run = BeamRun(n, K, C)
    amax = 0.0
    for pick in range(max_tokens):
        z = logits.astype(np.float64)
        if pick == 0 or pick < wo.MIN_TOKENS or not eot_stop:  # pick s + 1 of step s: EOT masked while s + 1 < 3
            z[:, EOT] = -np.inf
        amax = max(amax, float(np.abs(z[np.isfinite(z)]).max()))
        lp = np.stack([log_softmax(r) for r in z]).astype(np.float32)
        nxt, par = run.advance(lp)
        if pick + 1 == max_tokens or (eot_stop and run.all_complete()):
            break
        for L in cache:  # OpenAI's rearrange_kv_cache: the rows' caches follow their parents
            L["k"], L["v"] = L["k"][par], L["v"][par]
        logits = model.decoder_pass(nxt[:, None], np.array([position]), cache, fresh=False)
        position += 1
    return run.result(length_penalty), amax, sum(len(f) for f in run.finished)
