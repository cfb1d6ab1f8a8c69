"""Numpy reference of beam search under the timestamp rules and after caller
prompts (wa_transcribe_beam_ex; include/whisper_amd.h, "Beam search" ->
"Timestamps", "Caller prompts"): beam_ref.BeamRun driven with the rows'
log-probabilities after ts_rules.apply_rules, every row's history being the
tokens sampled along the beam it holds (BeamRun gathers them by parent), and
whisper_oracle.SynthWhisper.decoder_pass underneath.  A helper module, not a
test; beam_ref, ts_rules and prompt_ref are imported, not edited.
"""
from __future__ import annotations

import numpy as np

import beam_ref
import ts_rules as tr

EOT = beam_ref.EOT
NEG = beam_ref.NEG


def rule_f_margin(z_ae, ts0):
    """|logsumexp(z[ts0:]) - max(z[:ts0])| of a row after masks a-e; inf when a side is empty."""
    lse_ts, mt = tr.lse(z_ae[ts0:]), float(np.max(z_ae[:ts0]))
    return abs(lse_ts - mt) if np.isfinite(lse_ts) and np.isfinite(mt) else np.inf


def rows_lp(z_rows, histories, ts0, suppress_eot, max_initial=50):
    """The rows' float32 log-probabilities over the finally masked rows (masks
    a-f of ts_rules from each row's own history), whether rule f fired, and
    each row's rule-f margin on these logits."""
    lp, fired, margin = [], [], []
    for z, s in zip(z_rows, histories):
        z64 = np.asarray(z, np.float64)
        margin.append(rule_f_margin(tr.masks_ae(z64, s, ts0, suppress_eot, max_initial), ts0))
        zz, f, _ = tr.apply_rules(z64, s, ts0, suppress_eot, max_initial)
        lp.append(beam_ref.log_softmax(zz).astype(np.float32))
        fired.append(f)
    return np.stack(lp), fired, margin


class TsBeamRun(beam_ref.BeamRun):
    """BeamRun over raw logit rows: advance_logits masks every row under the
    timestamp rules from the row's history -- self.tokens[clip][beam], which
    BeamRun reindexes by parent -- before the plain advance.  margin_f[clip]:
    the smallest rule-f margin of a live row (finite S) before the clip
    completed."""

    def __init__(self, n_clips, K, C, ts0, max_initial=50, eot_stop=True):
        super().__init__(n_clips, K, C)
        self.ts0, self.max_initial, self.eot_stop = ts0, max_initial, eot_stop
        self.margin_f = [np.inf] * n_clips

    def histories(self):
        return [self.tokens[c][j] for c in range(self.n) for j in range(self.K)]

    def advance_logits(self, z_rows):
        pick = self.picks
        suppress = pick == 0 or pick < 3 or not self.eot_stop  # pick s + 1 of step s: EOT masked while s + 1 < 3
        lp, _, mf = rows_lp(z_rows, self.histories(), self.ts0, suppress, self.max_initial)
        for r, m in enumerate(mf):
            c, j = divmod(r, self.K)
            if not self.complete[c] and self.S[c][j] > NEG:
                self.margin_f[c] = min(self.margin_f[c], m)
        return self.advance(lp)


def default_prompt(model, lang_token, timestamps):
    """The fixed prompt of wa_transcribe_beam / wa_transcribe_timestamps with an explicit language."""
    tr_tok = 50260 + model.cfg["n_lang"]
    return [50258, lang_token, tr_tok] + ([] if timestamps else [tr_tok + 4])


def oracle_beam_ex(model, mel, K, C, lang_token=50259, max_tokens=12, eot_stop=True, timestamps=True, max_initial=50,
                   prompts=None, length_penalty=None, enc=None):
    """wa_transcribe_beam_ex over the numpy oracle, clip by clip (a clip does
    not depend on its neighbours): the prompt once (the fixed one, auto-detect
    with the runtime's position quirk, or the caller's through one
    decoder_pass), its caches repeated over the K rows, then decode steps whose
    self-attention caches are gathered by parent.  Returns (per clip
    BeamRun.result() entries with "margin_f" added, max |finite logit a pick
    saw|, finished sequences)."""
    import whisper_oracle as wo

    c = model.cfg
    enc = model.encode(mel) if enc is None else enc
    tr_tok = 50260 + c["n_lang"]
    ts0 = tr_tok + 5
    out, amax, n_fin = [], 0.0, 0
    for b in range(mel.shape[0]):
        cache = model.init_cache(enc[b:b + 1])
        if prompts is not None:
            p = list(prompts[b])
            logits = model.decoder_pass(np.array([p]), np.arange(len(p)), cache, fresh=True)
            position = len(p)
        elif lang_token is not None:
            p = default_prompt(model, lang_token, timestamps)
            logits = model.decoder_pass(np.array([p]), np.arange(len(p)), cache, fresh=True)
            position = len(p)
        else:
            z0 = model.decoder_pass(np.full((1, 1), wo.SOT), np.arange(1), cache, fresh=True)
            lo, hi = 50259, 50259 + c["n_lang"]
            lg = lo + model.argmax_last(z0[0, lo:hi])
            p = [lg, tr_tok] + ([] if timestamps else [tr_tok + 4])
            logits = model.decoder_pass(np.array([p]), np.arange(len(p)), cache, fresh=True)
            position = 1 + len(p)
        for L in cache:
            for k in ("k", "v", "ck", "cv"):
                L[k] = np.repeat(L[k], K, axis=0)
        logits = np.repeat(logits, K, axis=0)
        run = TsBeamRun(1, K, C, ts0, max_initial, eot_stop) if timestamps else beam_ref.BeamRun(1, K, C)
        for pick in range(max_tokens):
            z = logits.astype(np.float64)
            if timestamps:
                seen = np.stack([tr.masks_ae(r, s, ts0, pick < wo.MIN_TOKENS or not eot_stop, max_initial)
                                 for r, s in zip(z, run.histories())])
                amax = max(amax, float(np.abs(seen[np.isfinite(seen)]).max()))
                nxt, par = run.advance_logits(z)
            else:
                if pick < wo.MIN_TOKENS or not eot_stop:
                    z[:, EOT] = -np.inf
                amax = max(amax, float(np.abs(z[np.isfinite(z)]).max()))
                nxt, par = run.advance(np.stack([beam_ref.log_softmax(r) for r in z]).astype(np.float32))
            if pick + 1 == max_tokens or (eot_stop and run.all_complete()):
                break
            for L in cache:  # OpenAI's rearrange_kv_cache
                L["k"], L["v"] = L["k"][par], L["v"][par]
            logits = model.decoder_pass(nxt[:, None], np.array([position]), cache, fresh=False)
            position += 1
        res = run.result(length_penalty)[0]
        res["margin_f"] = run.margin_f[0] if timestamps else np.inf
        out.append(res)
        n_fin += len(run.finished[0])
    return out, amax, n_fin
