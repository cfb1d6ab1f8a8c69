"""The ctypes table of whisper_amd/_ffi.py against the two C headers (no GPU).

A ctypes declaration that disagrees with its prototype hands the library a
stray pointer; on a GPU that is a fault, here it is a failed count."""
from __future__ import annotations

import glob
import os
import re

import pytest

import whisper_amd
from whisper_amd import _ffi

# the per-mode check entries the unified ones replaced
DELETED = ("wa_logits_argmax_check", "wa_logits_logprob_check", "wa_logits_timestamp_check", "wa_logits_sample_check",
           "wa_logits_suppress_check", "wa_row_timestamp_check", "wa_row_sample_check", "wa_row_suppress_check",
           "wa_beam_topk_rules_check", "wa_beam_topk_suppress_check", "wa_beam_select_rules_check",
           "wa_self_attention_pad_check", "wa_self_attention_beam_check", "wa_self_attention_beam_pad_check",
           "wa_embed_pad_check")


def prototypes() -> dict:
    """name -> parameter count of every wa_* prototype of the two headers."""
    out = {}
    for path in (whisper_amd.HEADER_PATH, whisper_amd.CHECKS_HEADER_PATH):
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        for name, args in re.findall(r"\b(wa_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
            assert name not in out, name
            args = args.strip()
            out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_table_and_headers_name_the_same_functions():
    protos, (argtypes, restype) = prototypes(), _ffi._table()
    assert len(protos) >= 90
    assert sorted(argtypes) == sorted(protos)
    assert set(restype) <= set(argtypes)


@pytest.mark.parametrize("name", sorted(prototypes()))
def test_argument_count_matches_the_prototype(name):
    assert len(_ffi._table()[0][name]) == prototypes()[name]


def test_non_int_results_are_declared():
    """Every prototype that does not return wq4_status / int has a restype in the table."""
    text = "".join(re.sub(r"/\*.*?\*/", "", open(p).read(), flags=re.S)
                   for p in (whisper_amd.HEADER_PATH, whisper_amd.CHECKS_HEADER_PATH))
    other = {n for t, n in re.findall(r"^([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)(wa_[a-z0-9_]+)\s*\(", text, flags=re.M)
             if t.strip() not in ("wq4_status", "int")}
    assert other == set(_ffi._table()[1])


def test_deleted_entries_are_gone():
    L = whisper_amd.lib()
    assert not [n for n in DELETED if hasattr(L, n)]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = [f for pat in ("whisper-burn_amd/**/*", "include/*") for f in glob.glob(os.path.join(repo, pat), recursive=True)
             if os.path.isfile(f) and os.path.splitext(f)[1] in (".py", ".h", ".hpp", ".cpp", ".hip", "")]
    assert len(files) > 40
    named = [(os.path.relpath(f, repo), n) for f in files for n in DELETED if n in open(f, errors="replace").read()]
    assert not named, named
