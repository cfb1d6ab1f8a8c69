"""Register, scratch and LDS budgets of the decode chain's fit forms, read
from the built libraries' kernel metadata (no GPU).

Two 512-thread workgroups share a CU only if each wave needs at most 128
registers (4 waves per SIMD of a 512-entry file), spills nothing and two
workgroups' LDS fits the CU's 160 KB.  The gfx950 code objects are cut out of
the libraries' .hip_fatbin sections (clang offload bundles) and their
NT_AMDGPU_METADATA notes printed by llvm-readelf --notes of the ROCm LLVM;
only .vgpr_count, .private_segment_fixed_size and .group_segment_fixed_size
are read, never instructions.  Skipped when llvm-readelf is absent.
"""
from __future__ import annotations

import os
import re
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "..", "whisper-burn_amd", "lib")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _readelf():
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    for r in roots:
        for sub in ("lib/llvm/bin", "llvm/bin"):
            p = os.path.join(r or "", sub, "llvm-readelf")
            if r and os.path.isfile(p) and os.access(p, os.X_OK):
                return p
    return shutil.which("llvm-readelf")


def _code_objects(path):
    """The gfx950 code objects of every offload bundle in the file."""
    data = open(path, "rb").read()
    out, at = [], data.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, at + len(MAGIC))
    return out


def _kernels(tmp_path, lib):
    """{kernel symbol: {field: int}} of one library."""
    tool = _readelf()
    if tool is None:
        pytest.skip("llvm-readelf of the ROCm LLVM not found")
    path = os.path.join(LIBDIR, lib)
    assert os.path.isfile(path), f"{lib} is not built"
    objs = _code_objects(path)
    assert objs, f"no gfx950 code object in {lib}"
    meta = {}
    for i, blob in enumerate(objs):
        f = tmp_path / f"{lib}.{i}.co"
        f.write_bytes(blob)
        txt = subprocess.run([tool, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        # one YAML map per kernel under amdhsa.kernels: fields in alphabetical order, .name among them
        for block in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            block = ".agpr_count:" + block
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            vals = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", block)}
            meta[name.group(1)] = vals
    return meta


def _check(meta, pattern, expect, dynamic_lds=0):
    """dynamic_lds: what the launcher adds to the metadata's static LDS."""
    rx = re.compile(pattern)
    hits = {k: v for k, v in meta.items() if rx.search(k)}
    assert len(hits) == expect, (pattern, sorted(hits))
    for k, v in hits.items():
        assert v["vgpr_count"] <= 128, (k, v)
        assert v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] + dynamic_lds <= 80 * 1024, (k, v, dynamic_lds)


def test_gemm_fit_forms_fit_two_per_cu(tmp_path):
    """q4_gemm_decode_kernel<2, EPI, PER, 1, 8, Q4, false, FIT = true>: EPI
    f32 / tiled / head-major, PER 2 and 3.  Its LDS is dynamic: the metadata
    holds none, the launcher's size comes from the library itself
    (wq4_diag_decode_lds_bytes, the launcher's own decode_lds_bytes(8))."""
    import ctypes

    meta = _kernels(tmp_path, "libwq4.so")
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libwq4.so"))
    lib.wq4_diag_decode_lds_bytes.restype = ctypes.c_size_t
    lib.wq4_diag_decode_lds_bytes.argtypes = [ctypes.c_int]
    dyn = int(lib.wq4_diag_decode_lds_bytes(8))
    assert dyn >= 8 * 16 * 64 * 4, dyn  # at least the eight waves' reduction tiles
    _check(meta, r"q4_gemm_decode_kernelILi2ELi[012]ELi[23]ELi1ELi8ELi0ELb0ELb1EEE", 6, dynamic_lds=dyn)


def test_xattn_out_fit_forms_fit_two_per_cu(tmp_path):
    """xattn_out_kernel<NS, Q4, 4, SM, MTG, FIT = true>: NS 1 and 2, SM 5, 6
    and 8, MTG 1 and 4."""
    meta = _kernels(tmp_path, "libwhisper_amd.so")
    _check(meta, r"xattn_out_kernelILi[12]ELi0ELi4ELi[568]ELi[14]ELb1EEE", 12)
