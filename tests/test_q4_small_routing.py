"""CPU tests behind the Q4 GEMM tests at 128 rows and below
(test_q4_small_gpu.py): the launch plans of the decode and decode-step kernels
(wq4_gemm_plan, host code) against the rules restated in literal numbers in
q4_small_shapes.py, the covering shape table, and which plans exist at all.
No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import q4_small_shapes as S
import wq4


@pytest.fixture(autouse=True)
def _reset_modes():
    yield
    wq4.set_precision(wq4.PREC_F16X2)
    wq4.set_kernel_policy(0)


def _dec_key(p):
    return p["per"], p["ks"]


def _sk_key(p):
    return p["ks"], p["nt"], p["row_tiles"]


def test_small_shape_table_is_a_covering_set():
    """Every (K, rows) and every (K, N) pair of each kernel at least once;
    every epilogue variant and both precisions per kernel; f16 weights on at
    least one case of every ks of each kernel; the A-tiled output only where
    N % 32 == 0; K % 64 == 32 at least twice; nothing larger than the
    1312 x 12288 weight; the decode-step kernel's (272, 5376, 17) and
    (528, 5376, 17) are in the table."""
    for cases, ks_, rows_, ns_ in ((S.DEC_CASES, S.DEC_KS, S.DEC_ROWS, S.DEC_NS), (S.SK_CASES, S.SK_KS, S.SK_ROWS, S.SK_NS)):
        assert {(k, r) for _, r, _, k, *_ in cases} == {(k, r) for k in ks_ for r in rows_}
        assert {(k, n) for _, _, n, k, *_ in cases} == {(k, n) for k in ks_ for n in ns_}
        assert {(f, ip) for *_, f, ip, _, _ in cases} >= set(S.VARIANTS) | {(3, True)}
        for prec in (S.PREC_F16X2, S.PREC_F16):
            assert {f for c, *_, f, _, p, _ in S.CASES if p == prec and c == cases[0][0]} >= {0, 1, 2, 4}
    assert len(S.DEC_CASES) == 160 and len(S.SK_CASES) == 54 and len(S.CASES) <= 230
    assert all(n % 32 == 0 for _, _, n, _, f, *_ in S.CASES if f & 4)
    assert all(f & 2 for *_, f, ip, _, _ in S.CASES if ip)
    assert sum(k % 64 == 32 for k in S.DEC_KS) >= 2 and {1568, 3104} <= set(S.DEC_KS)
    assert max(n * k for _, _, n, k, *_ in S.CASES) == 1312 * 12288
    assert {(17, 272, 5376), (17, 528, 5376)} <= {(r, n, k) for _, r, n, k, *_ in S.SK_CASES + S.SK_EXTRA}
    f16w = {(kern, S.expected_plan(kern, n, k, r)["ks"]) for kern, r, n, k, *_, wt in S.CASES if wt == S.F16W}
    assert f16w == {(2, ks) for ks in range(1, 9)} | {(3, ks) for ks in (1, 2, 4, 8)}


def test_plan_of_every_tested_shape_and_the_plans_that_exist():
    """wq4_gemm_plan against the restated rules at every case of the table
    (each on the kernel the case names), and the literal list of plans: the
    table reaches every (per, ks) of the decode kernel at every launch count,
    and every (ks, nt, row tiles) of the decode-step kernel."""
    dec, sk = set(), set()
    for kern, rows, n, k, *_, wt in S.CASES + S.CONTROLS:
        wq4.set_kernel_policy(kern)
        p = wq4.gemm_plan(n, k, rows, wt)
        assert p == S.expected_plan(kern, n, k, rows), (kern, rows, n, k)
        assert p["kernel"] == kern, (kern, rows, n, k)  # the table names the kernel it runs
        if kern == 2:
            assert p["w"] == 8 and p["chunk"] == p["per"]
            dec.add(_dec_key(p) + (p["launches"],))
        else:
            sk.add(_sk_key(p))
    assert dec == {(per, ks, l) for per, ks in ((1, 1), (2, 1), (3, 1), (2, 2), (3, 2), (3, 3), (3, 4), (3, 5), (3, 6),
                                                (3, 7), (3, 8)) for l in (1, 2, 3, 4)}
    assert sk == {(ks, nt, rt) for ks in (1, 2, 4, 8) for nt in (1, 2, 4) for rt in (1, 2)}
    assert {(per, ks) for per, ks, _ in dec} == set(S.DEC_PLANS) and sk == set(S.SK_PLANS)
    for kern, rows, n, k in S.BATCH:
        assert S.expected_plan(kern, n, k, rows)["kernel"] == kern
    assert {(kern, S.expected_plan(kern, n, k, r)["ks"]) for kern, r, n, k in S.BATCH} == \
        {(2, ks) for ks in range(1, 9)} | {(3, ks) for ks in (1, 2, 4, 8)}
    for kern, pair in S.FOLLOW.items():
        assert [S.expected_plan(kern, n, k, r)["ks"] for n, k, r in pair] == ([2, 3] if kern == 2 else [2, 4])


def _boundary_ks():
    """Every K of the table, every plan boundary of either kernel, each with
    the K one block (32) below and above."""
    ks = set(S.DEC_KS) | set(S.SK_KS) | {12320, 5248, 10368}
    for lo, hi in S.DEC_PLANS.values():
        ks |= {lo, hi}
    ks |= {k + d for k in tuple(ks) for d in (-32, 32)}
    return sorted(k for k in ks if 32 <= k <= 16384)


def test_plan_walk_against_the_rules():
    """The restated rules against wq4_gemm_plan over a grid of (N, K, rows,
    weight type) under policies 2, 3 and 0: every table entry, every plan
    boundary K and the K one block to either side, N to either side of the
    workspace bounds, rows to either side of every m-tile and row-tile
    boundary.  The plans met are the literal list and no other; the (per, ks)
    of the decode kernel is the one DEC_PLANS gives for its K range.

    The workspace-bound branches (ntiles * ks * 1024 floats past the
    workspace: N > 16384 for the decode kernel, whose n-tiles come in pairs
    -- 514 of them from N = 16385) are covered here only and not on the GPU:
    the decode kernel never runs with a reduced ks -- its
    natural ks is the smallest with <= 3 block pairs per wave, so a smaller
    one always leaves the 8-wave branch and the launcher runs the tile
    kernel."""
    ns = sorted(set(S.DEC_NS) | set(S.SK_NS) | {c[2] for c in S.SK_EXTRA}
                | {1, 16, 32, 63, 65, 1280, 5120, 16384, 16400, 16416, 16448, 21824, 21888, 32768, 32784, 43712, 65536})
    rows_ = (1, 15, 16, 17, 32, 33, 64, 65, 96, 97, 100, 128, 129)
    seen_dec, seen_sk, bound = set(), set(), 0
    for pol in (2, 3, 0):
        wq4.set_kernel_policy(pol)
        for n in ns:
            for k in _boundary_ks():
                for rows in rows_:
                    for wt in (S.Q4, S.F16W):
                        got = wq4.gemm_plan(n, k, rows, wt)
                        if pol == 0:  # by rows: the decode-step kernel where it applies, else the decode kernel to 128
                            want = S.expected_plan(3, n, k, rows) if rows <= 128 else None
                            if want is None:
                                assert got["kernel"] == 1
                                continue
                        else:
                            want = S.expected_plan(pol, n, k, rows)
                            if rows > 128:
                                assert got["kernel"] == 1, (pol, n, k, rows)
                                continue
                        assert got == want, (pol, n, k, rows, wt)
                        if got["kernel"] == 2:
                            lo, hi = S.DEC_PLANS[_dec_key(got)]
                            assert lo <= k <= hi and got["w"] == 8 and got["launches"] == -(-rows // 32)
                            seen_dec.add(_dec_key(got))
                        elif got["kernel"] == 3:
                            seen_sk.add(_sk_key(got))
                        elif k <= 12288 and rows <= 128:  # the tile kernel below the K limit: the workspace bound
                            ntiles, ks = -(-n // 64) * 2, -(-(-(-k // 64)) // 24)
                            assert ntiles * ks > 4096 and n > 16384, (pol, n, k, rows)
                            bound += 1
    assert seen_dec == set(S.DEC_PLANS) and seen_sk == set(S.SK_PLANS)
    assert bound > 0
    # the first N whose 12288-wide weight is bound (514 n-tiles x 8 slices > 4096 slabs), and the last that is not
    wq4.set_kernel_policy(2)
    assert wq4.gemm_plan(16385, 12288, 1) == {"kernel": 1, "geo": 0}
    assert wq4.gemm_plan(16384, 12288, 1)["ks"] == 8
    assert wq4.gemm_plan(16416, 6144, 1)["ks"] == 4 and wq4.gemm_plan(65536, 3072, 128)["ks"] == 2
    assert wq4.gemm_plan(65536, 3104, 1) == {"kernel": 1, "geo": 0}
    # the decode-step kernel's workspace bound: 4096 slabs of 1024 floats
    wq4.set_kernel_policy(3)
    assert wq4.gemm_plan(16384, 5376, 32) == {"kernel": 3, "ks": 8, "nt": 4, "row_tiles": 2}  # 512 tiles x 8 slices
    assert wq4.gemm_plan(16400, 5376, 32)["kernel"] == 2 and wq4.gemm_plan(16400, 5376, 16)["kernel"] == 3


def test_the_three_fallbacks():
    """By name: the decode kernel at K = 12320 (193 block pairs) is the tile
    kernel's, at 1 and at 100 rows; the decode-step kernel at K = 5248 (164
    blocks: 41 per slice at ks 4, not a multiple of 8) and at K = 10368 (324
    blocks) is the decode kernel's; N % 16 != 0 is never the decode-step
    kernel's."""
    wq4.set_kernel_policy(2)
    for rows in (1, 100):
        assert wq4.gemm_plan(1312, 12288, rows)["kernel"] == 2
        assert wq4.gemm_plan(1312, 12320, rows) == {"kernel": 1, "geo": 0}
        assert wq4.gemm_kernel_name(1312, 12320, rows) == "q4_gemm_prefill_kernel"
        assert wq4.gemm_kernel_name(1312, 12288, rows) == "q4_gemm_decode_kernel"
    for pol in (3, 0):
        wq4.set_kernel_policy(pol)
        for k, ks in ((5248, 4), (10368, 7)):
            for rows in (1, 32):
                p = wq4.gemm_plan(96, k, rows)
                assert p["kernel"] == 2 and p["ks"] == ks, (pol, k, rows)
                assert wq4.gemm_kernel_name(96, k, rows) == "q4_gemm_decode_kernel"
        assert wq4.gemm_plan(96, 5120, 32)["kernel"] == 3 and wq4.gemm_plan(96, 10240, 32)["kernel"] == 3
        for n in (100, 8, 24, 1300):
            assert wq4.gemm_plan(n, 128, 16)["kernel"] == 2, (pol, n)
            assert wq4.gemm_kernel_name(n, 128, 16) == "q4_gemm_decode_kernel"
        assert wq4.gemm_plan(96, 128, 33)["kernel"] == 2  # rows <= 32 only
    assert wq4.gemm_plan(96, 100, 16) == {"kernel": 0} and wq4.gemm_plan(96, 128, 0) == {"kernel": 0}


def _accepted_four_wave(ntiles, nbp):
    """decode_rule over an array of n-tile counts at one nbp: where the plan
    is a 4-wave one the launcher accepts (per <= 4)."""
    ks8 = np.maximum(1, np.minimum(-(-nbp // 24), 4096 // ntiles))
    eight = (nbp <= 192) & (ntiles <= 65536) & (-(-nbp // (8 * ks8)) <= 3)
    per = np.ones_like(ntiles)
    for c in (1, 2, 4):  # the last assignment wins: 4 before 2 before 1
        per = np.where(ntiles * -(-nbp // (4 * c)) >= 192, c, per)
    ks = np.maximum(1, np.minimum(np.minimum(8, -(-nbp // (4 * per))), 2048 // ntiles))
    ks = np.where(ntiles > 65536, 1, ks)
    chunk = -(-nbp // (4 * ks))
    for _ in range(8):
        per = np.where(chunk > per, per * 2, per)
    return ~eight & (per <= 4) & (chunk <= per)


def test_no_four_wave_decode_plan_up_to_two_million_columns():
    """Settled by enumeration: over every n-tile count of N <= 2^21 (even
    counts 2 .. 65536) and every K <= 16384 (1 .. 256 block pairs), no shape
    selects a 4-wave decode plan that the launcher accepts (per <= 4).  A
    shape that leaves the 8-wave branch had its ks cut by the workspace to
    ks' with nbp > 24 ks'; the 4-wave branch may use at most as many slices
    (its slabs are twice as large), and 4 waves x 4 pairs x ks' = 16 ks'
    < nbp.  The first accepted 4-wave plan is past the counters, at N =
    2^21 + 64 (ntiles 65538, K <= 1024).  The array form of the rule used here
    is held to the scalar one, and the scalar one to wq4_gemm_plan, on a
    sample that includes those shapes."""
    ntiles = np.arange(2, 65537, 2, dtype=np.int64)
    hits = [(int(t), nbp) for nbp in range(1, 257) for t in ntiles[_accepted_four_wave(ntiles, nbp)]]
    assert hits == []
    past = np.array([65538], dtype=np.int64)
    assert [nbp for nbp in range(1, 257) if _accepted_four_wave(past, nbp)[0]] == list(range(1, 17))
    rng = np.random.default_rng(4)
    sample = [(int(t), int(b)) for t, b in zip(rng.choice(ntiles, 4000), rng.integers(1, 257, 4000))]
    sample += [(t, b) for t in (2, 42, 190, 192, 512, 1024, 1026, 2048, 2050, 4096, 4098, 65536, 65538)
               for b in (1, 4, 16, 17, 24, 25, 48, 49, 96, 97, 128, 129, 192, 193, 256)]
    wq4.set_kernel_policy(2)
    for t, b in sample:
        w, per, ks, chunk = S.decode_rule(t, b)
        four = w == 4 and per <= 4
        assert bool(_accepted_four_wave(np.array([t], dtype=np.int64), b)[0]) == four, (t, b)
        got = wq4.gemm_plan(t * 32, b * 64, 1)
        if w == 8 or four:
            assert (got["kernel"], got["w"], got["per"], got["ks"], got["chunk"]) == (2, w, per, ks, chunk), (t, b)
        else:
            assert got == {"kernel": 1, "geo": 0}, (t, b)
    # the one place a 4-wave plan runs: past 2^21 columns, one launch per two m-tiles
    assert wq4.gemm_plan((1 << 21) + 64, 1024, 128) == {"kernel": 2, "w": 4, "per": 4, "ks": 1, "chunk": 4, "launches": 2}
    assert wq4.gemm_plan((1 << 21) + 64, 1056, 1) == {"kernel": 1, "geo": 0}
    assert wq4.gemm_plan(1 << 21, 1024, 1)["w"] == 8
