"""The shape table of the Q4 GEMM tests at 128 rows and below, shared by
test_q4_small_gpu.py (GPU) and test_q4_small_routing.py (CPU), with the launch
plans of the two small-M kernels restated in literal numbers.  No GPU import.

Both kernels choose a plan from (N, K):

  the decode kernel (kernel 2, rows <= 128), plan_decode in wq4_q4gemm.hip.
    With nbp = ceil(K / 64) block pairs and ntiles = 2 ceil(N / 64) n-tiles,
    one 8-wave workgroup per (n-tile, K slice): ks = ceil(nbp / 24) slices,
    each wave chunk = ceil(nbp / (8 ks)) <= 3 block pairs, the kernel
    instance per = chunk.  K <= 12288.  One launch per 32-row m-tile, all on
    the stream's one workspace.  ks is kept within the workspace (ntiles * ks
    <= 4096 slabs); a smaller ks makes chunk > 3, and with every other shape
    that leaves this branch the launcher runs the tile kernel instead.
  the decode-step kernel (kernel 3, rows <= 32, K % 128 == 0, N % 16 == 0),
    skinny_ks / skinny_nt in wq4_skinny.hip.  With kb = K / 32 blocks: ks =
    the first of 1, 2, 4, 8 that divides kb with kb / ks <= 40; nt = the first
    of 1, 2 with (N padded to 64) / (16 nt) * ks * row tiles <= 256, else 4;
    row tiles = ceil(rows / 16).

The axes (every value sits on one side of a plan boundary):

  rows   1, 16, 17, 32 for both kernels; 33, 65, 100, 128 for the decode
         kernel: 2, 3, 4 and 4 m-tile launches on one workspace
  K      decode kernel: both sides of every (per, ks) boundary in block pairs;
         K % 64 == 32 (544, 1056, 1568, ...) is a padded half pair in the last
         wave that has work.  K = 1568 (nbp 25, ks 2, chunk 2) leaves waves
         5-7 of the second slice empty and its wave 4 with one pair; K = 3104
         (nbp 49, ks 3, chunk 3) gives the third slice one pair in wave 0.
         decode-step kernel: 128 (four of eight waves idle), both sides of
         every ks boundary, 2688 (21 blocks per slice, an odd split over the
         waves)
  N      decode kernel: 64, 96 (a padding n-tile), 100 (columns masked inside
         a tile), 1312.  decode-step kernel: 16, 48 (one padding subtile in
         the 64-column slab), 96, 272, 528, 1312

The tables are covering sets, not products.  DEC_CASES: K i and rows j meet in
every pair (160 cases) with N (i + j) % 4, so every (K, N) pair appears twice.
SK_CASES: K i and N l meet in every pair (54 cases) with rows (i + l) % 4, so
every (K, rows) pair appears at least once.  Over both, the epilogue variant is
VARIANTS[(2 i + j) % 5] (a case whose N % 32 != 0 runs GELU + an in-place
residual where the A-tiled output would come up), f16 operands where
(i + 3 j) % 4 == 0, and f16 weights in one case per K (rows index i % 8 of the
decode kernel; N index i % 6 of the decode-step kernel).  SK_EXTRA adds the
(ks, nt, row tiles) plans of the decode-step kernel that need N > 1312 (at
the smallest K of their ks; none of these weights is larger than 3.3 MB) or
N = 1312 at a row count the rotation does not pair it with, and (528, 5376)
at 17 rows.
The largest weight is 1312 x 12288 Q4_0 (8 MB).
"""
from __future__ import annotations

PREC_F16X2, PREC_F16 = 0, 1  # wq4.PREC_*
Q4, F16W = 0, 1              # weight types of wq4.gemm_plan

DEC_ROWS = (1, 16, 17, 32, 33, 65, 100, 128)
DEC_KS = (32, 512, 544, 1024, 1056, 1536, 1568, 3072, 3104, 4608, 4640, 6144, 6176, 7680, 7712, 9216, 9248, 10752,
          10784, 12288)
DEC_NS = (64, 96, 100, 1312)

SK_ROWS = (1, 16, 17, 32)
SK_KS = (128, 384, 1280, 1408, 2560, 2688, 5120, 5376, 10240)
SK_NS = (16, 48, 96, 272, 528, 1312)

# (flags, residual aliases y): 1 GELU, 2 residual, 4 A-tiled output
VARIANTS = ((0, False), (1, False), (2, True), (2, False), (4, False))

# The (per, ks) plans of the decode kernel (w = 8, chunk = per) with the K
# range of each, and the (ks, nt, row tiles) plans of the decode-step kernel:
# what the rules can produce for N <= 65536, K <= 12288.
DEC_PLANS = {(1, 1): (32, 512), (2, 1): (544, 1024), (3, 1): (1056, 1536), (2, 2): (1568, 2048), (3, 2): (2080, 3072),
             (3, 3): (3104, 4608), (3, 4): (4640, 6144), (3, 5): (6176, 7680), (3, 6): (7712, 9216),
             (3, 7): (9248, 10752), (3, 8): (10784, 12288)}
SK_PLANS = frozenset((ks, nt, rt) for ks in (1, 2, 4, 8) for nt in (1, 2, 4) for rt in (1, 2))


# ------------------------------------------------------------- the rules --
def decode_rule(ntiles, nbp):
    """plan_decode in literal numbers: (w, per, ks, chunk)."""
    if nbp <= 192 and ntiles <= 65536:
        ks = -(-nbp // 24)
        while ks > 1 and ntiles * ks > 4096:  # 16 MiB of 4 KiB slabs
            ks -= 1
        chunk = -(-nbp // (8 * ks))
        if chunk <= 3:
            return 8, chunk, ks, chunk
    per = 1
    for c in (4, 2, 1):  # the deepest waves whose grid still covers the CUs
        if ntiles * -(-nbp // (4 * c)) >= 192:
            per = c
            break
    ks = min(8, -(-nbp // (4 * per)))
    while ks > 1 and ntiles * ks > 2048:  # slabs of 2 m-tiles
        ks -= 1
    if ntiles > 65536:
        ks = 1
    chunk = -(-nbp // (4 * ks))
    while chunk > per:
        per *= 2
    return 4, per, ks, chunk


def decode_plan(n, k, rows):
    """The plan the decode kernel's launcher runs, as wq4.gemm_plan reports it,
    or None where it hands the GEMM to the tile kernel family."""
    w, per, ks, chunk = decode_rule(-(-n // 64) * 2, -(-k // 64))
    mtiles = -(-rows // 32)
    if rows < 1 or mtiles > 4 or per > (3 if w == 8 else 4):
        return None
    return {"kernel": 2, "w": w, "per": per, "ks": ks, "chunk": chunk,
            "launches": mtiles if w == 8 else -(-mtiles // 2)}


def skinny_plan(n, k, rows):
    """The decode-step kernel's plan, or None for a shape it does not take."""
    if rows < 1 or rows > 32 or k % 128 or n % 16:
        return None
    kb, sub, rt = k // 32, -(-n // 64) * 4, -(-rows // 16)
    ks = next((s for s in (1, 2, 4, 8) if kb % s == 0 and kb // s <= 40), 0)
    if ks == 0:
        return None
    nt = next((t for t in (1, 2) if sub // t * ks * rt <= 256), 4)
    tiles = sub // nt * rt
    if tiles * ks > 4096 or tiles > 65536:  # the workspace's slabs and counters
        return None
    return {"kernel": 3, "ks": ks, "nt": nt, "row_tiles": rt}


def expected_plan(kernel, n, k, rows):
    """wq4.gemm_plan under kernel policy `kernel` (2 or 3) for rows <= 128:
    policy 3 runs the decode kernel where the decode-step kernel does not take
    the shape, and either ends on the tile kernel (geometry 0 at these row
    counts) where the decode kernel does not."""
    p = skinny_plan(n, k, rows) if kernel == 3 else None
    return p or decode_plan(n, k, rows) or {"kernel": 1, "geo": 0}


# -------------------------------------------------------------- the cases --
def _variant(i, j, n):
    flags, inplace = VARIANTS[(2 * i + j) % 5]
    if flags == 4 and n % 32 != 0:  # an A-tiled output needs N % 32 == 0
        flags, inplace = 3, True
    return flags, inplace, PREC_F16 if (i + 3 * j) % 4 == 0 else PREC_F16X2


def _dec_cases():
    out = []
    for i, k in enumerate(DEC_KS):
        for j, rows in enumerate(DEC_ROWS):
            n = DEC_NS[(i + j) % 4]
            out.append((2, rows, n, k) + _variant(i, j, n) + (F16W if j == i % 8 else Q4,))
    return tuple(out)


def _sk_cases():
    out = []
    for i, k in enumerate(SK_KS):
        for l, n in enumerate(SK_NS):
            j = (i + l) % 4
            out.append((3, SK_ROWS[j], n, k) + _variant(i, j, n) + (F16W if l == i % 6 else Q4,))
    return tuple(out)


# (kernel, rows, n, k, flags, residual in place, prec, weight type)
DEC_CASES = _dec_cases()
SK_CASES = _sk_cases()
# the decode-step plans past N = 1312: ks 1 at K = 128, 2 at 1408, 4 at 2688
SK_EXTRA = ((3, 17, 2064, 128, 0, False, PREC_F16X2, Q4),    # (1, 2, 2)
            (3, 16, 4112, 128, 2, True, PREC_F16X2, Q4),     # (1, 2, 1)
            (3, 17, 4112, 128, 1, False, PREC_F16, Q4),      # (1, 4, 2)
            (3, 16, 8208, 128, 2, False, PREC_F16X2, F16W),  # (1, 4, 1)
            (3, 16, 2064, 1408, 3, True, PREC_F16X2, Q4),    # (2, 2, 1)
            (3, 1, 4112, 1408, 0, False, PREC_F16X2, Q4),    # (2, 4, 1)
            (3, 17, 2064, 1408, 2, True, PREC_F16, Q4),      # (2, 4, 2)
            (3, 16, 2064, 2688, 1, False, PREC_F16X2, Q4),   # (4, 4, 1)
            # N = 1312 with the row tiles the rotation does not pair it with
            (3, 32, 1312, 1408, 4, False, PREC_F16, Q4),     # (2, 2, 2); the A-tiled output at f16 operands
            (3, 16, 1312, 2688, 2, False, PREC_F16, Q4),     # (4, 2, 1)
            # ks 8 with nt 4 at 17 rows (the rotation pairs N = 528, K = 5376 with 32 rows)
            (3, 17, 528, 5376, 2, True, PREC_F16X2, Q4))     # (8, 4, 2)
CASES = DEC_CASES + SK_CASES + SK_EXTRA

# Launch independence: after three identical launches of a case with ks > 1,
# one launch of another (N, K) whose ks differs, on the same workspace:
# (n, k, rows) by kernel, the second entry where the case's own ks is the
# first entry's.
FOLLOW = {2: ((96, 1568, 17), (96, 3104, 17)),   # ks 2, ks 3
          3: ((48, 1408, 17), (48, 2688, 17))}   # ks 2, ks 4
# ks = 1 controls of the launch-independence test
CONTROLS = ((2, 100, 100, 1536, 0, False, PREC_F16X2, Q4), (3, 32, 96, 1280, 0, False, PREC_F16X2, Q4))

# Batch invariance: one (rows, n, k) per (kernel, ks), at the first K of the ks
BATCH = tuple((2, 100, 100, next(k for k in DEC_KS if -(-(-(-k // 64)) // 24) == ks)) for ks in range(1, 9)) + \
    tuple((3, 32, 96, k) for k in (128, 1408, 2688, 5376))
