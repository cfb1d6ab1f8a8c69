"""The small shape table of the encoder-size (rows > 128) Q4 GEMM tests, shared
by test_q4_guard_gpu.py (GPU) and test_q4_routing.py (CPU), with the routing
rule of those GEMMs restated in literal numbers.  No GPU import.

The smallest shapes at which the kernels' padding logic is live:

  rows 129   one past the 128-row granule of the A-tiled operand
       257   one past a wide-kernel group of 256 rows
       300   an m-tile partly real (300 = 9 * 32 + 12)
       384   a multiple of 128 but not of 256: the production case (48000 rows)
       512   no padding at all, the control
  N    64    one n-tile pair
       96    N % 64 == 32: a padding n-tile
       100   N % 32 != 0: columns masked inside an n-tile
       320   the second 8-tile n-group holds 2 of 8 n-tiles
       1312  the production N % 64 == 32 (42 n-tiles: 5 full groups + 2)
  K    32    one block: a padded half pair in the peeled first pair
       64, 96, 160, 448   1, 2 (one half padded), 3 (padded) and 7 block pairs

CASES is a covering set, not the product: with rows i, N j and K (i + j) % 5
every (rows, N) pair and every (N, K) pair appears exactly once in 25 cases;
the epilogue variant and the operand precision rotate over them.
"""
from __future__ import annotations

ROWS = (129, 257, 300, 384, 512)
NS = (64, 96, 100, 320, 1312)
KS = (32, 64, 96, 160, 448)

PREC_F16X2, PREC_F16 = 0, 1  # wq4.PREC_*

# (flags, residual aliases y): 1 GELU, 2 residual, 4 A-tiled output
VARIANTS = ((0, False), (1, False), (2, True), (2, False), (4, False))


def _cases():
    out = []
    for i, rows in enumerate(ROWS):
        for j, n in enumerate(NS):
            k = KS[(i + j) % 5]
            flags, inplace = VARIANTS[(2 * i + j) % 5]
            if flags == 4 and n % 32 != 0:  # an A-tiled output needs N % 32 == 0: GELU + in-place residual there
                flags, inplace = 3, True
            prec = PREC_F16 if (i + 3 * j) % 4 == 0 else PREC_F16X2
            out.append((rows, n, k, flags, inplace, prec))
    return tuple(out)


CASES = _cases()  # (rows, n, k, flags, residual in place, prec)

# The cases of test_q4_gpu.py::test_enc_kernel_bit_identical: (m, n, k, flags, prec)
ENC_BIT_IDENTICAL = (
    (1500, 1280, 1280, 0, 0), (3000, 3840, 1280, 0, 0), (700, 5120, 1280, 5, 0),
    (300, 1280, 5120, 2, 0), (2049, 1280, 1280, 1, 0), (16000, 1280, 1280, 2, 0),
    (4500, 5120, 1280, 5, 0), (200, 96, 160, 0, 0), (1000, 1312, 1280, 4, 0),
    (2049, 1280, 1280, 4, 0), (1500, 1280, 5120, 3, 0), (2000, 5120, 1280, 5, 1),
    (300, 1312, 160, 4, 1),
    # K loop lengths for the wide kernel's peeled first block pair,
    # three-pair trips and 0-3 trailing pairs (nbp = K / 64: 1, 4, 5, 6, 7)
    (600, 1280, 64, 1, 0), (500, 1280, 256, 0, 0), (900, 1280, 320, 2, 0),
    (400, 1280, 384, 0, 1), (700, 1280, 448, 4, 0))

TILE, RING, WIDE = "q4_gemm_prefill_kernel", "q4_gemm_enc_kernel", "q4_gemm_wide_kernel"


def enc_modes(prec):
    """The encoder-kernel modes a bit-equality test runs: the ring kernel
    (2, 3, 4: its three geometries) has f16x2 operands only."""
    return (0, 2, 3, 4, 5, 1) if prec == PREC_F16X2 else (0, 5, 1)


def expected_kernel(mode, rows, n, prec):
    """The kernel of a Q4_0 GEMM under kernel policy 1 (no decode kernels) and
    encoder-kernel mode `mode` (wq4_debug_set_enc_kernel), restated from
    enc_gemm_pick (wq4_enc.hip) in literal numbers.  K plays no part.

    Up to 128 rows: the tile kernel.  Above, with the rows padded to 128 and
    counted in m-tiles of 32 and N padded to 64 and counted in n-tiles of 32
    (so the n-tile count is always even, which is all the wide kernel asks of a
    shape): mode 0 the tile kernel; mode 5 the wide kernel; modes 2, 3, 4 the
    ring kernel at f16x2 operands and the tile kernel at f16; mode 1 the wide
    kernel from 170 of its 256 x 256 workgroups, else at f16x2 the ring kernel
    while the tile kernel's 128 x 256 grid is under 400 workgroups, else the
    tile kernel."""
    if rows <= 128 or mode == 0:
        return TILE
    if mode == 5:
        return WIDE
    mtiles = -(-rows // 128) * 4
    ngroups = -(-(-(-n // 64) * 2) // 8)
    if mode == 1 and -(-mtiles // 8) * ngroups >= 170:
        return WIDE
    if prec != PREC_F16X2:
        return TILE
    if mode in (2, 3, 4):
        return RING
    return RING if mtiles // 4 * ngroups < 400 else TILE
