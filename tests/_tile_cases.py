"""Case tables of tests/test_tile_instances_host.py and tests/test_gpu_tile_instances.py (a plain helper module, not a conftest).

csrc/conv_gemm.hip (dhz_conv4s2_fwd / _dgrad) and csrc/linear_gemm.hip (dhz_linear_fwd / _dgrad) pick a tile instance <WM, WN> from the
problem size and the CU count: the first candidate, largest first, with at least 2 x CUs blocks, else the candidate with the most
blocks.  On the whole device that is 512 slots and every small problem falls back to the smallest tiles on a single trip of the
persistent loop; under the reservations of tests/_grid.py (grids sized for 8 or 9 CUs: 16 or 18 slots) the small maps below select the
big tiles and make several trips.  Instances are written 10 WM + WN, as dhz_conv4s2_tile / dhz_linear_tile answer.

Trip rule.  A tile that is the FIRST candidate its width admits can be given any number of blocks: such cases make three trips with a
ragged last one.  A later candidate is chosen only when the candidate twice its height (which precedes it in the list) had fewer blocks
than slots, so it has fewer than 2 x slots blocks itself and can never make more than two trips: such cases make two, the second ragged.
"""

RESERVED = (8, 9)                      # the reserved levels of _grid.LEVELS: 16 and 18 workgroup slots

# ---- conv4s2 forward / backward-data.  Rows M = B (H/2) (W/2); N = Cout (forward), Cin (backward-data): every (Cin, Cout) pair names one
# forward and one backward-data instance, and every width is once the N of each mode.
CONV_CAND = ((4, 4), (4, 3), (4, 2), (2, 4), (2, 3), (2, 2), (4, 1), (2, 1))
CONV_PAIRS = ((32, 64), (64, 128), (128, 96), (96, 32))
CONV_MAPS = {
    "A": (5, 40, 100),                 # M = 5000 = 39 x 128 + 8: 40 tiles of the four first candidates, three trips (16+16+8, 18+18+4)
    "B": (2, 36, 82),                  # M = 1476 = 23 x 64 + 4: 24 tiles of the second choices, two trips
    "C": (2, 12, 118),                 # M = 708: H/2 = 6 rows of 59, so many border taps; small tiles
    "D": (2, 18, 100),                 # M = 900: the instance differs between 8 and 9 CUs
}
# CONV_TABLE[case][N] = ((instance, trips) at 8 CUs, (instance, trips) at 9 CUs); a width the table makes no claim for is absent
CONV_TABLE = {
    "A": {32: ((41, 3), (41, 3)), 64: ((42, 3), (42, 3)), 96: ((43, 3), (43, 3)), 128: ((44, 3), (44, 3))},
    "B": {32: ((21, 2), (21, 2)), 64: ((22, 2), (22, 2)), 96: ((23, 2), (23, 2)), 128: ((42, 2), (42, 2))},
    "C": {32: ((21, 1), (21, 1)), 64: ((21, 2), (21, 2)), 96: ((41, 2), (41, 1)), 128: ((22, 2), (22, 2))},
    "D": {64: ((41, 1), (21, 2)), 96: ((41, 2), (41, 2)), 128: ((42, 1), (22, 2))},
}
CONV_UNREACHABLE = (24,)               # (4,2) precedes (2,4) with at least as many blocks wherever N % 128 == 0

# ---- fp32 token GEMM.  Contraction per output width: 96 = three stages (the double-buffer parity flips from tile to tile), 32 = one
# stage (the next tile's prefetch sits in the only stage), 128 = four.  The conv contractions are always an even number of stages.
GEMM_CAND = ((4, 4), (4, 2), (2, 4), (2, 2), (4, 1), (2, 1))
GEMM_ROWS = (5000, 5120, 1476, 1472, 708, 704)
GEMM_CONTRACTION = {32: 96, 64: 32, 128: 128, 96: 64}
GEMM_PADDED_ROWS = (5000, 1476)        # these run with ldx > K and ldy > N
# GEMM_TABLE[rows][features] = (instance, trips), the same at 8 and at 9 CUs
GEMM_TABLE = {
    5000: {32: (41, 3), 64: (42, 3), 128: (44, 3)},
    5120: {32: (41, 3), 64: (42, 3), 128: (44, 3)},
    1476: {32: (21, 2), 64: (22, 2), 128: (42, 2)},
    1472: {32: (21, 2), 64: (22, 2), 128: (42, 2)},
    708: {32: (21, 1), 64: (21, 2), 128: (22, 2)},
    704: {32: (21, 1), 64: (21, 2), 128: (22, 2)},
    # 96 features = three column tiles of <4,1>: with the even grids of the rows above a workgroup meets one column tile only (two at
    # most, and grid-stride steps of 16 or 18 keep the parity); here 14 x 3 = 42 tiles, and on the grid of 16 every trip changes the column tile
    1668: {96: (41, 3)},
}
GEMM_CASES = tuple((M, N) for M in GEMM_TABLE for N in GEMM_TABLE[M])
GEMM_UNREACHABLE = (24,)

# ---- conv4s2 weight gradient: the instance is a function of (Cout, Cin) alone; Ho x Wo = 8 x 16, T = 384 tokens = 3 slabs of 128 at most
WGRAD_MAP = (3, 16, 32)
WGRAD_COUT = (32, 64, 96, 128)
WGRAD_CIN = (32, 64, 128)
WGRAD_NO_DB = ((32, 64), (64, 128), (96, 32), (128, 64))        # (Cout, Cin) run with db = NULL as well: once per WM


def wgrad_instance(Cout, Cin):
    return 10 * (Cout // 32) + {32: 1, 64: 2, 128: 4}[Cin]


def wgrad_splits(Cout, Cin, ncu):
    """token slabs per tile of launch_wgrad (csrc/conv_gemm.hip) on grids sized for ncu CUs"""
    wm, wn = divmod(wgrad_instance(Cout, Cin), 10)
    tiles = (Cout // (32 * wm)) * (16 * Cin // (32 * wn))
    T = WGRAD_MAP[0] * (WGRAD_MAP[1] // 2) * (WGRAD_MAP[2] // 2)
    return max(1, min(2 * ncu // tiles, max(1, T // 128)))


def conv_rows(case):
    B, H, W = CONV_MAPS[case]
    return B * (H // 2) * (W // 2)


def plan(instance, M, N, ncu):
    """(tiles, grid, trips, remap on) of the persistent launch of `instance` on grids sized for ncu CUs (launch() of both files)"""
    wm, wn = divmod(instance, 10)
    ntiles = -(-M // (32 * wm)) * (N // (32 * wn))
    grid = min(ntiles, 2 * ncu)
    return ntiles, grid, -(-ntiles // grid), grid % 8 == 0 and ntiles % 8 == 0


def first_candidate(cand, N):
    """the first tile of the candidate list that N admits, as an instance number"""
    return next(10 * a + b for a, b in cand if N % (32 * b) == 0)
