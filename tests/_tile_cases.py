"""Case tables of tests/test_tile_instances_host.py and tests/test_gpu_tile_instances.py, and (last section) of
tests/test_split6_instances_host.py and tests/test_gpu_split6_instances.py (a plain helper module, not a conftest).

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


# ---- six-term plane GEMMs (csrc/split6_gemm.hip: dhz_linear_fwd_split6 / _dgrad_split6 / _fwd_split6_res).  Instances are written
# 10 (tile rows / 32) + tile columns / 32, as dhz_linear_split6_tile answers: 84 = split6_wide_kernel (256 x 128, two-slot ring),
# 44 / 42 / 41 = split6_gemm_kernel at 128 x 128 / 64 / 32 (three-slot ring, loop unrolled x 6).  Each runs as forward, backward-data
# (features a multiple of 64: none at 41) and forward + residual epilogue: eleven instantiations.
#
# Levels: the whole device, grids sized for 8 and for 9 CUs, and deterministic mode at 8 and at 9 reserved CUs - there the CHOICE is
# made for 256 CUs while the GRID is the reserved one (one workgroup per CU: grid = min(tiles, CUs)).
#
# Trip rule.  84, 42 and 41 can be given any number of tiles: their cases make three trips and more with a ragged last trip and a
# ragged last row tile.  44 is chosen only when the 256-row tiles of the wide kernel number fewer than the CUs of the choice, so
# outside deterministic mode it has fewer than 2 x CUs tiles and can never make more than two trips: its plain cases make two, the
# second ragged; its many-trip cases (three and more, six and more for the one- and two-stage contractions) are deterministic ones.
S6_LEVELS = ((None, False), (8, False), (9, False), (8, True), (9, True))       # (reserved CUs, deterministic mode)
S6_TABLED = S6_LEVELS[1:]                      # the levels S6_TABLE makes claims for, in its column order
S6_INSTANCES = (84, 44, 42, 41)
S6_MODES = ("fwd", "dgrad", "epi")
S6_CONTRACTIONS = (32, 64, 96, 160, 192, 224)  # 1, 2, 3, 5, 6, 7 stages of 32 per tile
# S6_TABLE[(T, features)] = (instance, trips) at 8 CUs, at 9 CUs, deterministic at 8, deterministic at 9
S6_TABLE = {
    (7000, 128): ((84, 4), (84, 4), (44, 7), (44, 7)),     # 28 wide tiles, last trip 4 / 1, rows ragged by 88; det: 55 tiles, 7 trips
    (8100, 128): ((84, 4), (84, 4), (42, 16), (42, 15)),   # 32 wide tiles: four full trips at 8 with the XCD remap on
    (7104, 256): ((84, 7), (84, 7), (42, 28), (42, 25)),   # 56 wide tiles on two column tiles, seven trips (last 8 / 2), rows ragged by 192
    (3520, 128): ((84, 2), (84, 2), (44, 4), (44, 4)),     # det: 28 tiles, four trips (last 4 / 1), rows ragged by 64
    (3072, 128): ((84, 2), (84, 2), (44, 3), (44, 3)),     # det at 8: 24 tiles of 44, three full trips with the remap on
    (1728, 128): ((44, 2), (44, 2), (44, 2), (44, 2)),     # 14 tiles: 8 + 6, 9 + 5; rows ragged by 64
    (704, 256): ((44, 2), (44, 2), (44, 2), (44, 2)),      # 12 tiles on two column tiles: at 9 a workgroup changes column tile
    (704, 128): ((42, 2), (42, 2), (44, 1), (44, 1)),      # 42 by demotion (6 tiles of 128 x 128 < CUs): 12 tiles
    (2500, 192): ((42, 8), (42, 7), (42, 8), (42, 7)),     # 60 tiles on three column tiles, last trip 4 / 6, rows ragged by 68
    (3072, 64): ((42, 3), (42, 3), (42, 3), (42, 3)),      # 24 tiles: three full trips at 8 with the remap on
    (1216, 192): ((42, 4), (42, 4), (42, 4), (42, 4)),     # 30 tiles, rows ragged by 64
    (1200, 160): ((41, 7), (41, 6), (41, 7), (41, 6)),     # 50 tiles on five column tiles, last trip 2 / 5, rows ragged by 48
    (3072, 32): ((41, 3), (41, 3), (41, 3), (41, 3)),      # 24 tiles: three full trips at 8 with the remap on
    (1216, 96): ((41, 4), (41, 4), (41, 4), (41, 4)),      # 30 tiles on three column tiles, rows ragged by 64
}
S6_MAX = (8100, 384, 224)                      # no case is larger than this many tokens, features, contraction elements


def s6_modes(features):
    """the modes a width runs in: backward-data needs a multiple of 64 output features"""
    return tuple(m for m in S6_MODES if m != "dgrad" or features % 64 == 0)


def s6_query(lib, mode, T, features, contraction):
    """dhz_linear_split6_tile for `features` output columns: the forward has N = features, K = contraction, backward-data the reverse"""
    return lib.dhz_linear_split6_tile(2, T, contraction, features) if mode == "dgrad" else lib.dhz_linear_split6_tile(1, T, features, contraction)


def s6_plan(instance, T, features, ncu):
    """(tiles, grid, trips, remap on) of the persistent launch of `instance` on grids sized for ncu CUs (launch / launch_wide)"""
    bm, bn = 32 * (instance // 10), 32 * (instance % 10)
    ntiles = -(-T // bm) * (features // bn)
    grid = min(ntiles, ncu)
    return ntiles, grid, -(-ntiles // grid), grid % 8 == 0 and ntiles % 8 == 0


def s6_stream(instance, T, features, ncu, wg=0):
    """the (row tile, column tile) pairs workgroup `wg` walks, in order (tile_of of both kernels, XCD remap included)"""
    ntiles, grid, _, on = s6_plan(instance, T, features, ncu)
    tiles_n = features // (32 * (instance % 10))
    out = []
    for lin in range(wg, ntiles, grid):
        tile = (lin & 7) * (ntiles >> 3) + (lin >> 3) if on else lin
        out.append(divmod(tile, tiles_n))
    return out


def s6_level(ncu, det):
    """context: grids sized for ncu CUs (None: the whole device), in deterministic mode where det; both are given back on the way
    out.  Yields the CU count the grids are sized for."""
    import contextlib
    from _grid import reserved_grid
    from dehaze_hip import _lib as L

    @contextlib.contextmanager
    def level():
        assert L.load().dhz_get_deterministic() == 0
        with reserved_grid(ncu) as n:
            try:
                if det:
                    L.call("dhz_set_deterministic", 1)
                yield n
            finally:
                L.call("dhz_set_deterministic", 0)
    return level()


def s6_no_override():
    """the tables describe the dispatch as it ships: the diagnostic override of tools/pmc_split6.sh must not be set"""
    import os
    assert "DHZ_S6_TILE" not in os.environ, ("DHZ_S6_TILE is set: it forces the tile of csrc/split6_gemm.hip (a diagnostic of "
                                             "tools/pmc_split6.sh); unset it to run the instance tests")


S6_BOUND, S6_FLOOR = 2.0 ** -21, 1e-7          # the six-term bound: |err| <= 2^-21 mag + 1e-7, mag = the reference over absolute values


def s6_operands(T, features, contraction, device, seed):
    """activations [T, contraction], weight [features, contraction] (rows of unit norm on average), bias [features], drawn on `device`"""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(T, contraction, generator=g, device=device)
    w = torch.randn(features, contraction, generator=g, device=device) / contraction ** 0.5
    b = torch.randn(features, generator=g, device=device)
    return x, w, b
