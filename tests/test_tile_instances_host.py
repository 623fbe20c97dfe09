"""No GPU: which tile instance of csrc/conv_gemm.hip and csrc/linear_gemm.hip a shape gets, asked of the library itself
(dhz_conv4s2_tile, dhz_linear_tile: the function the dispatch calls), under the reservations tests/test_gpu_tile_instances.py runs at.
The tables of tests/_tile_cases.py select what they claim; their union is every instance a shape can reach at those levels; the one
instance outside it, <2,4>, is reachable at no level."""
import os
import re

from _grid import physical_cus, reserved_grid
import _tile_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhz_conv4s2_tile", "dhz_linear_tile")


def _lib():
    from dehaze_hip import _lib as L
    return L.load()


def conv_tile(lib, mode, case, Cin, Cout):
    return lib.dhz_conv4s2_tile(mode, *TC.CONV_MAPS[case], Cin, Cout)


def conv_tile_mn(lib, mode, M, N):
    """the forward / backward-data instance of M rows x N columns: M images with a 2 x 2 input map, the other width at 32"""
    return lib.dhz_conv4s2_tile(mode, M, 2, 2, 32 if mode == 1 else N, N if mode == 1 else 32)


def test_entries_declared_exported_bound():
    from dehaze_hip import _lib as L
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} is not declared in include/dehaze_hip.h"
        assert name in L.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == L.SIGNATURES[name]


def test_queries_answer_zero_for_refused_shapes():
    lib = _lib()
    for mode in (1, 2, 3):
        assert lib.dhz_conv4s2_tile(mode, 3, 16, 32, 32, 64) > 0
        for bad in [(3, 15, 32, 32, 64), (3, 16, 31, 32, 64), (3, 16, 32, 48, 64), (3, 16, 32, 32, 80), (0, 16, 32, 32, 64),
                    (3, 16, 32, 0, 64)]:
            assert lib.dhz_conv4s2_tile(mode, *bad) == 0, (mode, bad)
    assert lib.dhz_conv4s2_tile(0, 3, 16, 32, 32, 64) == 0 and lib.dhz_conv4s2_tile(4, 3, 16, 32, 32, 64) == 0
    assert lib.dhz_conv4s2_tile(1, 2, 12, 118, 32, 64) > 0 and lib.dhz_conv4s2_tile(3, 2, 12, 118, 32, 64) == 0   # wgrad: powers of two
    assert lib.dhz_conv4s2_tile(3, 1, 4, 8, 32, 64) == 0                                                          # wgrad: T % 32
    assert lib.dhz_linear_tile(100, 64) > 0
    for bad in [(0, 64), (100, 0), (100, 40), (100, 16 * 1024 + 32)]:
        assert lib.dhz_linear_tile(*bad) == 0, bad
    assert lib.dhz_linear_tile(100, 48) == 0 and lib.dhz_linear_tile(100, 16) == 0                               # the narrow kernel


def test_conv_table_selects_what_it_claims():
    """every row of CONV_TABLE, both modes, at 8 and 9 CUs: the instance by the query; tiles, grid and trips from that instance"""
    lib = _lib()
    best = {}                                   # (mode, instance) -> most trips seen with a ragged last one
    remap = {1: set(), 2: set()}
    for k, ncu in enumerate(TC.RESERVED):
        with reserved_grid(ncu):
            for case in TC.CONV_MAPS:
                M = TC.conv_rows(case)
                for Cin, Cout in TC.CONV_PAIRS:
                    for mode, N in ((1, Cout), (2, Cin)):
                        got = conv_tile(lib, mode, case, Cin, Cout)
                        assert got == conv_tile_mn(lib, mode, M, N)            # a function of (M, N) alone
                        if N not in TC.CONV_TABLE[case]:
                            continue
                        inst, trips = TC.CONV_TABLE[case][N][k]
                        assert got == inst, (case, mode, N, ncu, got)
                        ntiles, grid, t, on = TC.plan(got, M, N, ncu)
                        assert t == trips, (case, mode, N, ncu, ntiles, grid)
                        remap[mode].add(on)
                        if ntiles % grid:
                            best[(mode, got)] = max(best.get((mode, got), 0), t)
    assert remap == {1: {True, False}, 2: {True, False}}, "the XCD remap is on in one case and off in another, in both modes"
    every = {10 * a + b for a, b in TC.CONV_CAND} - set(TC.CONV_UNREACHABLE)
    firsts = {TC.first_candidate(TC.CONV_CAND, N) for N in (32, 64, 96, 128)}
    for mode in (1, 2):
        assert {i for m, i in best if m == mode} == every, (mode, sorted(best))
        for inst in every:                      # the trip rule of _tile_cases
            assert best[(mode, inst)] >= (3 if inst in firsts else 2), (mode, inst, best[(mode, inst)])
    # the cases the issue describes
    assert TC.plan(44, 5000, 128, 8) == (40, 16, 3, True) and TC.plan(23, 1476, 96, 8) == (24, 16, 2, True)
    assert TC.plan(44, 5000, 128, 9) == (40, 18, 3, False) and TC.plan(23, 1476, 96, 9) == (24, 18, 2, False)
    assert 5000 % 128 == 8 and 1476 % 64 == 4


def test_gemm_table_selects_what_it_claims():
    lib = _lib()
    best = {}                                   # (instance, ragged rows) -> most trips seen with a ragged last one
    for ncu in TC.RESERVED:
        with reserved_grid(ncu):
            for M, N in TC.GEMM_CASES:
                inst, trips = TC.GEMM_TABLE[M][N]
                got = lib.dhz_linear_tile(M, N)
                assert got == inst, (M, N, ncu, got)
                ntiles, grid, t, _ = TC.plan(got, M, N, ncu)
                assert t == trips, (M, N, ncu, ntiles, grid)
                rag = M % (32 * (got // 10)) != 0
                if ntiles % grid:
                    best[(got, rag)] = max(best.get((got, rag), 0), t)
                if N == 96 and ncu == 8:        # three column tiles against a grid of 16: every trip changes the column tile
                    assert N // (32 * (got % 10)) == 3 and grid % 3 != 0 and t == 3
    every = {10 * a + b for a, b in TC.GEMM_CAND} - set(TC.GEMM_UNREACHABLE)
    firsts = {TC.first_candidate(TC.GEMM_CAND, N) for N in TC.GEMM_CONTRACTION}
    assert set(best) == {(i, r) for i in every for r in (False, True)}, sorted(best)
    for (inst, rag), t in best.items():
        assert t >= (3 if inst in firsts else 2), (inst, rag, t)
    assert set(TC.GEMM_CASES) >= {(M, N) for M in TC.GEMM_ROWS for N in (32, 64, 128)} and set(TC.GEMM_PADDED_ROWS) <= set(TC.GEMM_ROWS)
    assert sorted(K // 32 for K in TC.GEMM_CONTRACTION.values()) == [1, 2, 3, 4]   # a single stage, odd and even numbers of them


def test_wgrad_table_runs_each_instance_once():
    lib = _lib()
    B, H, W = TC.WGRAD_MAP
    seen = []
    for lvl in (None,) + TC.RESERVED:
        with reserved_grid(lvl) as ncu:
            here = [lib.dhz_conv4s2_tile(3, B, H, W, Cin, Cout) for Cout in TC.WGRAD_COUT for Cin in TC.WGRAD_CIN]
            assert here == [TC.wgrad_instance(Cout, Cin) for Cout in TC.WGRAD_COUT for Cin in TC.WGRAD_CIN]
            splits = {TC.wgrad_splits(Cout, Cin, ncu) for Cout in TC.WGRAD_COUT for Cin in TC.WGRAD_CIN}
            assert splits == ({1} if lvl else {3}), (lvl, splits)       # one slab over all of T, or the cap T / 128
            seen.append(here)
    assert sorted(seen[0]) == [10 * a + b for a in (1, 2, 3, 4) for b in (1, 2, 4)]       # all twelve, once each
    assert sorted(wm for wm, _ in (divmod(TC.wgrad_instance(*c), 10) for c in TC.WGRAD_NO_DB)) == [1, 2, 3, 4]


def test_no_shape_reaches_2x4():
    """rows 1 .. 20000, widths 32 .. 1024, at 8 CUs, 9 CUs and the whole device: neither dispatcher ever answers <2,4> ((4,2) comes
    earlier in both candidate lists with at least as many blocks wherever N % 128 == 0); it runs only under the diagnostic
    DHZ_GEMM_TILE override of a DHZ_DIAG build.  Every other instance is reached."""
    lib = _lib()
    seen = {"conv fwd": set(), "conv dgrad": set(), "gemm": set()}
    for lvl in (8, 9, None):
        with reserved_grid(lvl):
            for N in range(32, 1025, 32):
                for M in range(1, 20001, 7):
                    seen["conv fwd"].add(conv_tile_mn(lib, 1, M, N))
                    seen["conv dgrad"].add(conv_tile_mn(lib, 2, M, N))
                    seen["gemm"].add(lib.dhz_linear_tile(M, N))
    for what, cand, table in (("conv fwd", TC.CONV_CAND, TC.CONV_UNREACHABLE), ("conv dgrad", TC.CONV_CAND, TC.CONV_UNREACHABLE),
                              ("gemm", TC.GEMM_CAND, TC.GEMM_UNREACHABLE)):
        every = {10 * a + b for a, b in cand}
        assert seen[what] <= every, (what, sorted(seen[what] - every))
        newly = seen[what] & set(table)
        assert not newly, (f"{what}: instance {sorted(newly)} is reachable now: a newly reachable instance needs a value case in "
                           "tests/_tile_cases.py and tests/test_gpu_tile_instances.py")
        assert seen[what] == every - set(table), (what, sorted(every - set(table) - seen[what]))


def test_deterministic_mode_answers_as_the_whole_device():
    """in deterministic mode a tile choice is a function of the shape: the answer at any reservation is the 256-CU one"""
    from dehaze_hip import _lib as L
    lib = L.load()
    shapes = [(M, N) for M in TC.GEMM_ROWS + (100000, 300000) for N in (32, 64, 96, 128, 256)]

    def answers():
        return [(conv_tile_mn(lib, 1, M, N), conv_tile_mn(lib, 2, M, N), lib.dhz_linear_tile(M, N)) for M, N in shapes]

    assert lib.dhz_get_deterministic() == 0
    whole = answers() if physical_cus() == 256 else None
    try:
        L.call("dhz_set_deterministic", 1)
        det = answers()
        for lvl in TC.RESERVED:
            with reserved_grid(lvl):
                assert answers() == det, lvl
    finally:
        L.call("dhz_set_deterministic", 0)
    if whole is not None:
        assert det == whole
    with reserved_grid(8):
        assert answers() != det                 # ... and out of the mode the reservation does change them
