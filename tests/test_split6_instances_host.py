"""No GPU: which kernel of csrc/split6_gemm.hip a shape gets, asked of the library itself (dhz_linear_split6_tile: the function the
dispatch calls), at the five levels tests/test_gpu_split6_instances.py runs at.  The table of tests/_tile_cases.py selects what it
claims; its union is every instance a shape can reach; and per kernel instantiation - (tile, mode), eleven in all - the cases meet
the conditions that make the value tests bite:
  (c) three trips and more with a ragged last trip and a ragged last row tile (44 outside deterministic mode: two, see the trip rule);
  (d) 1, 2, 3, 5, 6 and 7 stages per tile, and a later tile of workgroup 0 beginning at every stream position mod 6 (mod 2: the wide kernel);
  (e) six trips and more with one and with two stages per tile (the four-stage look-ahead spans several tile boundaries);
  (f) the XCD remap on, and off;
  (g) more than one column tile, with a workgroup that changes column tile between trips.
Last, float64 alone: the bound of the value tests rejects a result that lacks one 32-deep stage."""
import os
import re

import torch

from _grid import physical_cus
import _tile_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dhz_linear_split6_tile"
INSTANTIATIONS = tuple((i, m) for i in TC.S6_INSTANCES for m in TC.S6_MODES if (i, m) != (41, "dgrad"))


def _lib():
    from dehaze_hip import _lib as L
    return L.load()


def _cases():
    """every (instance, mode, T, features, contraction, grid CUs, deterministic) the value tests run at the tabled levels, by the library"""
    lib = _lib()
    out = []
    for (ncu, det) in TC.S6_TABLED:
        with TC.s6_level(ncu, det):
            for (T, F) in TC.S6_TABLE:
                for mode in TC.s6_modes(F):
                    for KC in TC.S6_CONTRACTIONS:
                        out.append((TC.s6_query(lib, mode, T, F, KC), mode, T, F, KC, ncu, det))
    return out


def test_entry_declared_exported_bound():
    from dehaze_hip import _lib as L
    TC.s6_no_override()
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    assert re.search(r"\bint %s\s*\(" % NAME, header), f"{NAME} is not declared in include/dehaze_hip.h"
    assert NAME in L.SIGNATURES and getattr(L.load(), NAME).argtypes == L.SIGNATURES[NAME]
    assert L.load().dhz_abi_version() == 1
    assert len(INSTANTIATIONS) == 11


def test_query_answers_zero_where_the_dispatch_refuses():
    TC.s6_no_override()
    q = _lib().dhz_linear_split6_tile
    assert q(1, 100, 64, 32) > 0 and q(2, 100, 32, 64) > 0
    for mode in (0, 3, -1):
        assert q(mode, 100, 64, 64) == 0, mode
    for mode in (1, 2):
        for bad in [(0, 64, 64), (-5, 64, 64), (100, 0, 64), (100, 64, 0), (100, -64, 64), (100, 64, -64),
                    (100, 48, 64), (100, 64, 48), (100, 16, 64), (100, 64, 16)]:
            assert q(mode, *bad) == 0, (mode, bad)
    # features: a multiple of 32 (forward: w's rows) or of 64 (backward-data: w's columns); the contraction a multiple of 32
    assert q(1, 100, 96, 64) == 41 and q(2, 100, 64, 96) == 0
    assert q(1, 100, 64, 96) > 0 and q(2, 100, 96, 64) > 0
    # at most 2048 features (the bias vector is staged in LDS); the contraction has no such bound
    assert q(1, 100, 2048, 64) > 0 and q(1, 100, 2048 + 32, 64) == 0 and q(1, 100, 64, 4096) > 0
    assert q(2, 100, 64, 2048) > 0 and q(2, 100, 64, 2048 + 64) == 0 and q(2, 100, 4096, 64) > 0
    # the weight matrix has fewer than 2^31 elements
    assert q(1, 100, 2048, 2 ** 20 - 32) > 0 and q(1, 100, 2048, 2 ** 20) == 0
    assert q(2, 100, 2 ** 20 - 32, 2048) > 0 and q(2, 100, 2 ** 20, 2048) == 0
    # mode 2 answers for K output features: the same shape as the forward of the transposed weight
    with TC.s6_level(8, False):
        for T, F in TC.S6_TABLE:
            if F % 64 == 0:
                assert q(2, T, 96, F) == q(1, T, F, 96), (T, F)


def test_table_selects_what_it_claims():
    """(a) every row, every mode and contraction, at the four tabled levels: the instance by the query, the trips from that instance"""
    TC.s6_no_override()
    lib = _lib()
    for k, (ncu, det) in enumerate(TC.S6_TABLED):
        with TC.s6_level(ncu, det) as n:
            assert n == ncu
            for (T, F), claims in TC.S6_TABLE.items():
                inst, trips = claims[k]
                for mode in TC.s6_modes(F):
                    for KC in TC.S6_CONTRACTIONS:
                        got = TC.s6_query(lib, mode, T, F, KC)
                        assert got == inst, (T, F, mode, KC, ncu, det, got)        # a function of (T, features) alone
                assert TC.s6_plan(inst, T, F, ncu)[2] == trips, (T, F, ncu, det, TC.s6_plan(inst, T, F, ncu))
                assert T <= TC.S6_MAX[0] and F <= TC.S6_MAX[1] and max(TC.S6_CONTRACTIONS) <= TC.S6_MAX[2]
    # the cases the table's comments describe
    assert TC.s6_plan(84, 7000, 128, 8) == (28, 8, 4, False) and 28 % 8 == 4 and 7000 % 256 == 88
    assert TC.s6_plan(84, 8100, 128, 8) == (32, 8, 4, True) and TC.s6_plan(84, 7104, 256, 8) == (56, 8, 7, True)
    assert TC.s6_plan(84, 7104, 256, 9) == (56, 9, 7, False) and 56 % 9 == 2
    assert TC.s6_plan(44, 7000, 128, 8) == (55, 8, 7, False) and TC.s6_plan(44, 3520, 128, 9) == (28, 9, 4, False)
    assert TC.s6_plan(44, 3072, 128, 8) == (24, 8, 3, True) and TC.s6_plan(44, 1728, 128, 8) == (14, 8, 2, False)
    assert TC.s6_plan(42, 704, 128, 8) == (12, 8, 2, False) and TC.s6_plan(44, 704, 128, 8)[0] == 6
    assert TC.s6_plan(42, 2500, 192, 8) == (60, 8, 8, False) and TC.s6_plan(42, 2500, 192, 9) == (60, 9, 7, False)
    assert TC.s6_plan(41, 1200, 160, 8) == (50, 8, 7, False) and TC.s6_plan(41, 1200, 160, 9) == (50, 9, 6, False)
    assert TC.s6_plan(41, 3072, 32, 8) == (24, 8, 3, True) and TC.s6_plan(42, 3072, 64, 8) == (24, 8, 3, True)
    # rows that run the windowed / scaled epilogues are whole images of 64 tokens; 7104, 1728 and 3072 are whole 8 x 24 maps too
    assert sum(T % 64 == 0 for T, _ in TC.S6_TABLE) >= 9 and all(T % 192 == 0 for T in (7104, 1728, 3072))


def test_the_table_reaches_every_reachable_instantiation():
    """(b) rows 1 .. 20000, widths 32 .. 1024, both modes, the whole device, 8 and 9 CUs and deterministic mode at both: the
    instances the query ever answers are those of the table, mode by mode - none is missing, none is new"""
    TC.s6_no_override()
    q = _lib().dhz_linear_split6_tile
    seen = {1: set(), 2: set()}
    for (ncu, det) in TC.S6_LEVELS:
        with TC.s6_level(ncu, det):
            for F in range(32, 1025, 32):
                for T in range(1, 20001, 7):
                    seen[1].add(q(1, T, F, 64))
                    seen[2].add(q(2, T, 64, F))
    assert seen[1] == set(TC.S6_INSTANCES), sorted(seen[1])
    assert seen[2] == {0, 84, 44, 42}, sorted(seen[2])                         # 0: widths that are no multiple of 64
    table = {(inst, mode) for inst, mode, *_ in _cases()}
    assert table == set(INSTANTIATIONS), sorted(set(INSTANTIATIONS) ^ table)


def test_conditions_hold_per_instantiation():
    """(c) .. (g) of the module docstring, from s6_plan / s6_stream and the stage count, for each of the eleven instantiations"""
    TC.s6_no_override()
    cases = _cases()
    for inst, mode in INSTANTIATIONS:
        mine = [c[2:] for c in cases if c[:2] == (inst, mode)]
        assert mine, (inst, mode)
        bm = 32 * (inst // 10)
        trips_ragged = {False: 0, True: 0}        # deterministic? -> most trips with a ragged last trip and a ragged last row tile
        residues, nsts, remap, long_short, col_change = set(), set(), set(), set(), False
        for T, F, KC, ncu, det in mine:
            ntiles, grid, trips, on = TC.s6_plan(inst, T, F, ncu)
            nst = KC // 32
            nsts.add(nst)
            remap.add(on)
            if ntiles % grid and T % bm:
                trips_ragged[det] = max(trips_ragged[det], trips)
            mine0 = TC.s6_stream(inst, T, F, ncu, 0)
            assert len(mine0) == trips
            residues |= {(j * nst) % 6 for j in range(1, trips)}            # stages workgroup 0 has completed when its tile j begins
            if nst in (1, 2) and trips >= 6:
                long_short.add(nst)
            if F // (32 * (inst % 10)) > 1 and ntiles % grid:
                col_change |= any(len({tn for _, tn in TC.s6_stream(inst, T, F, ncu, wg)}) > 1 for wg in range(grid))
        what = (inst, mode)
        if inst == 44:                                                         # the trip rule of _tile_cases
            assert trips_ragged[False] == 2 and trips_ragged[True] >= 3, (what, trips_ragged)
        else:
            assert trips_ragged[False] >= 3, (what, trips_ragged)
        assert nsts == {1, 2, 3, 5, 6, 7}, (what, sorted(nsts))
        if inst == 84:
            assert {r % 2 for r in residues} == {0, 1}, (what, sorted(residues))
        else:
            assert residues == set(range(6)), (what, sorted(residues))
        assert long_short == {1, 2}, (what, sorted(long_short))
        assert remap == {True, False}, (what, remap)
        assert col_change, what
    # 44 makes its six trips and more only in deterministic mode
    assert all(det for i, m, T, F, KC, ncu, det in cases if i == 44 and TC.s6_plan(i, T, F, ncu)[2] > 2)


def test_deterministic_mode_answers_as_the_whole_device():
    from dehaze_hip import _lib as L
    TC.s6_no_override()
    lib = L.load()

    def answers():
        return [TC.s6_query(lib, mode, T, F, 64) for (T, F) in TC.S6_TABLE for mode in TC.s6_modes(F)]

    assert lib.dhz_get_deterministic() == 0
    whole = answers() if physical_cus() == 256 else None
    with TC.s6_level(8, True):
        det = answers()
    with TC.s6_level(9, True):
        assert answers() == det
    assert lib.dhz_get_deterministic() == 0 and lib.dhz_get_reserved_cus() == 0
    if whole is not None:
        assert det == whole
    with TC.s6_level(8, False):
        assert answers() != det


def test_the_bound_rejects_a_missing_stage():
    """float64 alone: a product that lacks its last 32 contraction columns misses |err| <= 2^-21 mag + 1e-7 on most elements, with the
    operands the value tests draw"""
    for (T, F), KC in (((1216, 96), 64), ((704, 128), 160), ((1728, 128), 224)):
        x, w, b = (t.double() for t in TC.s6_operands(T, F, KC, torch.device("cpu"), seed=T + KC))
        ref = x @ w.t() + b
        mag = x.abs() @ w.abs().t() + b.abs()
        short = x[:, :KC - 32] @ w[:, :KC - 32].t() + b
        bad = ((short - ref).abs() > TC.S6_BOUND * mag + TC.S6_FLOOR).double().mean().item()
        assert bad > 0.99, (T, F, KC, bad)
