"""CPU: the two dispatch rules of the channel-sliced Winograd launches (dehaze_hip.vgg.f43_slices_rule, wino_slices_rule - the latter the
statement of the library's dhz_winograd_slices) on the training step's layers, and the declarations of the new entries."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dhz_winograd_conv3x3_slices", "dhz_winograd43_conv3x3_slices", "dhz_winograd_slices")


def _side(V, i, patch=128):
    return patch >> sum(1 for p in V.POOL_AFTER if p < i)


def _f43_rule(B, H, C, K, cus):
    """use_f43's rule at a given CU count (the function itself asks the library for the count)"""
    if H < 16 or C % 16 or K % 32:
        return False
    wgs = (B * (H // 16) ** 2 + 3) // 4 * (K // 32)
    return wgs >= 0.92 * ((wgs + cus - 1) // cus) * cus


def _launches(V):
    """(name, B, H, C, K) of the step's 13 layers x {32 differentiated, 64 reference images}, backward-data products of the 32 included"""
    for i in range(13):
        (C, K), H = V.CONVS[i], _side(V, i)
        yield f"conv{i} forward", 32, H, C, K
        yield f"conv{i} no-grad", 64, H, C, K
        yield f"conv{i} dgrad", 32, H, K, C


@pytest.mark.parametrize("cus", [256, 248])
def test_slice_rules_on_the_step_layers(cus):
    from dehaze_hip import vgg as V
    chosen = {}
    for name, B, H, C, K in _launches(V):
        if C % 8 or K % 32:                      # conv 0 (3 channels) runs the thin kernels
            continue
        s43 = V.f43_slices_rule(B, H, H, C, K, cus)
        s22 = V.wino_slices_rule(B, H, H, C, K, cus)
        assert s43 in (0, 2, 4) and s22 in (1, 2, 4)
        if s43:
            assert not _f43_rule(B, H, C, K, cus), name                        # never where use_f43 fires
            wgs = (B * (H // 16) ** 2 + 3) // 4 * (K // 32)
            assert 0.92 * cus <= s43 * wgs <= cus, name                        # one round, nearly full, never more than the CUs
            assert (C // 8) % s43 == 0 and C // 8 // s43 <= 32, name           # equal slices of one accumulation chain at the most
            assert C // 8 // s43 >= V.SLICE_MIN_GROUPS, name
        if s22 > 1:
            nblk = (B + 3) // 4 if H == 8 else B * (H // 16) ** 2
            assert s22 * ((nblk + 1) // 2) * (K // 32) <= cus, name
            assert C // 8 // s22 >= V.SLICE_MIN_GROUPS, name
            if s22 < 4:                                                        # the largest S that fits
                assert 2 * s22 * ((nblk + 1) // 2) * (K // 32) > cus or C // 8 // (2 * s22) < V.SLICE_MIN_GROUPS, name
        if s43 or s22 > 1:
            chosen[name] = (s43, s22)
    if cus == 256:
        # the under-filled launches of the step: conv5_1 (conv 12, 8 x 8 maps) on F(2x2) slices; the 16 x 16 layers of the 32 images, where
        # F(4x4) is refused for half a round, as two (conv4_1 backward-data, a quarter round: four) parallel chain links
        assert chosen["conv12 no-grad"] == (0, 2) and chosen["conv12 forward"] == (0, 4) and chosen["conv12 dgrad"] == (0, 4)
        for i in (8, 9, 10, 11):
            assert chosen[f"conv{i} forward"][0] == 2, i
        for i in (9, 10, 11):
            assert chosen[f"conv{i} dgrad"][0] == 2, i
        assert chosen["conv8 dgrad"] == (4, 2)          # F(4x4) in four links comes first; the F(2x2) rule alone would cut it in two
        assert not any(n.endswith("no-grad") and n != "conv12 no-grad" for n in chosen)      # the 64 images fill the CUs everywhere else
    else:
        # 248 CUs: the 128- and 256-workgroup grids of the 16 x 16 layers no longer fit one round - no F(4x4) links; conv5_1 keeps its slices
        assert all(s43 == 0 for s43, _ in chosen.values()), chosen
        assert chosen["conv12 forward"][1] >= 2 and chosen["conv12 dgrad"][1] >= 2


def test_library_query_is_the_stated_rule():
    from dehaze_hip import _lib, vgg as V
    lib = _lib.load()
    cus = lib.dhz_grid_cus() + lib.dhz_get_reserved_cus()
    for name, B, H, C, K in _launches(V):
        if C % 8 or K % 32:
            assert lib.dhz_winograd_slices(B, H, H, C, K) == 1
            continue
        assert lib.dhz_winograd_slices(B, H, H, C, K) == V.wino_slices_rule(B, H, H, C, K, cus), name
    assert lib.dhz_winograd_slices(0, 16, 16, 64, 64) == 1 and lib.dhz_winograd_slices(4, 24, 24, 64, 64) == 1


def test_sliced_entries_refuse_bad_arguments_without_gpu():
    from dehaze_hip import _lib
    lib = _lib.load()
    one = 16          # any non-null pointer: the checks come before any launch
    assert lib.dhz_winograd_conv3x3_slices(one, one, None, 0, None, None, one, one, 9, 1, 16, 16, 64, 64, None) == -22      # > C / 8
    assert lib.dhz_winograd_conv3x3_slices(one, one, None, 0, None, None, one, None, 2, 1, 16, 16, 64, 64, None) == -22     # no workspace
    assert lib.dhz_winograd_conv3x3_slices(one, one, None, 0, None, None, one, one, 0, 1, 16, 16, 64, 64, None) == -22
    assert lib.dhz_winograd43_conv3x3_slices(one, one, None, 0, None, None, one, None, 2, 1, 16, 16, 64, 64, None) == -22
    assert lib.dhz_winograd43_conv3x3_slices(one, one, None, 0, None, None, one, one, 1, 1, 16, 16, 64, 64, None) == -22
    assert lib.dhz_winograd43_conv3x3_slices(one, one, None, 0, None, None, one, one, 3, 1, 16, 16, 64, 64, None) == -22    # 8 groups % 3
    assert lib.dhz_winograd43_conv3x3_slices(one, one, None, 0, None, None, one, one, 2, 1, 16, 16, 1024, 64, None) == -22  # 64 groups per link
    assert lib.dhz_winograd43_conv3x3_slices(one, one, None, 0, None, None, one, one, 2, 1, 8, 8, 64, 64, None) == -22


def test_new_entries_are_declared_and_prototyped():
    from dehaze_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dehaze_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib._PROTOS if hasattr(_lib, "_PROTOS") else True
        assert hasattr(lib, name), name
    assert len(getattr(lib, "dhz_winograd_conv3x3_slices").argtypes) == 15
    assert len(getattr(lib, "dhz_winograd43_conv3x3_slices").argtypes) == 15
    assert len(getattr(lib, "dhz_winograd_slices").argtypes) == 5
