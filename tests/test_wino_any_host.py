"""CPU: the any-size entries of the F(2x2,3x3) Winograd convolution (dhz_winograd_conv3x3_any, _any_slices, dhz_winograd_slices_any,
dhz_winograd_any_blocks) - declarations, argument checks, the block count and the slice rule against their Python restatements in
dehaze_hip.vgg - and the image sizes the fp32 feature engine takes (vgg.engine_shape_ok)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"dhz_winograd_conv3x3_any": 13, "dhz_winograd_conv3x3_any_slices": 15, "dhz_winograd_slices_any": 5, "dhz_winograd_any_blocks": 3}

# (B, C, K, H, W) of tests/test_gpu_wino_any.py: ragged, packed 4, old-entry shapes, sliced
GPU_CASES = [(2, 32, 64, 24, 24), (1, 64, 32, 12, 12), (3, 32, 32, 40, 24), (1, 32, 32, 15, 15), (2, 32, 32, 30, 30), (1, 32, 64, 2, 2),
             (1, 32, 32, 1, 1), (1, 32, 32, 17, 33),
             (16, 32, 32, 4, 4), (5, 32, 32, 4, 4), (1, 32, 32, 4, 4), (17, 32, 32, 4, 4), (33, 32, 32, 4, 4), (3, 128, 64, 4, 4),
             (2, 64, 64, 32, 32), (5, 32, 64, 8, 8), (2, 32, 64, 16, 32),
             (6, 512, 512, 4, 4), (2, 512, 512, 24, 24), (2, 320, 32, 12, 12)]


def _lib_and_last_error():
    from dehaze_hip import _lib
    lib = _lib.load()
    return lib, lambda: lib.dhz_last_error().decode()


def test_entries_are_declared_and_exported():
    from dehaze_hip import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dehaze_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name             # the header's prototype ...
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name        # ... and the binding's
    # the entries of the same name without `_any` have the same argument lists
    assert _lib.SIGNATURES["dhz_winograd_conv3x3_any"] == _lib.SIGNATURES["dhz_winograd_conv3x3"]
    assert _lib.SIGNATURES["dhz_winograd_conv3x3_any_slices"] == _lib.SIGNATURES["dhz_winograd_conv3x3_slices"]
    assert _lib.SIGNATURES["dhz_winograd_slices_any"] == _lib.SIGNATURES["dhz_winograd_slices"]


def test_any_entries_refuse_bad_arguments_without_gpu():
    lib, err = _lib_and_last_error()
    one = 16          # any non-null pointer: the checks come before any launch
    conv, sl = lib.dhz_winograd_conv3x3_any, lib.dhz_winograd_conv3x3_any_slices
    for x, up, y in ((None, one, one), (one, None, one), (one, one, None)):
        assert conv(x, up, None, 0, None, None, y, 1, 24, 24, 64, 64, None) == -22
        assert err() == "dhz_winograd_conv3x3_any: null pointer"
        assert sl(x, up, None, 0, None, None, y, None, 1, 1, 24, 24, 64, 64, None) == -22
        assert err() == "dhz_winograd_conv3x3_any_slices: null pointer"
    for B, H, W, C, K in ((1, 24, 24, 60, 64), (1, 24, 24, 64, 48), (1, 0, 24, 64, 64), (1, 24, 0, 64, 64), (1, -3, 4, 64, 64),
                          (0, 24, 24, 64, 64), (1, 4, 4, 4, 32)):
        assert conv(one, one, None, 0, None, None, one, B, H, W, C, K, None) == -22, (B, H, W, C, K)
        assert err() == f"dhz_winograd_conv3x3_any: unsupported shape B={B} H={H} W={W} C={C} K={K}"
        assert sl(one, one, None, 0, None, None, one, one, 2, B, H, W, C, K, None) == -22, (B, H, W, C, K)
        assert err() == f"dhz_winograd_conv3x3_any_slices: unsupported shape B={B} H={H} W={W} C={C} K={K}"
    # bias / ReLU together with the backward epilogue
    assert conv(one, one, one, 0, one, None, one, 1, 24, 24, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3_any: bias/relu and out_mask/out_addend are exclusive"
    assert conv(one, one, None, 1, None, one, one, 1, 4, 4, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3_any: bias/relu and out_mask/out_addend are exclusive"
    # slices: more than one needs a workspace; 1 .. C / 8
    assert sl(one, one, None, 0, None, None, one, None, 2, 1, 24, 24, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3_any_slices: slices=2 of 8 channel groups, workspace null"
    assert sl(one, one, None, 0, None, None, one, one, 9, 1, 4, 4, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3_any_slices: slices=9 of 8 channel groups, workspace given"
    assert sl(one, one, None, 0, None, None, one, one, 0, 1, 15, 15, 64, 64, None) == -22
    # the entries without `_any` keep their contract: the sizes only the new entries take stay refused there, with the old message
    assert lib.dhz_winograd_conv3x3(one, one, None, 0, None, None, one, 1, 24, 24, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3: unsupported shape B=1 H=24 W=24 C=64 K=64"
    assert lib.dhz_winograd_conv3x3(one, one, None, 0, None, None, one, 1, 4, 4, 64, 64, None) == -22
    assert lib.dhz_winograd_conv3x3_slices(one, one, None, 0, None, None, one, one, 2, 1, 4, 4, 64, 64, None) == -22
    assert err() == "dhz_winograd_conv3x3_slices: unsupported shape B=1 H=4 W=4 C=64 K=64"
    assert lib.dhz_winograd_slices(64, 4, 4, 512, 512) == 1 and lib.dhz_winograd_slices(4, 24, 24, 512, 512) == 1


def test_block_count_is_the_stated_rule():
    from dehaze_hip import vgg as V
    lib, _ = _lib_and_last_error()
    grid = [(B, H, W) for B in (1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 64, 96) for H in (1, 2, 3, 4, 8, 12, 15, 16, 17, 24, 30, 32, 33, 40, 48)
            for W in (1, 2, 4, 8, 12, 15, 16, 17, 24, 30, 33)]
    grid += [(B, H, W) for B, _, _, H, W in GPU_CASES]
    for B, H, W in grid:
        assert lib.dhz_winograd_any_blocks(B, H, W) == V.any_blocks(B, H, W) > 0, (B, H, W)
    # the three forms, spelled out
    assert lib.dhz_winograd_any_blocks(33, 4, 4) == 3 and lib.dhz_winograd_any_blocks(16, 4, 4) == 1
    assert lib.dhz_winograd_any_blocks(5, 8, 8) == 2
    assert lib.dhz_winograd_any_blocks(3, 40, 24) == 3 * 3 * 2 and lib.dhz_winograd_any_blocks(1, 17, 33) == 2 * 3
    assert lib.dhz_winograd_any_blocks(2, 32, 48) == 2 * 2 * 3            # multiples of 16: the old entry's count
    assert lib.dhz_winograd_any_blocks(7, 4, 8) == 7                      # only 4 x 4 and 8 x 8 are packed
    for bad in ((0, 4, 4), (-1, 16, 16), (1, 0, 16), (1, 16, 0), (1, -4, 4)):
        assert lib.dhz_winograd_any_blocks(*bad) <= 0 and V.any_blocks(*bad) == 0, bad
    assert lib.dhz_winograd_any_blocks(1 << 20, 1 << 12, 1 << 12) <= 0    # more blocks than a grid holds


def _any_launches(V):
    """(B, H, W, C, K) of the feature stack's Winograd layers at the patch sizes the engine newly takes: differentiated images, the
    reference pair, backward-data products"""
    for patch, B in (((64, 64), 32), ((64, 64), 3), ((192, 192), 8), ((240, 240), 1), ((384, 384), 2), ((64, 192), 4)):
        for i in range(1, 13):
            (C, K), d = V.CONVS[i], sum(1 for p in V.POOL_AFTER if p < i)
            H, W = patch[0] >> d, patch[1] >> d
            yield B, H, W, C, K
            yield 2 * B, H, W, C, K
            yield B, H, W, K, C


@pytest.mark.parametrize("cus", [256, 248])
def test_slice_rule_any_restated(cus):
    """the restatement itself: S copies of the grid fit the CUs, every slice keeps SLICE_MIN_GROUPS groups, and S is the largest such"""
    from dehaze_hip import vgg as V
    sliced = 0
    for B, H, W, C, K in list(_any_launches(V)) + [(B, H, W, C, K) for B, C, K, H, W in GPU_CASES]:
        S = V.wino_slices_any_rule(B, H, W, C, K, cus)
        assert S in (1, 2, 4)
        grid = (V.any_blocks(B, H, W) + 1) // 2 * (K // 32)
        if S > 1:
            sliced += 1
            assert S * grid <= cus and C // 8 // S >= V.SLICE_MIN_GROUPS
        if S < 4:
            assert 2 * S * grid > cus or C // 8 // (2 * S) < V.SLICE_MIN_GROUPS
        if V._fixed_tiling(H, W):                         # shapes both rules take: one answer
            assert S == V.wino_slices_rule(B, H, W, C, K, cus)
    assert sliced
    # conv5_1 of 64-pixel patches, batch 32: 64 / 32 images of 4 x 4 are 4 / 2 blocks = 2 / 1 workgroups per 32 output channels
    assert V.wino_slices_any_rule(64, 4, 4, 512, 512, cus) == 4 and V.wino_slices_any_rule(32, 4, 4, 512, 512, cus) == 4
    # 384-pixel patches, batch 2: 8 blocks = 64 workgroups, four copies of which are exactly 256
    assert V.wino_slices_any_rule(2, 24, 24, 512, 512, cus) == (4 if cus == 256 else 2)
    assert V.wino_slices_any_rule(16, 24, 24, 512, 512, cus) == 1         # 64 blocks x 16 channel blocks fill the CUs
    assert V.wino_slices_any_rule(2, 24, 24, 64, 64, cus) == 1            # 8 channel groups: nothing to cut


def test_library_slice_query_is_the_stated_rule():
    from dehaze_hip import vgg as V
    lib, _ = _lib_and_last_error()
    cus = lib.dhz_grid_cus() + lib.dhz_get_reserved_cus()
    for B, H, W, C, K in list(_any_launches(V)) + [(B, H, W, C, K) for B, C, K, H, W in GPU_CASES]:
        assert lib.dhz_winograd_slices_any(B, H, W, C, K) == V.wino_slices_any_rule(B, H, W, C, K, cus), (B, H, W, C, K)
    for bad in ((0, 4, 4, 512, 512), (1, 0, 4, 512, 512), (1, 4, 4, 508, 512), (1, 4, 4, 512, 48), (1, 24, 24, 0, 512)):
        assert lib.dhz_winograd_slices_any(*bad) == 1, bad


def test_engine_shape_ok():
    from dehaze_hip import vgg as V
    for n in (64, 128, 192, 240, 256, 384):
        assert V.engine_shape_ok(n, n), n
    assert V.engine_shape_ok(64, 192) and V.engine_shape_ok(192, 64)
    for n in (16, 32, 48, 72, 100, 0):
        assert not V.engine_shape_ok(n, n), n
    assert not V.engine_shape_ok(64, 40) and not V.engine_shape_ok(40, 64) and not V.engine_shape_ok(64, 72)


def test_engine_gate_follows_engine_shape_ok():
    """Vgg19.engine_for's shape test is engine_shape_ok for the fp32 engine and stays multiples of 128 for the bf16 one (read from the
    source: building an engine needs a GPU tensor)"""
    import inspect
    import My_CR
    src = inspect.getsource(My_CR.Vgg19.engine_for)
    assert "engine_shape_ok(X.shape[2], X.shape[3])" in src
    assert "X.shape[2] % 128 or X.shape[3] % 128" in src
    from dehaze_hip import vgg as V
    assert not hasattr(V, "wino_supported")                 # no admitted shape reaches a library tail any more
