"""CPU-side checks of FFA-Net's recipe on whole images (csrc/winograd_conv.hip: the poolings on any map size; csrc/elementwise.hip: the L1
mean on any element count; csrc/data_feed.hip: the h x w feed; dehaze_hip/vgg.py, perceptual.py, dataset.py, FFA_main.py): the new entries are
declared, exported, bound and refuse bad arguments without a device; the gate of the VGG16 engine; the augmentation table of a non-square
crop."""
import os
import random
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
ENTRIES = (("dhz_maxpool2x2_blocked_fwd_any", 6), ("dhz_maxpool2x2_blocked_bwd_any", 7), ("dhz_maxpool2x2_blocked_bwd_add_any", 8),
           ("dhz_l1_pair_fwd_any", 6), ("dhz_l1_pair_bwd_any", 7), ("dhz_crop_augment_pair_rect", 11))


def test_entries_are_declared_exported_and_bound():
    from dehaze_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    for name, nargs in ENTRIES:
        m = re.search(r"\bint %s\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in include/dehaze_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)
    # the entries they extend keep their signatures
    for name in ("dhz_maxpool2x2_blocked_fwd", "dhz_maxpool2x2_blocked_bwd", "dhz_maxpool2x2_blocked_bwd_add", "dhz_l1_pair_fwd",
                 "dhz_l1_pair_bwd"):
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name + "_any"], name


def refused(lib, rc):
    assert rc == EINVAL, rc
    msg = lib.dhz_last_error()
    assert msg and len(msg) > 0
    return msg


def test_poolings_refuse_maps_without_a_window_and_bad_pointers_without_a_device():
    from dehaze_hip import _lib
    lib = _lib.load()
    A, G, S, D = 4096, 8192, 12288, 16384                    # 16-byte aligned stand-ins: nothing is launched, nothing is read
    for H, W in ((1, 8), (8, 1), (1, 1), (0, 4), (4, -2)):
        assert b"H, W >= 2" in refused(lib, lib.dhz_maxpool2x2_blocked_fwd_any(A, G, 4, H, W, None))
        assert b"H, W >= 2" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_any(A, G, D, 4, H, W, None))
        assert b"H, W >= 2" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_add_any(A, G, S, D, 4, H, W, None))
    assert b"N > 0" in refused(lib, lib.dhz_maxpool2x2_blocked_fwd_any(A, G, 0, 5, 5, None))
    assert b"null" in refused(lib, lib.dhz_maxpool2x2_blocked_fwd_any(A, None, 4, 5, 5, None))
    assert b"null" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_any(A, None, D, 4, 5, 5, None))
    assert b"null" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_add_any(A, G, None, D, 4, 5, 5, None))
    assert b"aligned" in refused(lib, lib.dhz_maxpool2x2_blocked_fwd_any(A + 4, G, 4, 5, 5, None))
    assert b"aligned" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_any(A, G, D + 8, 4, 5, 5, None))
    assert b"aligned" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_add_any(A, G, S + 4, D, 4, 5, 5, None))
    assert b"too large" in refused(lib, lib.dhz_maxpool2x2_blocked_bwd_any(A, G, D, 1 << 30, 1 << 12, 1 << 12, None))
    # the even-only entries are what they were
    assert lib.dhz_maxpool2x2_blocked_fwd(A, G, 4, 15, 16, None) == EINVAL


def test_l1_any_refuses_an_empty_count_and_bad_pointers_without_a_device():
    from dehaze_hip import _lib
    lib = _lib.load()
    A, P, S, D = 4096, 8192, 12288, 16384
    for count in (0, -3):
        assert b"positive" in refused(lib, lib.dhz_l1_pair_fwd_any(A, P, None, S, count, None))
        assert b"positive" in refused(lib, lib.dhz_l1_pair_bwd_any(A, P, None, S, D, count, None))
    assert b"null" in refused(lib, lib.dhz_l1_pair_fwd_any(None, P, None, S, 5, None))
    assert b"null" in refused(lib, lib.dhz_l1_pair_fwd_any(A, P, None, None, 5, None))
    assert b"null" in refused(lib, lib.dhz_l1_pair_bwd_any(A, P, None, S, None, 5, None))
    assert b"4-byte" in refused(lib, lib.dhz_l1_pair_fwd_any(A + 2, P, None, S, 5, None))
    assert b"4-byte" in refused(lib, lib.dhz_l1_pair_bwd_any(A, P, None, S, D + 1, 5, None))
    # the entry it extends still wants multiples of 4
    assert lib.dhz_l1_pair_fwd(A, P, None, S, 10, None) == EINVAL and b"multiple of 4" in lib.dhz_last_error()


def test_rect_feed_refuses_bad_sizes_without_a_device():
    from dehaze_hip import _lib
    lib = _lib.load()
    for h, w in ((11, 14), (10, 15), (0, 4), (4, 0)):
        assert b"bad sizes" in refused(lib, lib.dhz_crop_augment_pair_rect(8, 8, 8, 8, 8, 3, 10, 14, h, w, None))
    assert b"bad sizes" in refused(lib, lib.dhz_crop_augment_pair_rect(8, 8, 8, 8, 8, 0, 10, 14, 6, 9, None))
    assert b"null" in refused(lib, lib.dhz_crop_augment_pair_rect(8, 8, None, 8, 8, 3, 10, 14, 6, 9, None))


def test_engine16_gates():
    from dehaze_hip import vgg
    for hw in ((32, 32), (33, 38), (40, 64), (460, 620), (413, 550)):
        assert vgg.engine16_any_shape_ok(*hw), hw
    for hw in ((24, 40), (31, 64), (64, 31)):
        assert not vgg.engine16_any_shape_ok(*hw), hw
    # engine16_shape_ok is what it was (tests/test_perloss_host.py pins the same pairs)
    assert vgg.engine16_shape_ok(32, 32) and vgg.engine16_shape_ok(48, 80) and vgg.engine16_shape_ok(240, 240)
    assert not vgg.engine16_shape_ok(16, 32) and not vgg.engine16_shape_ok(24, 40) and not vgg.engine16_shape_ok(40, 64)
    assert not vgg.engine16_shape_ok(33, 38) and not vgg.engine16_shape_ok(460, 620)
    # the contrastive loss's gate does not move: whole images do not reach it
    assert not vgg.engine_shape_ok(460, 620) and not vgg.engine_shape_ok(72, 64) and vgg.engine_shape_ok(64, 64)


def test_the_switch_is_a_module_attribute_read_from_the_environment():
    import subprocess
    import sys
    from dehaze_hip import perceptual
    assert perceptual.ANY is True
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(perceptual.__file__)))
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); from dehaze_hip import perceptual; print(perceptual.ANY)",
                          pkg], env=dict(os.environ, DHZ_PERLOSS_ANY="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "False", out.stdout + out.stderr


def test_pool_wrappers_pick_the_any_entries_on_odd_maps_only():
    from dehaze_hip import vgg
    assert vgg._pool_sfx(12, 20) == "" and vgg._pool_sfx(230, 310) == ""
    assert vgg._pool_sfx(115, 155) == "_any" and vgg._pool_sfx(115, 154) == "_any" and vgg._pool_sfx(114, 155) == "_any"


def test_rect_table_draws_like_the_square_one_and_masks_k():
    """h == w: draw_crop_aug's own draws.  h != w: as many draws, k & 6.  Whole image: no numpy draw, r = c = 0."""
    import dataset
    for seed in range(8):
        np.random.seed(seed); random.seed(seed)
        sq = [dataset.draw_crop_aug(10, 14, 6) for _ in range(5)]
        st_np, st_py = np.random.get_state()[1].copy(), random.getstate()
        np.random.seed(seed); random.seed(seed)
        assert [dataset.draw_rect_aug(10, 14, 6, 6) for _ in range(5)] == sq
        np.random.seed(seed); random.seed(seed)
        rc = [dataset.draw_rect_aug(10, 14, 6, 9) for _ in range(5)]
        assert np.array_equal(np.random.get_state()[1], st_np) and random.getstate() == st_py          # the same number of draws
        random.seed(seed)
        raw = [random.getrandbits(3) for _ in range(5)]
        assert [k for _, _, k in rc] == [k & 6 for k in raw]
        assert all(k in (0, 2, 4, 6) and 0 <= r <= 10 - 6 and 0 <= c <= 14 - 9 for r, c, k in rc)
    np.random.seed(3); random.seed(3)
    before = np.random.get_state()[1].copy()
    whole = [dataset.draw_rect_aug(10, 14, 10, 14) for _ in range(20)]
    assert np.array_equal(np.random.get_state()[1], before)
    assert all(r == 0 and c == 0 and k in (0, 2, 4, 6) for r, c, k in whole) and {k for _, _, k in whole} == {0, 2, 4, 6}
    # an axis without room: still two draws, the crop stays inside
    np.random.seed(4); random.seed(4)
    assert all(r == 0 and 0 <= c <= 5 for r, c, _ in (dataset.draw_rect_aug(10, 14, 10, 9) for _ in range(20)))


def test_batch_refuses_a_crop_larger_than_the_store():
    import torch
    import dataset
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (3, 10, 14, 3), generator=g, dtype=torch.uint8)
    store = dataset.PatchStoreHBM(u8, u8.clone(), "cpu")
    for size in ((11, 14), (10, 15), (0, 3)):
        with pytest.raises(ValueError, match="does not fit"):
            store.batch([0, 1], size)


def test_ffa_main_whole_img_options():
    import FFA_main
    opt = FFA_main.parse([])
    assert opt.whole_img is False and opt.crop is False and opt.crop_size == 240          # today's behaviour without the option
    assert (opt.height, opt.width) == (460, 620)
    opt = FFA_main.parse(["--whole_img", "--synthetic", "4", "--height", "35", "--width", "50"])
    assert opt.whole_img and (opt.height, opt.width) == (35, 50)
    assert "data_utils.py:21" in FFA_main.__doc__ and "--whole_img" in FFA_main.__doc__
