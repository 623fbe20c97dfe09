"""The training feed for pools of images of any sizes (dhz_crop_augment_pair_ragged through dataset.ImageStoreHBM) against a numpy restatement,
bit for bit: value / 255, and with `norm` (value / 255 - mean) / std, are IEEE operations in fp32 on either side.  On a store of one size
the draws and the output are PatchStoreHBM.batch's; a pool beyond 4 GiB is addressed in 64 bits; FFA_main.py trains from a RESIDE-style
folder of mixed sizes."""
import ctypes
import glob
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEAN, STD = (0.64, 0.6, 0.58), (0.14, 0.15, 0.152)
# hazy H x W / clear H x W per item; item 3 shares item 0's clear frame.  Centre-crop origins by torchvision's rule, written out:
# differences (0, 0) -> (0, 0); (3, 5) -> (2, 2); (1, 7) -> (0, 4)
SIZES = [((10, 14), (10, 14)), ((7, 9), (10, 14)), ((12, 12), (13, 19)), ((10, 14), None)]
ORIGIN = [(0, 0), (2, 2), (0, 4), (0, 0)]


def u8(rng, h, w):
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def mixed():
    """(store, hazy arrays, clear arrays already centre-cropped by EXPLICIT slices - not by the store's origin table)"""
    import dataset
    rng = np.random.RandomState(33)
    hazy = [u8(rng, *hh) for hh, _ in SIZES]
    clear = [u8(rng, *cc) for _, cc in SIZES[:3]]
    ct = [torch.from_numpy(c) for c in clear]
    store = dataset.ImageStoreHBM([(ct[0], torch.from_numpy(hazy[0])), (ct[1], torch.from_numpy(hazy[1])),
                                   (ct[2], torch.from_numpy(hazy[2])), (ct[0], torch.from_numpy(hazy[3]))], "cuda")
    cropped = [clear[0], clear[1][2:9, 2:11], clear[2][0:12, 4:16], clear[0]]
    assert [c.shape[:2] for c in cropped] == [h.shape[:2] for h in hazy]
    return store, hazy, cropped


def restate(img, r, c, k, h, w, norm=None):
    """uint8 HWC image -> float32 CHW h x w crop under map k (tests/test_gpu_feed_rect.py::restate), then ToTensor + Normalize in float32"""
    crop = np.transpose(img[r:r + h, c:c + w].astype(np.float32) / np.float32(255.0), (2, 0, 1))
    if norm is not None:
        mean, std = (np.asarray(v, dtype=np.float32).reshape(3, 1, 1) for v in norm)
        crop = (crop - mean) / std
        assert crop.dtype == np.float32
    out = np.rot90(crop, k % 4, axes=(2, 1))
    if k >= 4:
        out = out[:, ::-1, :]
    return np.ascontiguousarray(out)


def rows_of(store, table):
    """descriptor rows of (item, r, c, k) from the pool layout and the origins written out above"""
    rows = []
    for i, r, c, k in table:
        W, j = store.hazy_hw[i][1], store.clear_of[i]
        Wc = store.clear_hw[j][1]
        top, left = ORIGIN[i]
        rows.append((store.hazy_off[i] + r * W + c, W, store.clear_off[j] + (top + r) * Wc + left + c, Wc, k))
    return rows


def call_ragged(gt_pool, hazy_pool, rows, h, w, norm=None):
    """one raw launch; the outputs carry a NaN tail that must stay NaN"""
    from dehaze_hip import _lib
    desc = torch.tensor(rows, dtype=torch.int64).cuda()
    n, m = len(rows), len(rows) * 3 * h * w
    clean = torch.full((m + 64,), float("nan"), device="cuda")
    noisy = torch.full((m + 64,), float("nan"), device="cuda")
    nm = None if norm is None else (ctypes.c_float * 6)(*(norm[0] + norm[1]))
    _lib.call("dhz_crop_augment_pair_ragged", gt_pool.data_ptr(), hazy_pool.data_ptr(), desc.data_ptr(), clean.data_ptr(), noisy.data_ptr(),
              nm, n, h, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(clean[m:]).all() and torch.isnan(noisy[m:]).all(), "written past the end"
    assert not torch.isnan(clean[:m]).any() and not torch.isnan(noisy[:m]).any()
    return clean[:m].cpu().view(n, 3, h, w).numpy(), noisy[:m].cpu().view(n, 3, h, w).numpy()


def test_layout_and_center_crop_origins(mixed):
    store, _, _ = mixed
    assert store.origin == ORIGIN and store.clear_of == [0, 1, 2, 0] and store.uniform is None
    assert store.gt_pool.numel() == (2 * 10 * 14 + 13 * 19) * 3 and store.hazy_pool.numel() == (2 * 10 * 14 + 7 * 9 + 12 * 12) * 3


def test_every_map_of_a_square_crop(mixed):
    """all eight k on a 6 x 6 crop, origins chosen per item up to the last one that fits; two blocks per launch and more"""
    store, hazy, clear = mixed
    room = [(H - 6, W - 6) for H, W in store.hazy_hw]
    table = [(k % 4, (k * 3) % (room[k % 4][0] + 1), (k * 5) % (room[k % 4][1] + 1), k) for k in range(8)]
    table += [(1, 1, 3, 5), (2, 6, 6, 3), (3, 4, 8, 1)]          # the far corner of three items
    clean, noisy = call_ragged(store.gt_pool, store.hazy_pool, rows_of(store, table), 6, 6)
    for j, (i, r, c, k) in enumerate(table):
        assert np.array_equal(clean[j], restate(clear[i], r, c, k, 6, 6)), (j, i, k)
        assert np.array_equal(noisy[j], restate(hazy[i], r, c, k, 6, 6)), (j, i, k)
    assert len({clean[j].tobytes() for j in range(8)}) == 8


def test_a_non_square_crop_reads_k_and_6(mixed):
    store, hazy, clear = mixed
    table = [(k % 4, k % 3, k % 2, k) for k in range(8)]          # 5 x 8 fits every item (7 x 9: r <= 2, c <= 1)
    clean, noisy = call_ragged(store.gt_pool, store.hazy_pool, rows_of(store, table), 5, 8)
    for j, (i, r, c, k) in enumerate(table):
        assert np.array_equal(clean[j], restate(clear[i], r, c, k & 6, 5, 8)), (j, i, k)
        assert np.array_equal(noisy[j], restate(hazy[i], r, c, k & 6, 5, 8)), (j, i, k)


@pytest.mark.parametrize("h,w", [(17, 17), (20, 23), (16, 16), (3, 23)])
def test_more_than_one_block_per_item(h, w):
    """256 pixels per block: 17 x 17 and 20 x 23 take two blocks per item with a ragged last one, 16 x 16 fills one exactly"""
    rng = np.random.RandomState(h * 100 + w)
    hz = [u8(rng, 20, 23), u8(rng, 21, 27)]
    cl = [u8(rng, 21, 26), u8(rng, 21, 27)]
    gt_pool = torch.from_numpy(np.concatenate([c.reshape(-1) for c in cl])).cuda()
    hazy_pool = torch.from_numpy(np.concatenate([x.reshape(-1) for x in hz])).cuda()
    base = [(0, 0, (0, 2)), (20 * 23, 21 * 26, (0, 0))]          # hazy offset, clear offset, centre-crop origin (differences 1, 3 / 0, 0)
    table = [(k % 2, min(k % 3, hz[k % 2].shape[0] - h), min(k % 5, hz[k % 2].shape[1] - w), k) for k in range(8)]
    rows = []
    for i, r, c, k in table:
        ho, co, (top, left) = base[i]
        W, Wc = hz[i].shape[1], cl[i].shape[1]
        rows.append((ho + r * W + c, W, co + (top + r) * Wc + left + c, Wc, k))
    clean, noisy = call_ragged(gt_pool, hazy_pool, rows, h, w, (MEAN, STD))
    crop = [cl[0][0:20, 2:25], cl[1]]
    for j, (i, r, c, k) in enumerate(table):
        kk = k if h == w else k & 6
        assert np.array_equal(clean[j], restate(crop[i], r, c, kk, h, w)), (j, i, k)
        assert np.array_equal(noisy[j], restate(hz[i], r, c, kk, h, w, (MEAN, STD))), (j, i, k)


@pytest.mark.parametrize("h,w", [(6, 6), (5, 8), (7, 9)])
def test_normalisation_of_the_hazy_output_only(mixed, h, w):
    store, hazy, clear = mixed
    table = [(k % 4, 0, k % 2 if w < 9 else 0, k) for k in range(8)]
    rows = rows_of(store, table)
    clean, noisy = call_ragged(store.gt_pool, store.hazy_pool, rows, h, w, (MEAN, STD))
    plain_clean, plain_noisy = call_ragged(store.gt_pool, store.hazy_pool, rows, h, w, None)
    for j, (i, r, c, k) in enumerate(table):
        kk = k if h == w else k & 6
        assert np.array_equal(noisy[j], restate(hazy[i], r, c, kk, h, w, (MEAN, STD))), (j, i, k)
        assert np.array_equal(clean[j], restate(clear[i], r, c, kk, h, w)), (j, i, k)
        assert np.array_equal(plain_noisy[j], restate(hazy[i], r, c, kk, h, w)), (j, i, k)
    assert np.array_equal(plain_clean, clean)
    assert noisy.min() < -1 and noisy.max() > 1          # (normalised values leave [0, 1])


@pytest.mark.parametrize("ps", [6, (6, 9), (5, 5), None])
def test_batch_on_the_mixed_store(mixed, ps):
    """through the store: its own origins and descriptor rows, the draws of draw_rect_aug with each item's size"""
    import dataset
    store, hazy, clear = mixed
    idx = [0, 3, 3, 0, 0, 3] if ps is None else [2, 0, 1, 3, 1, 2, 0, 3, 3, 1, 2, 2]
    h, w = store.hazy_hw[0] if ps is None else ((ps, ps) if isinstance(ps, int) else ps)
    for norm in (None, (MEAN, STD)):
        np.random.seed(5); random.seed(5)
        clean, noisy = store.batch(idx, ps, normalize=norm)
        np.random.seed(5); random.seed(5)
        draws = [dataset.draw_rect_aug(*store.hazy_hw[i], h, w) for i in idx]
        assert clean.shape == noisy.shape == (len(idx), 3, h, w) and clean.dtype == torch.float32 and clean.is_cuda
        assert store._draws.tolist() == [[i, r, c, k] for i, (r, c, k) in zip(idx, draws)]
        assert store._table.dtype == torch.int64 and store._table.tolist() == [list(r) for r in rows_of(store, store._draws.tolist())]
        for j, (i, (r, c, k)) in enumerate(zip(idx, draws)):
            assert np.array_equal(clean[j].cpu().numpy(), restate(clear[i], r, c, k, h, w)), j
            assert np.array_equal(noisy[j].cpu().numpy(), restate(hazy[i], r, c, k, h, w, norm)), j


def test_whole_images_per_bucket_and_refusals(mixed):
    store, hazy, clear = mixed
    for i in (1, 2):
        np.random.seed(1); random.seed(1)
        clean, noisy = store.batch([i, i], None)
        random.seed(1)
        ks = [random.getrandbits(3) & (7 if i == 2 else 6) for _ in range(2)]          # whole images draw no origin
        H, W = store.hazy_hw[i]
        for j, k in enumerate(ks):
            assert np.array_equal(clean[j].cpu().numpy(), restate(clear[i], 0, 0, k, H, W)), (i, j)
            assert np.array_equal(noisy[j].cpu().numpy(), restate(hazy[i], 0, 0, k, H, W)), (i, j)
    for ids in ([0, 1], [3, 2, 3]):
        with pytest.raises(ValueError, match="different sizes"):
            store.batch(ids, None)
    for ids, ps in (([0, 1], 8), ([2, 0], 11), ([1], (7, 10)), ([0], (0, 3))):
        with pytest.raises(ValueError, match="does not fit"):
            store.batch(ids, ps)
    assert store.eligible(8, 8).tolist() == [0, 2, 3] and store.eligible(7, 9).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("ps", [6, (6, 9), None])
def test_a_uniform_store_equals_the_old_store_bit_for_bit(ps):
    import dataset
    g = torch.Generator().manual_seed(21)
    gt = torch.randint(0, 256, (3, 10, 14, 3), generator=g, dtype=torch.uint8)
    hazy = torch.randint(0, 256, (3, 10, 14, 3), generator=g, dtype=torch.uint8)
    old = dataset.PatchStoreHBM(gt, hazy, "cuda")
    new = dataset.ImageStoreHBM([(gt[i], hazy[i]) for i in range(3)], "cuda")
    assert new.uniform == (10, 14) and len(new) == len(old) == 3
    idx = [0, 1, 2, 2, 1, 0, 1, 1, 0, 2, 0, 1, 2, 0, 2, 1]
    np.random.seed(9); random.seed(9)
    c0, n0 = old.batch(idx, ps)
    after = (np.random.get_state()[1].copy(), random.getstate())
    np.random.seed(9); random.seed(9)
    c1, n1 = new.batch(idx, ps)
    assert np.array_equal(np.random.get_state()[1], after[0]) and random.getstate() == after[1]          # as many draws
    assert torch.equal(new._draws, old._table) and len(set(old._table[:, 3].tolist())) > 1
    assert c1.shape == c0.shape and torch.equal(c0.view(torch.int32), c1.view(torch.int32))
    assert torch.equal(n0.view(torch.int32), n1.view(torch.int32))


def test_pools_beyond_4_gib_are_addressed_in_64_bits():
    """one 7 x 9 / 10 x 14 pair just above byte 2^32 of two pools that are allocated, never filled"""
    if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:
        pytest.skip("less than 12 GiB of device memory free")
    rng = np.random.RandomState(7)
    hz, cl = u8(rng, 7, 9), u8(rng, 10, 14)
    at = 2 ** 32 // 3 + 1                                         # pixel offset: byte 2^32 + 2
    assert at * 3 > 2 ** 32
    hazy_pool = torch.empty(at * 3 + hz.size, dtype=torch.uint8, device="cuda")
    gt_pool = torch.empty(at * 3 + cl.size, dtype=torch.uint8, device="cuda")
    hazy_pool[at * 3:].copy_(torch.from_numpy(hz).view(-1))
    gt_pool[at * 3:].copy_(torch.from_numpy(cl).view(-1))
    table = [(1, 2, 5), (0, 0, 2), (2, 4, 7), (1, 1, 0)]          # (r, c, k) of 5 x 5 crops; the clear origin is (2, 2)
    rows = [(at + r * 9 + c, 9, at + (2 + r) * 14 + 2 + c, 14, k) for r, c, k in table]
    clean, noisy = call_ragged(gt_pool, hazy_pool, rows, 5, 5, (MEAN, STD))
    for j, (r, c, k) in enumerate(table):
        assert np.array_equal(clean[j], restate(cl[2:9, 2:11], r, c, k, 5, 5)), j
        assert np.array_equal(noisy[j], restate(hz, r, c, k, 5, 5, (MEAN, STD))), j
    del hazy_pool, gt_pool
    torch.cuda.empty_cache()


def write_png(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8), "RGB").save(path)


@pytest.fixture(scope="module")
def reside_folder(tmp_path_factory):
    """five hazy frames of 40 x 56 and 48 x 48 under RESIDE names for three clear frames of 44 x 58 / 48 x 48; validation pairs, one to one"""
    d = str(tmp_path_factory.mktemp("reside"))
    for name, (h, w) in (("1", (44, 58)), ("2", (44, 58)), ("3", (48, 48))):
        write_png(f"{d}/train/gt/{name}.png", h, w, int(name))
    for k, (name, (h, w)) in enumerate((("1_1", (40, 56)), ("1_2_0.85", (40, 56)), ("2_1", (40, 56)), ("3_1", (48, 48)), ("3_2", (48, 48)))):
        write_png(f"{d}/train/hazy/{name}.png", h, w, 10 + k)
    for k, (h, w) in enumerate(((40, 56), (48, 48))):
        write_png(f"{d}/val/gt/{k}.png", h, w, 20 + k)
        write_png(f"{d}/val/hazy/{k}.png", h, w, 30 + k)
    return d


def run_main(folder, out, extra=()):
    import FFA_main
    from dehaze_hip import ops
    os.makedirs(out)
    benchmark = torch.backends.cudnn.benchmark          # main() sets process-wide switches: put them back for the tests that follow
    try:
        FFA_main.main(["--pairing", "reside", "--normalize", "--blocks", "1", "--steps", "2", "--bs", "2", "--crop_size", "32", "--eval_step", "2",
                       "--log_every", "1", "--model_dir", out + "/", "--train_dir", folder + "/train", "--val_dir", folder + "/val",
                       "--deterministic", *extra])
    finally:
        ops.set_deterministic(False)
        torch.backends.cudnn.benchmark = benchmark
    pk = glob.glob(out + "/*_2_psnr*.pk")
    assert len(pk) == 1
    state = torch.load(pk[0], map_location="cpu")
    assert set(state) == {"step", "max_psnr", "max_ssim", "ssims", "psnrs", "losses", "model"}          # --normalize adds no key
    losses = np.load(glob.glob(out + "/*_2_losses.npy")[0])
    assert losses.shape == (2,) and np.isfinite(losses).all() and state["losses"] == losses.tolist()
    return losses


def test_ffa_main_trains_from_a_reside_folder_of_mixed_sizes(reside_folder, tmp_path, monkeypatch):
    import dataset
    seen = []
    real = dataset.ImageStoreHBM.batch
    monkeypatch.setattr(dataset.ImageStoreHBM, "batch", lambda self, ids, ps, normalize=None: seen.append((list(ids), ps, normalize))
                        or real(self, ids, ps, normalize=normalize))
    a = run_main(reside_folder, str(tmp_path / "a"))
    assert len(seen) == 2 and all(ps == 32 and norm == (MEAN, STD) and len(ids) == 2 for ids, ps, norm in seen)
    b = run_main(reside_folder, str(tmp_path / "b"))
    assert np.array_equal(a, b)          # --deterministic: the same losses from run to run


def test_ffa_main_whole_images_of_mixed_sizes(reside_folder, tmp_path, monkeypatch):
    import dataset
    drawn = []
    real = dataset.ImageStoreHBM.draw_whole_batch
    monkeypatch.setattr(dataset.ImageStoreHBM, "draw_whole_batch", lambda self, bs: drawn.append(real(self, bs)) or drawn[-1])
    run_main(reside_folder, str(tmp_path / "w"), ("--whole_img",))
    assert len(drawn) == 2 and all(len(ids) == 2 for ids in drawn)
    sizes = [{(40, 56) if int(i) < 3 else (48, 48) for i in ids} for ids in drawn]          # sorted hazy names: three 40 x 56, two 48 x 48
    assert all(len(s) == 1 for s in sizes)
