"""The training feed for h x w crops and whole images (dhz_crop_augment_pair_rect through PatchStoreHBM.batch(indices, (h, w) | None)) against
a numpy restatement, bit for bit: value / 255 in fp32 is one IEEE division on either side.  A square request through the rect entry equals
the square entry (PatchStoreHBM.batch(indices, int)) bit for bit."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 10, 14


def make_store():
    import dataset
    g = torch.Generator().manual_seed(21)
    gt = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8)
    hazy = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8)
    return dataset.PatchStoreHBM(gt, hazy, "cuda"), gt.numpy(), hazy.numpy()


def restate(img, r, c, k, h, w):
    """uint8 HWC image -> float32 CHW h x w crop under map k, in numpy: 0 id, 2 rot180, 4 flip rows, 6 flip columns; the odd maps (square
    crops only) as utils/dataset_utils.py composes them: rot90(k, dims=[-1, -2]) then, from 4 up, flip(-2)"""
    crop = np.transpose(img[r:r + h, c:c + w].astype(np.float32) / np.float32(255.0), (2, 0, 1))
    out = np.rot90(crop, k % 4, axes=(2, 1))
    if k >= 4:
        out = out[:, ::-1, :]
    return np.ascontiguousarray(out)


def call_rect(store, table, h, w):
    """one raw launch with a given table (every admitted k, chosen origins)"""
    from dehaze_hip import _lib
    tab = torch.tensor(table, dtype=torch.int32).cuda()
    n = len(table)
    clean = torch.full((n * 3 * h * w + 64,), float("nan"), device="cuda")
    noisy = torch.full((n * 3 * h * w + 64,), float("nan"), device="cuda")
    _lib.call("dhz_crop_augment_pair_rect", store.gt.data_ptr(), store.hazy.data_ptr(), tab.data_ptr(), clean.data_ptr(), noisy.data_ptr(),
              n, H, W, h, w, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    m = n * 3 * h * w
    assert torch.isnan(clean[m:]).all() and torch.isnan(noisy[m:]).all(), "written past the end"
    return clean[:m].cpu().view(n, 3, h, w).numpy(), noisy[:m].cpu().view(n, 3, h, w).numpy()


@pytest.mark.parametrize("h,w", [(10, 14), (6, 9)])
def test_every_admitted_map_of_a_non_square_crop(h, w):
    """k = 0 .. 7 in the table: the kernel reads k & 6"""
    store, gt, hazy = make_store()
    table = [(k % 3, min(k % 5, H - h), min((3 * k) % 6, W - w), k) for k in range(8)]
    clean, noisy = call_rect(store, table, h, w)
    for j, (i, r, c, k) in enumerate(table):
        assert np.array_equal(clean[j], restate(gt[i], r, c, k & 6, h, w)), (j, k)
        assert np.array_equal(noisy[j], restate(hazy[i], r, c, k & 6, h, w)), (j, k)
    assert not np.array_equal(clean[0], clean[2])          # (the maps differ)


def test_every_map_of_a_square_crop_through_the_rect_entry():
    store, gt, hazy = make_store()
    table = [(k % 3, k % 4, (2 * k) % 8, k) for k in range(8)]
    clean, noisy = call_rect(store, table, 6, 6)
    for j, (i, r, c, k) in enumerate(table):
        assert np.array_equal(clean[j], restate(gt[i], r, c, k, 6, 6)), (j, k)
        assert np.array_equal(noisy[j], restate(hazy[i], r, c, k, 6, 6)), (j, k)


@pytest.mark.parametrize("size", [(10, 14), (6, 9), None])
def test_batch_against_the_numpy_restatement(size):
    import dataset
    store, gt, hazy = make_store()
    h, w = size if size is not None else (H, W)
    idx = [2, 0, 1, 1, 2, 0, 0, 1, 2, 2, 1, 0]
    np.random.seed(5); random.seed(5)
    clean, noisy = store.batch(idx, size)
    np.random.seed(5); random.seed(5)
    draws = [dataset.draw_rect_aug(H, W, h, w) for _ in idx]
    assert clean.shape == noisy.shape == (len(idx), 3, h, w) and clean.dtype == torch.float32 and clean.is_cuda
    assert {k for _, _, k in draws} <= {0, 2, 4, 6} and len({k for _, _, k in draws}) > 1
    for j, (i, (r, c, k)) in enumerate(zip(idx, draws)):
        assert np.array_equal(clean[j].cpu().numpy(), restate(gt[i], r, c, k, h, w)), j
        assert np.array_equal(noisy[j].cpu().numpy(), restate(hazy[i], r, c, k, h, w)), j
    if size is None or size == (H, W):
        assert all(r == 0 and c == 0 for r, c, _ in draws)


def test_square_request_through_the_rect_entry_equals_the_square_entry():
    store, _, _ = make_store()
    idx = [0, 1, 2, 2, 1, 0, 1, 1, 0, 2, 0, 1, 2, 0, 2, 1]
    np.random.seed(9); random.seed(9)
    c0, n0 = store.batch(idx, 6)
    tab0 = store._table.clone()
    np.random.seed(9); random.seed(9)
    c1, n1 = store.batch(idx, (6, 6))
    assert torch.equal(store._table, tab0) and len(set(tab0[:, 3].tolist())) > 4          # the same draws, odd maps among them
    assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)) and torch.equal(n0.view(torch.int32), n1.view(torch.int32))


@pytest.mark.parametrize("ps", [17, 16, 3])
def test_the_square_entry_itself_on_full_and_partial_blocks(ps):
    """dhz_crop_augment_pair called directly on a 20 x 23 store of 3 images, one block of 256 pixels per item at a time: ps = 17 is 289
    pixels, two blocks with a tail of 33; 16 exactly one full block; 3 one partial block.  n = 9: every k of 0 .. 7 and several (r, c).
    Bit for bit the numpy restatement, and bit for bit dhz_crop_augment_pair_rect on the same table."""
    import dataset
    from dehaze_hip import _lib
    Hs, Ws, n = 20, 23, 9
    g = torch.Generator().manual_seed(33)
    gt = torch.randint(0, 256, (3, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    hazy = torch.randint(0, 256, (3, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    store = dataset.PatchStoreHBM(gt, hazy, "cuda")
    table = [(t % 3, (2 * t) % (Hs - ps + 1), (5 * t) % (Ws - ps + 1), t % 8) for t in range(n)]
    assert {k for *_, k in table} == set(range(8)) and len({(r, c) for _, r, c, _ in table}) >= 2
    tab = torch.tensor(table, dtype=torch.int32).cuda()
    m = n * 3 * ps * ps
    outs = {}
    for entry, sizes in (("dhz_crop_augment_pair", (ps,)), ("dhz_crop_augment_pair_rect", (ps, ps))):
        clean = torch.full((m + 64,), float("nan"), device="cuda")
        noisy = torch.full((m + 64,), float("nan"), device="cuda")
        _lib.call(entry, store.gt.data_ptr(), store.hazy.data_ptr(), tab.data_ptr(), clean.data_ptr(), noisy.data_ptr(), n, Hs, Ws, *sizes,
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.isnan(clean[m:]).all() and torch.isnan(noisy[m:]).all(), "written past the end"
        outs[entry] = (clean[:m].cpu().view(n, 3, ps, ps), noisy[:m].cpu().view(n, 3, ps, ps))
    clean, noisy = outs["dhz_crop_augment_pair"]
    for j, (i, r, c, k) in enumerate(table):
        assert np.array_equal(clean[j].numpy(), restate(gt[i].numpy(), r, c, k, ps, ps)), (j, k)
        assert np.array_equal(noisy[j].numpy(), restate(hazy[i].numpy(), r, c, k, ps, ps)), (j, k)
    rect_clean, rect_noisy = outs["dhz_crop_augment_pair_rect"]
    assert torch.equal(clean.view(torch.int32), rect_clean.view(torch.int32)) and torch.equal(noisy.view(torch.int32), rect_noisy.view(torch.int32))


def test_a_crop_larger_than_the_store_is_refused():
    from dehaze_hip import _lib
    store, _, _ = make_store()
    for size in ((11, 14), (10, 15), (12, 12)):
        with pytest.raises(ValueError, match="does not fit"):
            store.batch([0, 1], size)
    tab = torch.zeros((2, 4), dtype=torch.int32).cuda()
    out = torch.empty(2 * 3 * 11 * 14, device="cuda")
    with pytest.raises(_lib.DehazeHipError, match="bad sizes"):
        _lib.call("dhz_crop_augment_pair_rect", store.gt.data_ptr(), store.hazy.data_ptr(), tab.data_ptr(), out.data_ptr(), out.data_ptr(),
                  2, H, W, 11, 14, torch.cuda.current_stream().cuda_stream)
