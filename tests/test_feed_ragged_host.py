"""CPU-side checks of the store for image folders of mixed sizes (dataset.ImageStoreHBM, csrc/data_feed.hip: dhz_crop_augment_pair_ragged): the
two pairing rules on folders written with PIL, the centre-crop rule, the eligible lists, the size buckets of whole-image batches, the entry's
argument checks without a device, and that a folder today's store can serve stays on it."""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write(path, h, w, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    Image.fromarray(img, "RGB").save(path)
    return img


def image(store, pool, off, hw):
    return pool[off * 3:(off + hw[0] * hw[1]) * 3].view(hw[0], hw[1], 3).numpy()


def test_center_crop_rule_is_torchvisions():
    """int(round(d / 2.0)), Python's round: half to even"""
    import dataset
    assert [dataset.center_crop_origin(10 + d, 20, 10, 20)[0] for d in range(9)] == [0, 0, 1, 2, 2, 2, 3, 4, 4]
    assert [dataset.center_crop_origin(10, 20 + d, 10, 20)[1] for d in range(9)] == [0, 0, 1, 2, 2, 2, 3, 4, 4]
    assert dataset.center_crop_origin(480, 640, 460, 620) == (10, 10)          # ITS


def test_reside_pairing_shares_clear_frames(tmp_path):
    import dataset
    d = str(tmp_path)
    clear7 = write(f"{d}/gt/7.png", 12, 16, 1)
    clear9 = write(f"{d}/gt/9.png", 9, 11, 2)
    write(f"{d}/gt/unused.png", 5, 5, 3)
    h71 = write(f"{d}/hazy/7_1.png", 10, 14, 4)
    h72 = write(f"{d}/hazy/7_2_0.85.png", 10, 14, 5)
    h9 = write(f"{d}/hazy/9_10_0.2.png", 9, 8, 6)
    open(f"{d}/hazy/notes.txt", "w").write("not an image")
    store = dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="reside")
    assert len(store) == 3 and [os.path.basename(f) for f in store.hazy_files] == ["7_1.png", "7_2_0.85.png", "9_10_0.2.png"]
    assert [os.path.basename(f) for f in store.clear_files] == ["7.png", "9.png"] and store.clear_of == [0, 0, 1]
    assert store.gt_pool.numel() == (12 * 16 + 9 * 11) * 3 and store.hazy_pool.numel() == (2 * 10 * 14 + 9 * 8) * 3
    assert store.hazy_hw == [(10, 14), (10, 14), (9, 8)] and store.origin == [(1, 1), (1, 1), (0, 2)] and store.uniform is None
    for i, ref in enumerate((h71, h72, h9)):
        assert np.array_equal(image(store, store.hazy_pool, store.hazy_off[i], store.hazy_hw[i]), ref)
    for j, ref in enumerate((clear7, clear9)):
        assert np.array_equal(image(store, store.gt_pool, store.clear_off[j], store.clear_hw[j]), ref)


def test_reside_pairing_other_clear_format_and_jpeg_hazy(tmp_path):
    import dataset
    d = str(tmp_path)
    write(f"{d}/gt/0001.jpg", 8, 8, 1)
    write(f"{d}/hazy/0001_0.8_0.2.jpg", 8, 8, 2)
    write(f"{d}/hazy/0001_1.JPEG", 8, 8, 3)
    store = dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="reside", clear_format=".jpg")
    assert len(store) == 2 and store.clear_of == [0, 0] and store.uniform == (8, 8)
    with pytest.raises(FileNotFoundError, match="0001"):
        dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="reside")          # .png clear frames: there are none


def test_a_missing_clear_frame_names_the_file(tmp_path):
    import dataset
    d = str(tmp_path)
    write(f"{d}/gt/7.png", 12, 16, 1)
    write(f"{d}/hazy/7_1.png", 10, 14, 2)
    write(f"{d}/hazy/8_1.png", 10, 14, 3)
    with pytest.raises(FileNotFoundError, match=r"8_1\.png.*8\.png"):
        dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="reside")


@pytest.mark.parametrize("hw", [(9, 16), (12, 13)])
def test_a_clear_frame_smaller_than_its_hazy_frame_is_refused(tmp_path, hw):
    import dataset
    d = str(tmp_path)
    write(f"{d}/gt/7.png", hw[0], hw[1], 1)
    write(f"{d}/hazy/7_1.png", 10, 14, 2)
    with pytest.raises(ValueError, match=r"7_1\.png.*smaller"):
        dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="reside")
    with pytest.raises(ValueError, match="smaller"):
        dataset.ImageStoreHBM([(torch.zeros(hw + (3,), dtype=torch.uint8), torch.zeros((10, 14, 3), dtype=torch.uint8))], "cpu")


def test_ranks_load_only_the_clear_frames_of_their_share(tmp_path):
    import dataset
    d = str(tmp_path)
    for c in range(4):
        write(f"{d}/gt/{c}.png", 8 + c, 9, c)
        for v in range(2):
            write(f"{d}/hazy/{c}_{v}.png", 8 + c, 9, 10 + 2 * c + v)
    names = [f"{c}_{v}.png" for c in range(4) for v in range(2)]
    seen = []
    for rank in range(4):
        store = dataset.ImageStoreHBM.from_dir(d, "cpu", rank=rank, world=4, pairing="reside")
        assert [os.path.basename(f) for f in store.hazy_files] == names[rank::4]
        assert [os.path.basename(f) for f in store.clear_files] == [f"{rank // 2}.png", f"{rank // 2 + 2}.png"]          # 2 of the 4
        assert store.gt_pool.numel() == sum((8 + c) * 9 * 3 for c in (rank // 2, rank // 2 + 2))
        seen += store.hazy_files
    assert sorted(os.path.basename(f) for f in seen) == names


def test_sorted_pairing_takes_any_sizes_and_refuses_unequal_counts(tmp_path):
    import dataset
    d = str(tmp_path)
    write(f"{d}/gt/a.png", 8, 9, 1), write(f"{d}/hazy/x.png", 8, 9, 2)
    write(f"{d}/gt/b.png", 13, 11, 3), write(f"{d}/hazy/y.png", 10, 10, 4)
    store = dataset.ImageStoreHBM.from_dir(d, "cpu")
    assert store.hazy_hw == [(8, 9), (10, 10)] and store.clear_of == [0, 1] and store.origin == [(0, 0), (2, 0)]
    assert [len(dataset.ImageStoreHBM.from_dir(d, "cpu", rank=r, world=2)) for r in (0, 1)] == [1, 1]
    write(f"{d}/hazy/z.png", 10, 10, 5)
    with pytest.raises(ValueError, match="reside"):
        dataset.ImageStoreHBM.from_dir(d, "cpu")
    with pytest.raises(ValueError, match="pairing"):
        dataset.ImageStoreHBM.from_dir(d, "cpu", pairing="names")


def mixed_store(counts=((6, 8, 3), (7, 5, 5), (9, 9, 2))):
    import dataset
    pairs = []
    for h, w, n in counts:
        for _ in range(n):
            pairs.append((torch.zeros((h, w, 3), dtype=torch.uint8), torch.zeros((h, w, 3), dtype=torch.uint8)))
    order = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(0)).tolist()          # buckets interleaved
    return dataset.ImageStoreHBM([pairs[i] for i in order], "cpu")


def test_eligible_lists_and_their_cache():
    store = mixed_store()
    for h, w in ((6, 5), (7, 5), (6, 8), (9, 9), (1, 9)):
        want = [i for i, (H, W) in enumerate(store.hazy_hw) if H >= h and W >= w]
        got = store.eligible(h, w)
        assert got.dtype == torch.long and got.tolist() == want
        assert store.eligible(h, w) is got          # cached per size
    assert len(store.eligible(6, 5)) == len(store) and len(store.eligible(9, 9)) == 2
    for h, w in ((10, 1), (1, 10), (8, 8 + 2)):
        with pytest.raises(ValueError, match="no stored image"):
            store.eligible(h, w)


def test_a_shared_clear_tensor_is_stored_once():
    import dataset
    clear = torch.full((10, 14, 3), 7, dtype=torch.uint8)
    other = torch.full((10, 14, 3), 9, dtype=torch.uint8)
    hz = [torch.full((10, 14, 3), v, dtype=torch.uint8) for v in (1, 2, 3)]
    store = dataset.ImageStoreHBM([(clear, hz[0]), (other, hz[1]), (clear, hz[2])], "cpu")
    assert store.clear_of == [0, 1, 0] and store.gt_pool.numel() == 2 * 10 * 14 * 3 and store.uniform == (10, 14)


def test_whole_batches_have_one_size_and_buckets_come_up_by_their_counts():
    """2 000 seeded draws: each bucket's share of the batches lies within 4 binomial standard deviations of count / N"""
    counts = ((6, 8, 3), (7, 5, 5), (9, 9, 2))
    store = mixed_store(counts)
    N, draws = len(store), 2000
    torch.manual_seed(11)
    hits = {}
    for _ in range(draws):
        ids = store.draw_whole_batch(3)
        assert ids.dtype == torch.long and ids.shape == (3,)
        sizes = {store.hazy_hw[i] for i in ids.tolist()}
        assert len(sizes) == 1
        hits[next(iter(sizes))] = hits.get(next(iter(sizes)), 0) + 1
    for h, w, n in counts:
        p = n / N
        sd = math.sqrt(p * (1 - p) / draws)
        share = hits[(h, w)] / draws
        print(f"bucket {h} x {w}: share {share:.4f}, expected {p:.4f}, {abs(share - p) / sd:.2f} sd")
        assert abs(share - p) <= 4 * sd, (h, w, share, p, sd)
    # every item of a bucket comes up
    torch.manual_seed(12)
    assert {int(i) for _ in range(200) for i in store.draw_whole_batch(4)} == set(range(N))


def test_batch_refuses_before_any_draw():
    """mixed whole images and a crop that an item does not hold: ValueError, no generator touched, no device needed"""
    import random
    store = mixed_store()
    small = store.hazy_hw.index((6, 8))
    big = store.hazy_hw.index((9, 9))
    np.random.seed(3), random.seed(3)
    before = (np.random.get_state()[1].copy(), random.getstate())
    with pytest.raises(ValueError, match="different sizes"):
        store.batch([small, big], None)
    for ps in (7, (7, 5), (6, 9)):
        with pytest.raises(ValueError, match="does not fit"):
            store.batch([big, small], ps)
    assert np.array_equal(np.random.get_state()[1], before[0]) and random.getstate() == before[1]


def test_the_entry_is_declared_bound_and_checks_its_arguments_without_a_gpu():
    from dehaze_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    assert "dhz_crop_augment_pair_ragged(" in hdr and "data_utils.py:51-81" in hdr and "DHZ_RAGGED_DESC_WORDS 5" in hdr
    assert len(_lib.SIGNATURES["dhz_crop_augment_pair_ragged"]) == 10
    f = lib.dhz_crop_augment_pair_ragged
    for hole in range(5):          # gt pool, hazy pool, descriptor, both outputs
        ptrs = [8] * 5
        ptrs[hole] = None
        assert f(*ptrs, None, 2, 4, 4, None) == -22 and b"dhz_crop_augment_pair_ragged: null pointer" in lib.dhz_last_error()
    for n, h, w in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (-1, 4, 4), (2, -4, 4), (2, 4, -4)):
        assert f(8, 8, 8, 8, 8, None, n, h, w, None) == -22 and b"dhz_crop_augment_pair_ragged: bad sizes" in lib.dhz_last_error()
    assert f(8, 8, 8, 8, 8, None, 1 << 11, 1 << 10, 1 << 10, None) == -22 and b"batch too large" in lib.dhz_last_error()
    assert f(8, 8, 8, 8, 8, None, 1 << 15, 1 << 15, 2, None) == -22 and b"batch too large" in lib.dhz_last_error()


def test_ffa_main_defaults_and_new_switches():
    import FFA_main
    opt = FFA_main.parse([])
    assert opt.pairing == "sorted" and opt.clear_format == ".png" and opt.normalize is False
    opt = FFA_main.parse(["--pairing", "reside", "--clear_format", ".jpg", "--normalize"])
    assert opt.pairing == "reside" and opt.clear_format == ".jpg" and opt.normalize is True
    with pytest.raises(SystemExit):
        FFA_main.parse(["--pairing", "names"])
    doc = FFA_main.__doc__
    assert "loaders are not restated" not in doc and "FFA_test.py --normalize" in doc and "data_utils.py:54-56" in doc


def test_the_store_choice_keeps_todays_folders_on_the_old_store(tmp_path, monkeypatch):
    """a spy on both from_dir: a uniform, equally counted folder under default options is built by PatchStoreHBM.from_dir with today's
    arguments; mixed sizes, unequal counts, RESIDE pairing and normalisation go to ImageStoreHBM.from_dir"""
    import dataset
    calls = []
    monkeypatch.setattr(dataset.PatchStoreHBM, "from_dir", classmethod(lambda cls, *a, **k: calls.append(("patch", a, k)) or "P"))
    monkeypatch.setattr(dataset.ImageStoreHBM, "from_dir", classmethod(lambda cls, *a, **k: calls.append(("image", a, k)) or "I"))
    d = str(tmp_path / "u")
    for i in range(3):
        write(f"{d}/gt/{i}.png", 8, 9, i), write(f"{d}/hazy/{i}_1.png", 8, 9, 10 + i)
    assert dataset.train_store(d, "cpu") == "P" and calls[-1] == ("patch", (d, "cpu", 0, 1), {})
    assert dataset.train_store(d, "cpu", 1, 2) == "P" and calls[-1] == ("patch", (d, "cpu", 1, 2), {})
    assert dataset.train_store(d, "cpu", normalize=True) == "I"
    assert calls[-1] == ("image", (d, "cpu", 0, 1), {"pairing": "sorted", "clear_format": ".png"})
    assert dataset.train_store(d, "cpu", pairing="reside", clear_format=".jpg") == "I"
    assert calls[-1] == ("image", (d, "cpu", 0, 1), {"pairing": "reside", "clear_format": ".jpg"})
    write(f"{d}/hazy/2_2.png", 8, 9, 20)                     # counts differ
    assert dataset.train_store(d, "cpu") == "I"
    os.remove(f"{d}/hazy/2_2.png")
    assert dataset.train_store(d, "cpu") == "P"
    write(f"{d}/gt/2.png", 9, 9, 21)                         # one clear frame of another size
    assert dataset.train_store(d, "cpu", 1, 2) == "I" and calls[-1][1] == (d, "cpu", 1, 2)
