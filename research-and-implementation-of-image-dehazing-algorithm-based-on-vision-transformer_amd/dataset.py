"""Drop-in for Uformer_ProbSparse/dataset.py (PNG pair datasets over <dir>/gt and <dir>/hazy) plus the MI355X-native
feed for training: `PatchStoreHBM`.

The reference's DataLoaderTrain (dataset.py:17-77) decodes two PNGs per item on the host, crops a random ps x ps
window, applies one of 8 rotate/flip augmentations and ships float32 through DataLoader workers and PCIe every step.
`PatchStoreHBM` decodes every patch pair ONCE into two uint8 [N,H,W,3] tensors resident in HBM (NH-HAZE train
patches: 2 x 5.4 GB of 288 GB) and produces a batch with one kernel launch (dhz_crop_augment_pair: gather + crop +
rotate/flip + /255 to float32 CHW), drawing (r, c, augmentation) per item from the same host generators in the same
order as DataLoaderTrain.__getitem__, so a batch equals what the reference dataset returns for those items and draws.
With `mixup=` the same launch also forms My_train.py's MixUp of the batch (the `_mix` entries; `gather_pair` for resident tensors).
"""
import collections
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from utils import is_png_file, load_img, load_img_u8, Augment_RGB_torch

augment = Augment_RGB_torch()
transforms_aug = [method for method in dir(augment) if callable(getattr(augment, method)) if not method.startswith('_')]


def _pair_files(rgb_dir, gt_dir='gt', input_dir='hazy'):
    clean_files = sorted(os.listdir(os.path.join(rgb_dir, gt_dir)))
    noisy_files = sorted(os.listdir(os.path.join(rgb_dir, input_dir)))
    clean = [os.path.join(rgb_dir, gt_dir, x) for x in clean_files if is_png_file(x)]
    noisy = [os.path.join(rgb_dir, input_dir, x) for x in noisy_files if is_png_file(x)]
    return clean, noisy


def draw_crop_aug(H, W, ps):
    """(r, c, augmentation index) exactly as dataset.py:56-70 draws them (numpy global RNG, then `random`)."""
    if H - ps == 0:
        r, c = 0, 0
    else:
        r = np.random.randint(0, H - ps)
        c = np.random.randint(0, W - ps)
    return r, c, random.getrandbits(3)


def draw_rect_aug(H, W, h, w):
    """(r, c, k) for an h x w crop of an H x W image.  h == w: draw_crop_aug itself.  h != w: the same number of draws - none for the
    whole image, else one per axis, an axis without room drawing from [0, 1) - and the augmentation masked to the four maps that keep
    the shape (k & 6: 0 identity, 2 rot180, 4 flip(-2), 6 flip(-1))."""
    if h == w:
        return draw_crop_aug(H, W, h)
    if H == h and W == w:
        r, c = 0, 0
    else:
        r = np.random.randint(0, max(H - h, 1))
        c = np.random.randint(0, max(W - w, 1))
    return r, c, random.getrandbits(3) & 6


def _chw(path):
    """One PNG as float32 CHW in [0, 1] (the reference's load_img + permute)."""
    return torch.from_numpy(np.float32(load_img(path))).permute(2, 0, 1)


class _PngFolder(Dataset):
    """Host-side datasets of the reference's evaluation scripts: item -> decoded tensors + file names.  `pairs` = gt / hazy
    sub-directories (training, validation), otherwise a HAZY directory only (test).  Attribute names are the reference's."""

    def __init__(self, rgb_dir, pairs=True, target_transform=None):
        super().__init__()
        self.target_transform = target_transform
        if pairs:
            self.clean_filenames, self.noisy_filenames = _pair_files(rgb_dir)
        else:
            self.clean_filenames = None
            self.noisy_filenames = [os.path.join(rgb_dir, 'HAZY', f) for f in sorted(os.listdir(os.path.join(rgb_dir, 'HAZY')))
                                    if is_png_file(f)]
        self.tar_size = len(self.noisy_filenames)

    def __len__(self):
        return self.tar_size

    def _pair(self, index):
        i = index % self.tar_size
        cf, nf = self.clean_filenames[i], self.noisy_filenames[i]
        return _chw(cf), _chw(nf), os.path.basename(cf), os.path.basename(nf)


class DataLoaderVal(_PngFolder):                       # dataset.py:82-110: whole image pairs
    def __init__(self, rgb_dir, target_transform=None):
        super().__init__(rgb_dir, True, target_transform)

    def __getitem__(self, index):
        return self._pair(index)


class DataLoaderTrain(_PngFolder):                     # dataset.py:17-77: random ps x ps crop + one of 8 rotations / flips
    def __init__(self, rgb_dir, img_options=None, target_transform=None):
        super().__init__(rgb_dir, True, target_transform)
        self.img_options = img_options

    def __getitem__(self, index):
        clean, noisy, cn, nn_ = self._pair(index)
        ps = self.img_options['patch_size']
        r, c, k = draw_crop_aug(clean.shape[1], clean.shape[2], ps)        # the reference's draw order (numpy, then random)
        aug = getattr(augment, transforms_aug[k])
        return aug(clean[:, r:r + ps, c:c + ps]), aug(noisy[:, r:r + ps, c:c + ps]), cn, nn_


class DataLoaderTest(_PngFolder):                      # dataset.py:115-138: hazy images only
    def __init__(self, rgb_dir, target_transform=None):
        super().__init__(rgb_dir, False, target_transform)

    def __getitem__(self, index):
        f = self.noisy_filenames[index % self.tar_size]
        return _chw(f), os.path.basename(f)


class DataLoaderTestSR(Dataset):                       # dataset.py:205-232: PNGs directly under rgb_dir -> (tensor, file name)
    def __init__(self, rgb_dir, target_transform=None):
        super().__init__()
        self.target_transform = target_transform
        self.LR_filenames = [os.path.join(rgb_dir, f) for f in sorted(os.listdir(rgb_dir)) if is_png_file(f)]
        self.tar_size = len(self.LR_filenames)

    def __len__(self):
        return self.tar_size

    def __getitem__(self, index):
        f = self.LR_filenames[index % self.tar_size]
        return _chw(f), os.path.split(f)[-1]


FEED_MIXUP = os.environ.get("DHZ_FEED_MIXUP", "1") != "0"      # A/B switch: off = My_train.py mixes with MixUp_AUG.aug after the feed
_RECENT_TABLES = collections.deque(maxlen=8)                   # the last pinned tables: each stays alive until its upload ran


def _mix_table(rows, mixup, device, dtype=None):
    """The host table of ONE feed launch - every caller's: rows [n, k] (a list of int tuples, or a host tensor) as `dtype` (default: the
    tensor's own, int32 or int64), in pinned memory when `device` is a GPU, kept alive here until the non-blocking upload ran.  With a
    mixup the table is [n, k + 2], the table of the `_mix` entries: the rows, then MixUp's partner and the bit pattern of its fp32 lam,
    both from mixup.draw(n) - called HERE, after the caller drew every row's geometry.  The kernels index the table with partner
    unchecked, so it is checked here."""
    rows = torch.as_tensor(rows, dtype=dtype)
    pin = torch.device(device).type == "cuda"
    if mixup is None:
        tab = rows.pin_memory() if pin else rows
    else:
        n = rows.shape[0]
        partner, lam = mixup.draw(n)
        assert partner.shape == (n,) and lam.shape == (n,) and lam.dtype == torch.float32
        assert n > 0 and 0 <= int(partner.min()) and int(partner.max()) < n, "MixUp partner outside the batch"
        tab = torch.empty((n, rows.shape[1] + 2), dtype=rows.dtype, pin_memory=pin)
        tab[:, :-2] = rows
        tab[:, -2] = partner
        tab[:, -1] = lam.contiguous().view(torch.int32)            # (a lam is positive: the int32 is the bit pattern in an int64 row too)
    _RECENT_TABLES.append(tab)
    return tab


def gather_pair(tgt_all, inp_all, sel, mixup=None):
    """(tgt_all[sel], inp_all[sel]) of two resident float32 tensors [N, ...] of one shape in ONE launch (dhz_gather_mix_pair); with a
    utils.MixUp_AUG, mixup.aug of that pair bit for bit, out of the same draws.  sel: host LongTensor or a list of item ids; it travels
    in the pinned table - no sel.to(device), no blocking copy."""
    from dehaze_hip import _lib
    from dehaze_hip.ops import _p, _stream
    assert tgt_all.is_cuda and tgt_all.dtype == inp_all.dtype == torch.float32 and tgt_all.shape == inp_all.shape
    assert tgt_all.is_contiguous() and inp_all.is_contiguous() and tgt_all.device == inp_all.device
    sel = torch.as_tensor(sel, dtype=torch.int64).reshape(-1)
    assert not sel.is_cuda, "gather_pair: sel is a host tensor (it goes into the pinned table)"
    n, N = sel.numel(), tgt_all.shape[0]
    assert n > 0 and 0 <= int(sel.min()) and int(sel.max()) < N, "gather_pair: item id outside the resident tensors"
    rows = sel.view(n, 1)
    if mixup is None:
        rows = torch.nn.functional.pad(rows, (0, 2))                # (the entry reads rows of three words with mix == 0 too)
    tab_d = _mix_table(rows, mixup, tgt_all.device).to(tgt_all.device, non_blocking=True)
    target = torch.empty((n,) + tuple(tgt_all.shape[1:]), device=tgt_all.device, dtype=torch.float32)
    input_ = torch.empty_like(target)
    _lib.call("dhz_gather_mix_pair", _p(tgt_all), _p(inp_all), tab_d.data_ptr(), _p(target), _p(input_), n, tgt_all[0].numel(),
              int(mixup is not None), _stream())
    return target, input_


class PatchStoreHBM:
    """All (gt, hazy) patch pairs of a directory as uint8 [N,H,W,3] tensors in HBM + the batch kernel."""

    def __init__(self, gt_u8, hazy_u8, device):
        assert gt_u8.dtype == torch.uint8 and gt_u8.shape == hazy_u8.shape and gt_u8.dim() == 4 and gt_u8.shape[-1] == 3
        self.device = torch.device(device)
        self.gt = gt_u8.contiguous().to(self.device)
        self.hazy = hazy_u8.contiguous().to(self.device)
        self.N, self.H, self.W = gt_u8.shape[0], gt_u8.shape[1], gt_u8.shape[2]
        self._table = None

    @classmethod
    def from_dir(cls, rgb_dir, device, rank=0, world=1):
        clean, noisy = _pair_files(rgb_dir)
        clean, noisy = clean[rank::world], noisy[rank::world]
        assert clean, f"no PNG pairs under {rgb_dir}/gt and {rgb_dir}/hazy"
        first = load_img_u8(clean[0])
        gt = torch.empty((len(clean),) + first.shape, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() \
            else torch.empty((len(clean),) + first.shape, dtype=torch.uint8)
        hz = torch.empty_like(gt)
        for i, (a, b) in enumerate(zip(clean, noisy)):
            ia, ib = load_img_u8(a), load_img_u8(b)
            assert ia.shape == first.shape and ib.shape == first.shape, "patches must share one size (generate_patches_SIDD.py)"
            gt[i] = torch.from_numpy(ia)
            hz[i] = torch.from_numpy(ib)
        return cls(gt, hz, device)

    def __len__(self):
        return self.N

    def batch(self, indices, ps, mixup=None):
        """indices: iterable of patch ids.  Returns (clean, noisy) float32 [n,3,ps,ps] on the device; per item the crop
        origin and the augmentation are drawn like DataLoaderTrain.__getitem__ does, in item order.

        mixup: None, or a utils.MixUp_AUG - the batch is then mixup.aug(*batch(indices, ps)) bit for bit, out of the same draws in the
        same order (every item's geometry first, then mixup.draw(n)), from ONE launch of dhz_crop_augment_mix_pair_rect and one pinned
        upload: no gathers, no temporaries, no blocking copy.

        ps may also be (h, w) - an h x w crop, [n,3,h,w] - or None: the stored size, i.e. whole images (FFA_main.py --whole_img).  These go
        through dhz_crop_augment_pair_rect; an int keeps the square entry.  The table is drawn by draw_rect_aug: for h == w exactly
        draw_crop_aug's draws (the batch then equals batch(indices, h) bit for bit), for h != w the same number of draws with the
        augmentation masked to k & 6 - identity, rot180 and the two flips, the four of the eight maps that keep an h x w shape.  The
        reference (FFA_model/data_utils.py:69-77, FF.rotate) rotates the PIL images by 90 degrees WITHOUT expanding the canvas, so its non-square
        frames come out with black corners and cut-off ends; that artefact is deliberately not restated here."""
        from dehaze_hip import _lib
        from dehaze_hip.ops import _p, _stream
        square = isinstance(ps, int)
        h, w = (ps, ps) if square else (self.H, self.W) if ps is None else (int(ps[0]), int(ps[1]))
        if not (0 < h <= self.H and 0 < w <= self.W):
            raise ValueError(f"PatchStoreHBM.batch: a {h} x {w} crop does not fit the stored {self.H} x {self.W} images")
        idx = [int(i) % self.N for i in indices]
        n = len(idx)
        rows = [(i,) + draw_rect_aug(self.H, self.W, h, w) for i in idx]         # (h == w: draw_crop_aug's draws)
        self._table = _mix_table(rows, mixup, self.device, torch.int32)
        tab_d = self._table.to(self.device, non_blocking=True)
        clean = torch.empty((n, 3, h, w), device=self.device, dtype=torch.float32)
        noisy = torch.empty_like(clean)
        if mixup is not None:                                   # (the rect entry equals the square one on h == w)
            entry, sizes = "dhz_crop_augment_mix_pair_rect", (h, w)
        else:
            entry, sizes = ("dhz_crop_augment_pair", (ps,)) if square else ("dhz_crop_augment_pair_rect", (h, w))
        _lib.call(entry, self.gt.data_ptr(), self.hazy.data_ptr(), tab_d.data_ptr(), _p(clean), _p(noisy), n, self.H, self.W, *sizes, _stream())
        return clean, noisy


RESIDE_MEAN, RESIDE_STD = (0.64, 0.6, 0.58), (0.14, 0.15, 0.152)          # FFA_model/data_utils.py:79, test.py:54
_PIL_EXT = ('.png', '.jpg', '.jpeg')


def center_crop_origin(Hc, Wc, Hh, Wh):
    """(top, left) of torchvision's CenterCrop((Hh, Wh)) on an Hc x Wc image, restated: int(round(d / 2.0)) with Python's round, half to
    even - differences 1, 3, 5, 7 give 0, 2, 2, 4."""
    return int(round((Hc - Hh) / 2.0)), int(round((Wc - Wh) / 2.0))


def _image_hw(path):
    """(H, W) from the file's header, nothing decoded"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


class ImageStoreHBM:
    """Image pairs of ANY sizes in HBM: FFA_model/data_utils.py's RESIDE_Dataset (lines 51-81) as two uint8 pools + one kernel launch per
    batch (dhz_crop_augment_pair_ragged).  Item i is hazy frame i; several hazy frames may share one clear frame, which is stored once
    (RESIDE ITS: 13 990 hazy frames for 1 399 clear ones), and a clear frame larger than its hazy frame is centre-cropped to it
    (data_utils.py:61; ITS: 640 x 480 against 620 x 460) - kept as an origin per item (center_crop_origin), no copy of the clear frame.

    pairs: a sequence of (clear, hazy) uint8 [H,W,3] tensors or arrays.  Pairs that hold the SAME clear object share its storage.

    Not restated: the reference zero-pads a clear frame smaller than its hazy frame (CenterCrop pads) - here that is an error; it redraws
    the index until the image holds the crop (data_utils.py:54-56, randint(0, 20000)) - here callers draw from eligible(h, w); and
    FF.rotate's no-expand 90 degree turns of non-square frames (see PatchStoreHBM.batch)."""

    def __init__(self, pairs, device):
        pairs = list(pairs)
        if not pairs:
            raise ValueError("ImageStoreHBM: no image pairs")
        clear_of, clears, seen = [], [], {}
        for clear, _ in pairs:
            if id(clear) not in seen:
                seen[id(clear)] = len(clears)
                clears.append(clear)
            clear_of.append(seen[id(clear)])
        self._layout([tuple(h.shape[:2]) for _, h in pairs], [tuple(c.shape[:2]) for c in clears], clear_of, device)
        for j, c in enumerate(clears):
            self._put(self.gt_pool, self.clear_off[j], self.clear_hw[j], c)
        for i, (_, h) in enumerate(pairs):
            self._put(self.hazy_pool, self.hazy_off[i], self.hazy_hw[i], h)

    def _layout(self, hazy_hw, clear_hw, clear_of, device, names=None):
        """offsets (in pixels) of every image in its pool, the centre-crop origins, the size buckets; allocates the pools"""
        self.device = torch.device(device)
        self.hazy_hw, self.clear_hw, self.clear_of = list(hazy_hw), list(clear_hw), list(clear_of)
        self.N = len(self.hazy_hw)
        self.hazy_off, self.clear_off, self.origin = [], [], []
        at = 0
        for H, W in self.hazy_hw:
            self.hazy_off.append(at)
            at += H * W
        n_hazy, at = at, 0
        for H, W in self.clear_hw:
            self.clear_off.append(at)
            at += H * W
        for i, ((Hh, Wh), j) in enumerate(zip(self.hazy_hw, self.clear_of)):
            Hc, Wc = self.clear_hw[j]
            if Hc < Hh or Wc < Wh:
                who = f" ({names[i]})" if names else ""
                raise ValueError(f"ImageStoreHBM: item {i}{who}: the clear frame {Hc} x {Wc} is smaller than its hazy frame {Hh} x {Wh} "
                                 "(the reference would zero-pad it; not restated)")
            self.origin.append(center_crop_origin(Hc, Wc, Hh, Wh))
        self.hazy_pool = torch.empty(n_hazy * 3, dtype=torch.uint8, device=self.device)
        self.gt_pool = torch.empty(at * 3, dtype=torch.uint8, device=self.device)
        self._buckets = {}
        for i, hw in enumerate(self.hazy_hw):
            self._buckets.setdefault(hw, []).append(i)
        self._buckets = {hw: torch.tensor(ids, dtype=torch.long) for hw, ids in self._buckets.items()}
        self.uniform = self.hazy_hw[0] if len(self._buckets) == 1 else None          # (H, W) when every hazy frame has it
        self._eligible = {}
        self._table = self._draws = None

    @staticmethod
    def _put(pool, off, hw, img):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.array(img))               # (a copy: PIL's arrays are read-only)
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[-1] == 3 and tuple(img.shape[:2]) == tuple(hw)
        pool[off * 3:(off + hw[0] * hw[1]) * 3].copy_(img.contiguous().view(-1))

    @classmethod
    def from_dir(cls, rgb_dir, device, rank=0, world=1, pairing="sorted", clear_format=".png"):
        """pairing "sorted": sorted <dir>/gt PNGs against sorted <dir>/hazy PNGs one to one (PatchStoreHBM's rule), sizes free.
        pairing "reside": every <dir>/hazy file PIL opens (.png, .jpg, .jpeg) belongs to <dir>/gt/<stem up to the first "_"> +
        clear_format (`1400_1.png`, `1400_1_0.85.png` -> `1400.png`).  Ranks take hazy[rank::world] and load only the clear frames their
        share names.  Sizes are read from the headers first, then every file is decoded once, straight into its place in the pool."""
        if pairing == "sorted":
            clean, noisy = _pair_files(rgb_dir)
            if len(clean) != len(noisy):
                raise ValueError(f"ImageStoreHBM.from_dir: {len(clean)} gt against {len(noisy)} hazy PNGs under {rgb_dir} cannot pair one to "
                                 "one (pairing='sorted'); RESIDE's layout is pairing='reside'")
            clean, noisy = clean[rank::world], noisy[rank::world]
            clear_files, clear_of = clean, list(range(len(clean)))
        elif pairing == "reside":
            noisy = [os.path.join(rgb_dir, 'hazy', f) for f in sorted(os.listdir(os.path.join(rgb_dir, 'hazy')))
                     if f.lower().endswith(_PIL_EXT)][rank::world]
            clear_files, clear_of, seen = [], [], {}
            for f in noisy:
                want = os.path.join(rgb_dir, 'gt', os.path.splitext(os.path.basename(f))[0].split('_')[0] + clear_format)
                if want not in seen:
                    if not os.path.exists(want):
                        raise FileNotFoundError(f"ImageStoreHBM.from_dir: hazy frame {f} has no clear frame {want}")
                    seen[want] = len(clear_files)
                    clear_files.append(want)
                clear_of.append(seen[want])
        else:
            raise ValueError(f"ImageStoreHBM.from_dir: pairing={pairing!r}")
        if not noisy:
            raise ValueError(f"no image pairs under {rgb_dir}/gt and {rgb_dir}/hazy")
        self = cls.__new__(cls)
        self._layout([_image_hw(f) for f in noisy], [_image_hw(f) for f in clear_files], clear_of, device, names=noisy)
        self.hazy_files, self.clear_files = noisy, clear_files
        for j, f in enumerate(clear_files):
            self._put(self.gt_pool, self.clear_off[j], self.clear_hw[j], load_img_u8(f))
        for i, f in enumerate(noisy):
            self._put(self.hazy_pool, self.hazy_off[i], self.hazy_hw[i], load_img_u8(f))
        return self

    def __len__(self):
        return self.N

    def eligible(self, h, w):
        """LongTensor of the item ids whose hazy frame holds an h x w crop (cached per size): what a caller draws from instead of the
        reference's redraw loop"""
        key = (int(h), int(w))
        if key not in self._eligible:
            ids = [i for i, (H, W) in enumerate(self.hazy_hw) if H >= key[0] and W >= key[1]]
            if not ids:
                raise ValueError(f"ImageStoreHBM.eligible: no stored image holds a {key[0]} x {key[1]} crop")
            self._eligible[key] = torch.tensor(ids, dtype=torch.long)
        return self._eligible[key]

    def draw_whole_batch(self, bs):
        """item ids of ONE size for a batch of whole images: torch.randint(N) picks an anchor, whose size names the bucket - so buckets
        come up in proportion to their counts -, then torch.randint(len(bucket), (bs,)) picks the items"""
        anchor = int(torch.randint(self.N, (1,)))
        bucket = self._buckets[self.hazy_hw[anchor]]
        return bucket[torch.randint(len(bucket), (bs,))]

    def batch(self, indices, ps, normalize=None, mixup=None):
        """(clean, noisy) float32 [n,3,h,w] on the device.  ps: an int, (h, w), or None - whole images, which then must share one size.  Per
        item, in item order, (r, c, k) = draw_rect_aug(H_i, W_i, h, w) with the item's own size (an int ps: draw_crop_aug), so on a store
        whose images share one size the draws and the output are PatchStoreHBM.batch's bit for bit.  normalize: None, or (mean, std) of
        three floats each - the hazy output becomes (v / 255 - mean) / std in fp32 (ToTensor + Normalize, data_utils.py:78-79); the clear
        output never is.  mixup: None, or a utils.MixUp_AUG - the batch is then mixup.aug(*batch(indices, ps, normalize)) bit for bit out
        of the same draws (geometry of every item first, then mixup.draw(n)), in the same single launch
        (dhz_crop_augment_mix_pair_ragged; _table gets two more words per row, _draws stays).  One pinned descriptor upload per batch."""
        import ctypes
        from dehaze_hip import _lib
        from dehaze_hip.ops import _p, _stream
        idx = [int(i) % self.N for i in indices]
        n = len(idx)
        if ps is None:
            sizes = {self.hazy_hw[i] for i in idx}
            if len(sizes) != 1:
                raise ValueError(f"ImageStoreHBM.batch: whole images of {len(sizes)} different sizes in one batch (draw_whole_batch)")
            h, w = next(iter(sizes))
        else:
            h, w = (int(ps), int(ps)) if isinstance(ps, int) else (int(ps[0]), int(ps[1]))
        for i in idx:
            H, W = self.hazy_hw[i]
            if not (0 < h <= H and 0 < w <= W):
                raise ValueError(f"ImageStoreHBM.batch: a {h} x {w} crop does not fit the stored {H} x {W} image {i} (eligible)")
        rows, draws = [], []
        for i in idx:
            (H, W), j = self.hazy_hw[i], self.clear_of[i]
            r, c, k = draw_rect_aug(H, W, h, w)
            top, left = self.origin[i]
            Wc = self.clear_hw[j][1]
            rows.append((self.hazy_off[i] + r * W + c, W, self.clear_off[j] + (top + r) * Wc + left + c, Wc, k))
            draws.append((i, r, c, k))
        self._table = _mix_table(rows, mixup, self.device, torch.int64)     # (after every item's geometry: the order of batch + MixUp_AUG.aug)
        self._draws = torch.tensor(draws, dtype=torch.int32)    # (id, r, c, k) per item: PatchStoreHBM's table
        tab_d = self._table.to(self.device, non_blocking=True)
        norm = None
        if normalize is not None:
            mean, std = normalize
            norm = (ctypes.c_float * 6)(*[float(v) for v in tuple(mean) + tuple(std)])
        clean = torch.empty((n, 3, h, w), device=self.device, dtype=torch.float32)
        noisy = torch.empty_like(clean)
        _lib.call("dhz_crop_augment_pair_ragged" if mixup is None else "dhz_crop_augment_mix_pair_ragged", self.gt_pool.data_ptr(),
                  self.hazy_pool.data_ptr(), tab_d.data_ptr(), _p(clean), _p(noisy), norm, n, h, w, _stream())
        return clean, noisy


def train_store(rgb_dir, device, rank=0, world=1, pairing="sorted", clear_format=".png", normalize=False):
    """The store a training script feeds from.  PatchStoreHBM, built exactly as before, wherever it can serve: sorted pairing, as many gt
    as hazy PNGs, one size throughout (read from the headers of the WHOLE folder, so every rank decides alike), no normalisation.
    ImageStoreHBM otherwise."""
    if pairing == "sorted" and not normalize:
        clean, noisy = _pair_files(rgb_dir)
        if len(clean) == len(noisy) and len({_image_hw(f) for f in clean + noisy}) <= 1:
            return PatchStoreHBM.from_dir(rgb_dir, device, rank, world)
    return ImageStoreHBM.from_dir(rgb_dir, device, rank, world, pairing=pairing, clear_format=clear_format)
