"""PSNR / SSIM of image pairs scored on the device in float64 (dhz_ssim_pair, csrc/metrics.hip; include/dehaze_hip.h K14), in the two
forms the repository reports:

  * the FFA form - FFA_model/metrics.py (M): `ssim` = 11 x 11 Gaussian window (sigma 1.5) over zero padding of 5, both images clamped to
    [0, 1], C1 = 0.01^2, C2 = 0.03^2, mean over the whole map (M:31-58); `psnr` = 20 log10(1 / rmse) of the clamped pair, 100 when
    rmse == 0 (M:61-68).  ssim_gauss / psnr_ffa.  The window table is built as M:19-28 builds it, fp32 outer product included.
  * the uniform form - utils/metrics.py (U), the scikit-image form for float images: 7 x 7 uniform window, sample covariance,
    data_range 2, borders cropped, channel mean (U:34-60); PSNR with data_range 1 if gt.min() >= 0 else 2 (U:17-31).
    ssim_uniform / psnr_uniform.

Routing: fp32 device tensors go to the kernel; anything else (CPU tensors, other dtypes) runs the plain torch / numpy formula of M or U.
The kernel's arithmetic is double throughout, so a device score is the float64 evaluation of the formula on the fp32 inputs (M's own
fp32 evaluation is up to 7.7e-5 off that on near-constant images).  `Scores` keeps per-image results on the device and reads them back
once per validation pass.  Opt-in: nothing on the default paths imports this module.
"""
import math
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

FFA_K, UNI_K = 11, 7
_C1, _C2 = 0.01 ** 2, 0.03 ** 2


# ---- the window, M:19-28: exp(-(i - K // 2)^2 / (2 sigma^2)) in Python doubles, rounded to fp32, divided by its fp32 sum; the 2-D window is
#      the fp32 outer product of that vector with itself (one rounded product per weight), one copy per channel
def gaussian(window_size, sigma):
    c = window_size // 2
    g = torch.tensor([exp(-((i - c) ** 2) / (2.0 * sigma ** 2)) for i in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def create_window(window_size, channel):
    g = gaussian(window_size, 1.5)
    return torch.outer(g, g).float().expand(channel, 1, window_size, window_size).contiguous()


def window_table(window_size=FFA_K):
    """the K x K fp32 weights dhz_ssim_pair takes for the FFA form: create_window's 2-D window (CPU tensor)"""
    return create_window(window_size, 1)[0, 0].contiguous()


_TABLES = {}


def _table(kind, device):
    key = (kind, device)
    if key not in _TABLES:
        t = window_table(FFA_K) if kind == "gauss" else torch.ones(UNI_K, UNI_K)
        _TABLES[key] = t.to(device)
    return _TABLES[key]


def _on_device(*ts):
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts)


def _planes(t):
    """[B, C, H, W] view the kernel can address: rows W apart, unit column stride, image / channel strides >= 0"""
    if t.stride(3) != 1 or t.stride(2) != t.shape[3] or t.stride(0) < 0 or t.stride(1) < 0:
        t = t.contiguous()
    return t


def pair_sums(a, b, K, valid, C1, C2, cov_norm, clamp, window, wscale=1.0):
    """dhz_ssim_pair on fp32 device tensors a, b [B, C, H, W] (any image / channel strides): (ssim_sum, sqerr_sum), two [B, C] float64
    device tensors - the sum of the SSIM map over its extent and the squared-error sum over the plane.  No host sync."""
    if not _on_device(a, b, window):
        raise ValueError("pair_sums: fp32 device tensors only")
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError(f"pair_sums: two [B, C, H, W] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, C, H, W = a.shape
    if K not in (UNI_K, FFA_K) or tuple(window.shape) != (K, K) or min(B, C, H, W) < 1 or (valid and min(H, W) < K):
        raise ValueError(f"pair_sums: unsupported K={K} / window {tuple(window.shape)} / shape {tuple(a.shape)} (valid={bool(valid)})")
    a, b, window = _planes(a), _planes(b), window.contiguous()
    lib = _lib.load()
    nbytes = lib.dhz_ssim_pair_workspace_bytes(B, C, H, W)
    if nbytes == 0:
        raise ValueError(f"pair_sums: shape {tuple(a.shape)} is outside the kernel's range")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(2, B, C, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.call("dhz_ssim_pair", out[0].data_ptr(), out[1].data_ptr(), a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0),
                  b.stride(1), B, C, H, W, K, window.data_ptr(), float(wscale), int(bool(valid)), float(C1), float(C2), float(cov_norm),
                  int(bool(clamp)), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    return out[0], out[1]


def _as4(t):
    return t.unsqueeze(0) if t.dim() == 3 else t


# ---- device forms: per-image float64 tensors [B], no host sync
def _ffa_dev(img1, img2, rmse0=100.0):
    """M:50-68 per image: (ssim [B], psnr [B]); rmse0 is the value of an image whose rmse is 0 (M:66-67: 100)"""
    B, C, H, W = img1.shape
    s, e = pair_sums(img1, img2, FFA_K, False, _C1, _C2, 1.0, True, _table("gauss", img1.device))
    mse = e.sum(1) / (C * H * W)
    psnr = torch.where(mse == 0, torch.full_like(mse, rmse0), 20 * torch.log10(1.0 / torch.sqrt(mse)))
    return s.sum(1) / (C * H * W), psnr


def _uniform_dev(pred, gt):
    """U per image, gt = image_true: (ssim [B], psnr [B], gt.min [B], gt.max [B]); the minimum that picks PSNR's data_range stays on the
    device"""
    B, C, H, W = pred.shape
    R = 2.0
    s, e = pair_sums(gt, pred, UNI_K, True, (0.01 * R) ** 2, (0.03 * R) ** 2, UNI_K ** 2 / (UNI_K ** 2 - 1.0), False,
                     _table("ones", pred.device), 1.0 / UNI_K ** 2)
    ssim = (s / ((H - UNI_K + 1) * (W - UNI_K + 1))).mean(1)
    tmin, tmax = gt.amin(dim=(1, 2, 3)).double(), gt.amax(dim=(1, 2, 3)).double()
    rng = torch.where(tmin >= 0, torch.ones_like(tmin), torch.full_like(tmin, 2.0))
    psnr = 10 * torch.log10(rng * rng / (e.sum(1) / (C * H * W)))
    return ssim, psnr, tmin, tmax


def _check_range(tmin, tmax):
    if tmax > 1 or tmin < -1:
        raise ValueError("image_true has intensity values outside the range expected for its data type")


# ---- the FFA form
def _ssim(img1, img2, window, window_size, channel, size_average=True):
    """M:31-47 (ATen depthwise convolutions, in the dtype of the inputs): the local moments, the map, its mean"""
    def local(t):
        return F.conv2d(t, window, padding=window_size // 2, groups=channel)
    m1, m2 = local(img1), local(img2)
    m11, m22, m12 = m1.pow(2), m2.pow(2), m1 * m2
    v1, v2, v12 = local(img1 * img1) - m11, local(img2 * img2) - m22, local(img1 * img2) - m12
    smap = ((2 * m12 + _C1) * (2 * v12 + _C2)) / ((m11 + m22 + _C1) * (v1 + v2 + _C2))
    return smap.mean() if size_average else smap.mean(1).mean(1).mean(1)


def ssim_gauss(img1, img2, size_average=True):
    """M:50-58, `ssim(img1, img2)` with window_size 11 on [B, C, H, W]: the mean of the map (a 0-dim tensor), or with size_average=False
    one value per image.  fp32 device tensors: the kernel, a float64 tensor on the device, no sync.  Anything else: M's ATen formula."""
    if _on_device(img1, img2):
        s, _ = _ffa_dev(img1, img2)
        return s.mean() if size_average else s            # images of one batch share a size: the mean of the means is the map's mean
    img1 = torch.clamp(img1, min=0, max=1)
    img2 = torch.clamp(img2, min=0, max=1)
    channel = img1.size(1)
    window = create_window(FFA_K, channel).to(img1.device).type_as(img1)
    return _ssim(img1, img2, window, FFA_K, channel, size_average)


def psnr_ffa(pred, gt):
    """M:61-68 over the whole tensor: a Python number (one host sync), 100 when rmse == 0"""
    if _on_device(pred, gt):
        p4, g4 = _as4(pred), _as4(gt)
        _, e = pair_sums(p4, g4, FFA_K, False, _C1, _C2, 1.0, True, _table("gauss", p4.device))
        rmse = math.sqrt(float(e.sum()) / p4.numel())
    else:
        imdff = pred.clamp(0, 1).cpu().numpy() - gt.clamp(0, 1).cpu().numpy()
        rmse = math.sqrt(np.mean(imdff ** 2))
    if rmse == 0:
        return 100
    return 20 * math.log10(1.0 / rmse)


# ---- the uniform form: pred, gt [C, H, W] or [B, C, H, W] float images; Python floats like U (the mean over the images of a batch)
def _host_hwc(t):
    return [im.permute(1, 2, 0).cpu().numpy() for im in _as4(t)]


def ssim_uniform(pred, gt):
    """U:49-60 `structural_similarity(gt, pred, multichannel=True)`: data_range 2"""
    if _on_device(pred, gt):
        return float(_uniform_dev(_as4(pred), _as4(gt))[0].mean())
    from utils.metrics import structural_similarity
    return float(np.mean([structural_similarity(a, b, multichannel=True) for a, b in zip(_host_hwc(gt), _host_hwc(pred))]))


def psnr_uniform(pred, gt):
    """U:17-31 `peak_signal_noise_ratio(gt, pred)`: data_range 1 if gt.min() >= 0 else 2 (the minimum is taken on the device and comes back
    with the score: one sync); inf for identical images"""
    if _on_device(pred, gt):
        _, p, tmin, tmax = (v.tolist() for v in torch.stack(_uniform_dev(_as4(pred), _as4(gt))).cpu())
        _check_range(min(tmin), max(tmax))
        return float(np.mean(p))
    from utils.metrics import peak_signal_noise_ratio
    return float(np.mean([peak_signal_noise_ratio(a, b) for a, b in zip(_host_hwc(gt), _host_hwc(pred))]))


class Scores:
    """Per-image (ssim, psnr) of a validation pass, kept on the device: add_ffa / add_uniform enqueue the kernel for a batch of one size and
    keep its results there; read() copies everything to the host once and returns (ssims, psnrs), two lists of floats, one entry per image in
    the order added.  CPU / non-fp32 inputs are scored by the host formulas and kept as they are."""

    def __init__(self):
        self._rows = []          # [n, 4] float64 tensors: ssim, psnr, gt.min, gt.max (the last two -0 / 0 for the FFA form)
        self.readbacks = 0

    def __len__(self):
        return sum(r.shape[0] for r in self._rows)

    def add_ffa(self, pred, gt, rmse0=100.0):
        pred, gt = _as4(pred), _as4(gt)
        if _on_device(pred, gt):
            s, p = _ffa_dev(pred, gt, rmse0)
        else:
            s = torch.stack([ssim_gauss(a[None], b[None]).double() for a, b in zip(pred, gt)])
            p = torch.tensor([float(psnr_ffa(a, b)) for a, b in zip(pred, gt)], dtype=torch.float64)
        self._rows.append(torch.stack([s, p, torch.zeros_like(s), torch.zeros_like(s)], 1))

    def add_uniform(self, pred, gt):
        pred, gt = _as4(pred), _as4(gt)
        if _on_device(pred, gt):
            self._rows.append(torch.stack(_uniform_dev(pred, gt), 1))
        else:
            rows = [[ssim_uniform(a, b), psnr_uniform(a, b), 0.0, 0.0] for a, b in zip(pred, gt)]
            self._rows.append(torch.tensor(rows, dtype=torch.float64))

    def read(self):
        if not self._rows:
            return [], []
        dev = next((r.device for r in self._rows if r.is_cuda), torch.device("cpu"))
        rows = torch.cat([r.to(dev) for r in self._rows])
        if rows.is_cuda:
            rows = rows.cpu()                    # the one read-back (and sync) of the pass
            self.readbacks += 1
        s, p, tmin, tmax = rows.t().tolist()
        _check_range(min(tmin), max(tmax))
        return s, p
