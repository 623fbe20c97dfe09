"""Drop-in for FFA_model/metrics.py: `gaussian`, `create_window`, `_ssim`, `ssim`, `psnr` - the validation metrics of FFA-Net's recipe
(FFA_model/main.py:151-173: `ssim(pred, targets).item()`, `psnr(pred, targets)` per validation image).

`ssim` / `psnr` route through dehaze_hip.metrics: fp32 device tensors are scored by the float64 HIP kernel (dhz_ssim_pair), anything else
by the reference's ATen / numpy formula.  On the device `ssim` returns a float64 tensor there (`.item()` as the reference's caller does);
`psnr` returns a Python number, 100 for identical images.  The reference's `window_size` argument exists for 11 only on the device.
"""
from dehaze_hip.metrics import _ssim, create_window, gaussian, psnr_ffa, ssim_gauss  # noqa: F401


def ssim(img1, img2, window_size=11, size_average=True):
    if window_size != 11:
        raise NotImplementedError(f"ssim: window_size {window_size}: the recipe and the kernel use 11")
    return ssim_gauss(img1, img2, size_average)


def psnr(pred, gt):
    return psnr_ffa(pred, gt)
