"""SSIM as a training loss on the HIP kernels: `SSIMLoss()(pred, target) = 1 - ssim(pred, target)`, differentiable with respect to `pred`
(dhz_ssim_loss_fwd / _bwd, csrc/ssim_loss.hip; include/dehaze_hip.h K15), in the two forms the reference has:

  * `SSIMLoss()` - FFA_model/metrics.py (M): 11 x 11 Gaussian window over zero padding of 5, both images clamped to [0, 1] (M:31-58);
  * `SSIMLoss(valid=True, clamp=False)` - Uformer_ProbSparse/aaa.py (A) with val_range=1: the same window without padding (A:42-57).

Routing: fp32 device tensors with a target that does not require grad take the two kernels (float64 arithmetic, no atomics: covered by the
deterministic mode as they are).  Everything else - CPU tensors, other dtypes, a target that requires grad, planes smaller than the window
under `valid` - takes the ATen formula of M / A in the input's dtype.  DHZ_SSIM_LOSS=0 (or ssim_loss.KERNELS = False) forces the ATen
formula: the A/B switch.  Opt-in: nothing on the default paths imports this module.
"""
import os

import torch
import torch.nn.functional as F

from . import _lib

K = 11
KERNELS = os.environ.get("DHZ_SSIM_LOSS", "1") != "0"      # A/B switch: off = the ATen formula everywhere

_TABLES = {}


def _table(device):
    """create_window's 11 x 11 fp32 window (M:19-28, A:8-19) on `device`: the table dehaze_hip.metrics builds, imported on first use"""
    if device not in _TABLES:
        from .metrics import window_table
        _TABLES[device] = window_table(K).to(device)
    return _TABLES[device]


def ssim_aten(img1, img2, valid=False, clamp=True, C1=0.01 ** 2, C2=0.03 ** 2):
    """the reference formula on ATen depthwise convolutions, in the dtype of img1: M:31-58 (valid=False) or A:42-69 (valid=True, where a plane
    smaller than the window shrinks the window as A:45-46 does)"""
    if clamp:
        img1, img2 = torch.clamp(img1, min=0, max=1), torch.clamp(img2, min=0, max=1)
    channel, H, W = img1.shape[1:]
    from .metrics import create_window
    size = min(K, H, W) if valid else K
    window = create_window(size, channel).to(img1.device).type_as(img1)
    pad = 0 if valid else K // 2

    def local(t):
        return F.conv2d(t, window, padding=pad, groups=channel)
    mu1, mu2 = local(img1), local(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = local(img1 * img1) - mu1_sq, local(img2 * img2) - mu2_sq, local(img1 * img2) - mu1_mu2
    smap = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return smap.mean()


class _SSIMLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, valid, C1, C2, clamp):
        pred, target = pred.contiguous(), target.contiguous()
        B, C, H, W = pred.shape
        window = _table(pred.device)
        lib = _lib.load()
        nbytes = lib.dhz_ssim_loss_workspace_bytes(B, C, H, W, int(valid))
        if nbytes == 0:
            raise ValueError(f"SSIMLoss: shape {tuple(pred.shape)} is outside the kernel's range")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        need_grad = bool(ctx.needs_input_grad[0])
        with torch.cuda.device(pred.device):
            _lib.call("dhz_ssim_loss_fwd", loss.data_ptr(), pred.data_ptr(), target.data_ptr(), B, C, H, W, K, window.data_ptr(), int(valid),
                      float(C1), float(C2), int(clamp), int(need_grad), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        if need_grad:
            ctx.save_for_backward(pred, target, window, ws)
            ctx.args = (int(valid), float(C1), float(C2), int(clamp), nbytes)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable          # dx is no differentiable function of pred here: a double backward raises
    def backward(ctx, g):
        pred, target, window, ws = ctx.saved_tensors
        valid, C1, C2, clamp, nbytes = ctx.args
        B, C, H, W = pred.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.call("dhz_ssim_loss_bwd", dx.data_ptr(), g.data_ptr(), pred.data_ptr(), target.data_ptr(), B, C, H, W, K, window.data_ptr(),
                      valid, C1, C2, clamp, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        return dx, None, None, None, None, None


class SSIMLoss(torch.nn.Module):
    """forward(pred, target) -> the 0-dim loss 1 - mean(SSIM map).  valid: the no-padding border rule of A (default: M's zero padding);
    clamp: clamp both images to [0, 1] first, as M does; val_range: L of C1 = (0.01 L)^2, C2 = (0.03 L)^2.  `last_value` keeps the detached
    device scalar of the most recent call, for logging."""

    def __init__(self, valid=False, clamp=True, val_range=1.0):
        super().__init__()
        self.valid, self.clamp = bool(valid), bool(clamp)
        self.C1, self.C2 = (0.01 * val_range) ** 2, (0.03 * val_range) ** 2
        self.last_value = None

    def _on_kernels(self, pred, target):
        if not KERNELS or not (torch.is_tensor(pred) and torch.is_tensor(target)):
            return False
        if not (pred.is_cuda and target.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32):
            return False
        if pred.dim() != 4 or pred.shape != target.shape or pred.device != target.device or pred.numel() == 0:
            return False
        if target.requires_grad and torch.is_grad_enabled():
            return False
        return not (self.valid and min(pred.shape[2:]) < K)

    def forward(self, pred, target):
        if self._on_kernels(pred, target):
            loss = _SSIMLossFn.apply(pred, target, self.valid, self.C1, self.C2, self.clamp)
        else:
            loss = 1 - ssim_aten(pred, target, self.valid, self.clamp, self.C1, self.C2)
        self.last_value = loss.detach()
        return loss
