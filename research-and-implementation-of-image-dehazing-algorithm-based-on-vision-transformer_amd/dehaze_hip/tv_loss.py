"""The two total-variation losses of Uformer_ProbSparse/losses.py (L) on the HIP kernels (dhz_tv_loss_fwd / _bwd, csrc/tv_loss.hip;
include/dehaze_hip.h K16), with the reference's names and defaults:

  * `tv_loss(x, beta=0.5, reg_coeff=5)` - L:8-18, form "beta": reg_coeff * sum(s ** beta) / x.numel() over the (H - 1) x (W - 1) sites
    s = (x[i,j+1] - x[i,j]) ** 2 + (x[i+1,j] - x[i,j]) ** 2 of every plane;
  * `TVLoss(tv_loss_weight=1)` - L:20-37, form "sq": weight * 2 * (sum_v / (C (H - 1) W) + sum_h / (C H (W - 1))) / B over the squared
    vertical and horizontal first differences;
  * `TVTerm(form='sq' | 'beta', beta=0.5)` - either of them as a training term with `last_value` for logging.

The one deviation from the reference, the zero-site rule: a site with s == 0 exactly contributes 0 to the gradient.  Autograd of L:18 gives
beta * 0 ** (beta - 1) * 0 = inf * 0 = NaN there for beta < 1, at every pixel of such a site, and an image clamped to [0, 1] always has such
sites.  The value is unaffected (0 ** beta = 0), the other sites of the same pixels contribute as ever, and both routes obey the rule.

Routing: fp32 device tensors [B, C, H, W] with H, W >= 2 take the kernels (float64 arithmetic, no atomics: covered by the deterministic
mode as they are).  Everything else - CPU tensors, other dtypes, planes without a site - takes the ATen formula in the input's dtype.
DHZ_TV_LOSS=0 (or tv_loss.KERNELS = False) forces the ATen formula: the A/B switch.  Opt-in: nothing on the default paths imports this
module.
"""
import math
import os

import torch

from . import _lib

KERNELS = os.environ.get("DHZ_TV_LOSS", "1") != "0"        # A/B switch: off = the ATen formula everywhere
FORMS = {"beta": 0, "sq": 1}


def tv_beta_aten(x, beta=0.5, reg_coeff=5):
    """L:15-18 in the dtype of x, with the power guarded so that autograd obeys the zero-site rule: a site with s == 0 is 0 and passes no
    gradient.  A plane with H < 2 or W < 2 has no site: value 0, gradient 0."""
    dh = (x[:, :, :-1, 1:] - x[:, :, :-1, :-1]) ** 2
    dv = (x[:, :, 1:, :-1] - x[:, :, :-1, :-1]) ** 2
    s = dh + dv
    zero = s == 0
    powed = torch.where(zero, torch.ones_like(s), s) ** beta
    return reg_coeff * (torch.where(zero, torch.zeros_like(s), powed).sum() / x.numel())


def tv_sq_aten(x, weight=1):
    """L:25-33 in the dtype of x; a plane with H < 2 or W < 2 gives the reference's 0 / 0 = NaN"""
    B, C, H, W = x.shape
    sum_v = ((x[:, :, 1:, :] - x[:, :, :-1, :]) ** 2).sum()
    sum_h = ((x[:, :, :, 1:] - x[:, :, :, :-1]) ** 2).sum()
    return weight * 2 * (sum_v / (C * (H - 1) * W) + sum_h / (C * H * (W - 1))) / B


class _TVLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, form, beta, coeff):
        x = x.contiguous()
        B, C, H, W = x.shape
        lib = _lib.load()
        nbytes = lib.dhz_tv_loss_workspace_bytes(B, C, H, W)
        if nbytes == 0:
            raise ValueError(f"tv_loss: shape {tuple(x.shape)} is outside the kernel's range")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("dhz_tv_loss_fwd", loss.data_ptr(), x.data_ptr(), B, C, H, W, form, beta, coeff, ws.data_ptr(), nbytes,
                      torch.cuda.current_stream().cuda_stream)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x)
            ctx.args = (form, beta, coeff)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable          # dx is no differentiable function of x here: a double backward raises
    def backward(ctx, g):
        x, = ctx.saved_tensors
        form, beta, coeff = ctx.args
        B, C, H, W = x.shape
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.call("dhz_tv_loss_bwd", dx.data_ptr(), g.data_ptr(), x.data_ptr(), B, C, H, W, form, beta, coeff,
                      torch.cuda.current_stream().cuda_stream)
        return dx, None, None, None


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _on_kernels(x, beta, coeff):
    if not KERNELS or not torch.is_tensor(x) or not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        return False
    if not (_number(beta) and beta > 0 and _number(coeff)):
        return False
    B, C, H, W = x.shape
    return H >= 2 and W >= 2 and _lib.load().dhz_tv_loss_workspace_bytes(B, C, H, W) > 0


def tv_loss(x, beta=0.5, reg_coeff=5):
    """L:8-18 with the zero-site rule: never a NaN gradient"""
    if _on_kernels(x, beta, reg_coeff):
        return _TVLossFn.apply(x, FORMS["beta"], float(beta), float(reg_coeff))
    return tv_beta_aten(x, beta, reg_coeff)


class TVLoss(torch.nn.Module):
    """L:20-37: forward(x) -> tv_loss_weight * 2 * (h_tv / count_h + w_tv / count_w) / batch_size"""

    def __init__(self, tv_loss_weight=1):
        super().__init__()
        self.tv_loss_weight = tv_loss_weight

    def forward(self, x):
        if _on_kernels(x, 0.5, self.tv_loss_weight):
            return _TVLossFn.apply(x, FORMS["sq"], 0.5, float(self.tv_loss_weight))
        return tv_sq_aten(x, self.tv_loss_weight)

    @staticmethod
    def tensor_size(t):
        return t.shape[1] * t.shape[2] * t.shape[3]


class TVTerm(torch.nn.Module):
    """forward(x) -> the 0-dim term: TVLoss()(x) under form 'sq', tv_loss(x, beta) with the reference's reg_coeff = 5 under form 'beta'.
    `last_value` keeps the detached device scalar of the most recent call, for logging."""

    def __init__(self, form="sq", beta=0.5):
        super().__init__()
        if form not in FORMS:
            raise ValueError(f"TVTerm: form={form!r} ('sq' or 'beta')")
        if not (_number(beta) and beta > 0):
            raise ValueError(f"TVTerm: beta={beta} (finite and > 0)")
        self.form, self.beta = form, float(beta)
        self._sq = TVLoss()
        self.last_value = None

    def forward(self, x):
        loss = self._sq(x) if self.form == "sq" else tv_loss(x, self.beta)
        self.last_value = loss.detach()
        return loss
