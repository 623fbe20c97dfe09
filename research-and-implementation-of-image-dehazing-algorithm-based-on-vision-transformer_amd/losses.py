"""Drop-in for Uformer_ProbSparse/losses.py: CharbonnierLoss (losses.py:41-52) on the fused HIP
reduction kernel (dhz_charbonnier_fwd/bwd); tv_loss (losses.py:8-18) and TVLoss (losses.py:20-37) on
dhz_tv_loss_fwd/bwd, loaded from dehaze_hip/tv_loss.py when first asked for."""
import torch.nn as nn

from dehaze_hip import ops

_LAZY = ("tv_loss", "TVLoss")


def __getattr__(name):
    """`from losses import TVLoss, tv_loss` works; `import losses` alone does not load dehaze_hip.tv_loss"""
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("dehaze_hip.tv_loss"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_LAZY))


class CharbonnierLoss(nn.Module):
    """mean(sqrt((x-y)^2 + eps^2)), eps = 1e-3."""

    def __init__(self, eps=1e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        return ops.charbonnier(x, y, self.eps)

    def forward_clamped(self, x, y):
        """(loss(clamp(x,0,1), y), clamp(x,0,1)) in one pass - the train step's TR:230+234."""
        return ops.charbonnier_clamped(x, y, self.eps)
