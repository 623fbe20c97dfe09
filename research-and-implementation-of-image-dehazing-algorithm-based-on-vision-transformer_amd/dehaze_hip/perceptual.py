"""FFA-Net's perceptual loss (FFA_model/models/PerceptualLoss.py; `--perloss` of FFA_model/main.py:89-91,186-191): the mean over three
taps of vgg16().features[:16] - relu1_2, relu2_2, relu3_3 - of the MSE between the features of the dehazed image and of the ground
truth.  No ImageNet normalisation (the reference applies none).

On a HIP device, with frozen filters and an fp32 image whose sides are at least 32 - multiples of 16 (vgg.engine16_shape_ok) or, for whole
images (the reference's default: FFA_model/data_utils.py:21), any other size (vgg.engine16_any_shape_ok; ragged Winograd blocks and
floor-mode poolings whose backward writes the dropped odd row / column too; DHZ_PERLOSS_ANY=0 / perceptual.ANY = False: off) -, the
stack runs on the Winograd engine of dehaze_hip/vgg.py built as VggEngine(7 convolutions, pool_after (1, 3), taps (1, 3, 6)): one
no-gradient pass for the ground truth, one differentiated pass for the dehazed image, features channel-blocked throughout, the three
squared-error sums into one zeroed 3-float buffer (dhz_mse_pair_fwd) and ONE autograd node whose backward is three dhz_mse_pair_bwd
launches (the last with the ReLU mask) and the engine's walk down the stack.  Any other input runs the plain layers with F.mse_loss -
one ops.warn_library_fallback warning per shape when only the shape is in the way.

VGG16 weights: the reference pulls torchvision's ImageNet checkpoint at run time (main.py:187).  That file is a third-party artefact,
so LossNetwork loads a user-supplied torchvision state_dict (`weights=` or $DEHAZE_VGG16_WEIGHTS, keys `features.N.*`) and otherwise
draws SEEDED RANDOM weights with a warning, as My_CR.Vgg19 does."""
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

# torchvision cfg 'D' up to features[15]
VGG16_CFG = (64, 64, 'M', 128, 128, 'M', 256, 256, 256)
POOL_AFTER16 = (1, 3)
TAPS16 = (1, 3, 6)                               # relu1_2, relu2_2, relu3_3 = features[3], [8], [15]
TAP_LAYERS = {3: "relu1_2", 8: "relu2_2", 15: "relu3_3"}
VGG16_SEED = 1606
# A/B switch: image sizes that are no multiples of 16 (sides from 32 up) on the engine - its `_any` convolutions and floor-mode poolings -, and
# the image-space L1 of ffa_train_step on any element count (off: such sizes on the library path, with the warning)
ANY = os.environ.get("DHZ_PERLOSS_ANY", "1") != "0"


def vgg16_feature_layers():
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return layers          # 16 entries = torchvision vgg16().features[0:16]


def seeded_vgg16_init_(layers, seed=VGG16_SEED):
    """He-scaled normal filters and small normal biases for the 7 convolutions, drawn in order from a generator of its own"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in layers:
            if isinstance(m, nn.Conv2d):
                cout, cin = m.weight.shape[:2]
                m.weight.copy_(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5)
                m.bias.copy_(torch.randn(cout, generator=g) * 0.05)


def _is_vgg16_head(seq):
    """the 16 layers of vgg16().features[:16]: what the engine restates"""
    want = vgg16_feature_layers()
    mods = list(seq.children()) if isinstance(seq, nn.Sequential) else None
    if mods is None or len(mods) != len(want):
        return False
    for m, w in zip(mods, want):
        if type(m) is not type(w):
            return False
        if isinstance(m, nn.Conv2d) and (m.weight.shape != w.weight.shape or m.bias is None or m.kernel_size != (3, 3)
                                         or m.padding != (1, 1) or m.stride != (1, 1) or m.dilation != (1, 1) or m.groups != 1):
            return False
        if isinstance(m, nn.MaxPool2d) and (m.kernel_size not in (2, (2, 2)) or m.stride not in (2, (2, 2)) or m.padding not in (0, (0, 0))
                                            or m.ceil_mode):
            return False
    return True


_COEF = {}


class _PerLossTaps(Function):
    """loss = mean_i mean((taps_i(x) - gt_i)^2) as one autograd node: the differentiated pass over the stack, the three squared-error sums,
    and in the backward three dhz_mse_pair_bwd launches followed by the engine's backward walk.  Gradient w.r.t. x only."""

    @staticmethod
    def forward(ctx, engine, x, *gt_taps):
        from . import _lib, ops
        need = ctx.needs_input_grad[1]
        saved = {} if need else None
        taps = [t.contiguous() for t in engine.forward_taps(x, save=saved)]
        gts = [t.contiguous() for t in gt_taps]
        k = len(taps)
        dev = x.device
        key = (str(dev), tuple(t.numel() for t in taps))
        if key not in _COEF:
            _COEF[key] = torch.tensor([1.0 / (k * t.numel()) for t in taps], dtype=torch.float32).to(dev)
        sums = ops.zeros_f32((k,), dev)
        for i in range(k):
            _lib.call("dhz_mse_pair_fwd", ops._p(taps[i]), ops._p(gts[i]), sums.data_ptr() + 4 * i, taps[i].numel(), ops._stream())
        out = (sums * _COEF[key]).sum()
        if need:
            ctx.engine, ctx.saved, ctx.taps, ctx.gts = engine, saved, taps, gts
        return out

    @staticmethod
    def backward(ctx, g):
        from . import _lib, ops
        taps, gts = ctx.taps, ctx.gts
        k = len(taps)
        gmean = (g.to(torch.float32) * (1.0 / k)).reshape(1).contiguous()          # d loss / d mean_i, the same for every tap
        das = []
        for i in range(k):
            da = torch.empty_like(taps[i])
            # the last tap is where the first gradient enters the stack: its ReLU is applied here
            _lib.call("dhz_mse_pair_bwd", ops._p(taps[i]), ops._p(gts[i]), ops._p(gmean), ops._p(da), taps[i].numel(), int(i == k - 1),
                      ops._stream())
            das.append(da)
        gx = ctx.engine.backward_taps(ctx.saved, das, last_masked=True)
        ctx.saved = ctx.taps = ctx.gts = None
        return (None, gx) + (None,) * k


class LossNetwork(nn.Module):
    def __init__(self, vgg_model=None, weights=None):
        """vgg_model: an nn.Sequential with the 16 layers of vgg16().features[:16] (the reference's call; used as it is), or None: built
        here, frozen, filled from `weights` / $DEHAZE_VGG16_WEIGHTS (a torchvision vgg16 state_dict) or seeded-random with a warning."""
        super().__init__()
        self.pretrained = None
        if vgg_model is None:
            layers = vgg16_feature_layers()
            vgg_model = nn.Sequential(*layers)
            weights = weights or os.environ.get("DEHAZE_VGG16_WEIGHTS")
            if weights:
                sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, os.PathLike)) else weights
                sd = sd.get("state_dict", sd)
                mine = vgg_model.state_dict()
                for k in mine:                                   # '5.weight' <- 'features.5.weight'
                    src = sd.get("features." + k, sd.get(k))
                    if src is None:
                        raise KeyError(f"VGG16 weight file lacks features.{k}")
                    mine[k].copy_(src)
                self.pretrained = True
            else:
                warnings.warn("LossNetwork: no ImageNet checkpoint available offline - using SEEDED RANDOM weights "
                              "(set DEHAZE_VGG16_WEIGHTS=/path/to/vgg16-397923af.pth for the reference behaviour)")
                seeded_vgg16_init_(layers)
                self.pretrained = False
            for p in vgg_model.parameters():
                p.requires_grad = False
        self.vgg_layers = vgg_model
        self.layer_name_mapping = {str(k): v for k, v in TAP_LAYERS.items()}
        self._head_ok = _is_vgg16_head(vgg_model)
        self._engine = None

    def engine_for(self, x):
        """the Winograd engine (dehaze_hip/vgg.py) when it applies, else None: the plain layers"""
        if not (self._head_ok and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
            return None
        if x.dtype != torch.float32 or any(p.requires_grad for p in self.vgg_layers.parameters()) \
                or self.vgg_layers[0].weight.device != x.device or self.vgg_layers[0].weight.dtype != torch.float32:
            return None
        from . import ops
        from .vgg import VggEngine, engine16_any_shape_ok, engine16_shape_ok
        if not (engine16_shape_ok(x.shape[2], x.shape[3]) or (ANY and engine16_any_shape_ok(x.shape[2], x.shape[3]))):
            ops.warn_library_fallback("PerLoss VGG16", (3, x.shape[2], x.shape[3]))
            return None
        if self._engine is None:
            self._engine = VggEngine([m for m in self.vgg_layers if isinstance(m, nn.Conv2d)], POOL_AFTER16, TAPS16)
        return self._engine

    def _plain_features(self, x):
        output = []
        for name, module in self.vgg_layers._modules.items():
            x = module(x)
            if name in self.layer_name_mapping:          # (behind a tap comes a pooling or the end: nothing writes the tap in place)
                output.append(x)
        return output

    def output_features(self, x):
        """the three taps (relu1_2, relu2_2, relu3_3) as plain NCHW tensors"""
        eng = self.engine_for(x)
        if eng is not None:
            from . import vgg as _v
            return [_v.to_plain_tap(t) for t in _v.vgg_taps(eng, x)]
        return self._plain_features(x)

    def forward(self, dehaze, gt):
        eng = self.engine_for(dehaze) if dehaze.shape == gt.shape and gt.dtype == dehaze.dtype and gt.device == dehaze.device else None
        if eng is not None:
            with torch.no_grad():
                gt_taps = eng.forward_taps(gt)
            return _PerLossTaps.apply(eng, dehaze, *gt_taps)
        return self.forward_library(dehaze, gt)

    def forward_library(self, dehaze, gt):
        """the reference's forward on the plain layers (PerceptualLoss.py:24-31): any device, any dtype"""
        df, gf = self._plain_features(dehaze), self._plain_features(gt)
        loss = [F.mse_loss(a, b) for a, b in zip(df, gf)]
        return sum(loss) / len(loss)


PerLoss = LossNetwork
