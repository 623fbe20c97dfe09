"""VGG19[:30] feature stack of the contrastive loss (My_CR.py:56-86) on the Winograd-MFMA convolution kernel.

conv 0 (3 -> 64) runs thin-input kernels (dhz_conv3x3_in3_blocked forward with bias + ReLU straight into the blocked layout,
dhz_thin_conv3x3_dgrad_blocked backward-data straight from it); convs 1..12 run dhz_winograd_conv3x3 with bias + ReLU fused,
in the channel-blocked NCHW8c layout end to end (conv 12 works on 8x8 maps for 128x128 patches: the kernel then packs four
images into one of its 16x16 blocks).  Maps that are neither multiples of 16 nor 8x8 - the 8x8 / 4x4 maps of 64-pixel patches, 24x24 and
12x12 at 192, 30x30 and 15x15 at 240, 24x24 at 384 - run dhz_winograd_conv3x3_any: the same kernel with ragged blocks at the right and
bottom edges, and sixteen 4x4 images per block.  Every patch whose sides are multiples of 16 and at least 64 pixels (engine_shape_ok)
therefore runs the whole stack on these kernels; no layer goes to the library.  The filters are frozen
(My_CR.py:75-77), so their transform-domain forms (forward and backward-data) are prepacked once per device.

Launches whose grid leaves CUs idle (the 8 x 8 maps; the 16 x 16 maps of the 32 differentiated images) run with their input-channel
contraction cut into 2 or 4 slices side by side (dhz_winograd_conv3x3_slices, dhz_winograd43_conv3x3_slices) and one small kernel that adds
the parts and applies the store epilogue - see SLICES_ON below (DHZ_WINO_SLICES=0: the plain launches).

Forward-only passes (target / hazy input, My_CR.py:102) save nothing; the pass on the restored image is one autograd
node whose backward walks the stack with the same kernel (rotated/transposed filters, ReLU mask fused into the patch
load) - weight gradients are never formed (the reference freezes the VGG, My_CR.py:75-77).

The stack is a parameter of the engine: VggEngine(convs, pool_after, taps).  The defaults are VGG19[:30] with the five taps above; the
perceptual loss of FFA-Net's recipe (dehaze_hip/perceptual.py) builds the 7 convolutions of VGG16[:16] with pool_after (1, 3) and taps
(1, 3, 6).  There two taps are pooled as well: their un-pooled maps are always written, and in the backward the tap's gradient joins
the pooled one on the un-pooled map in one launch (dhz_maxpool2x2_blocked_bwd_add, csrc/perceptual.hip).  That stack also takes whole
images of any size from 32 x 32 up (engine16_any_shape_ok): a map with an odd side is pooled in floor mode by the `_any` pooling entries
(csrc/winograd_conv.hip), whose backward writes the dropped row / column too; even maps keep the launches they always had.
"""
import os

import torch
from torch.autograd import Function

from . import _lib
from . import ops
from .ops import _p, _stream

CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 512),
         (512, 512), (512, 512), (512, 512), (512, 512))
POOL_AFTER = (1, 3, 7, 11)
TAPS = (0, 2, 4, 8, 12)          # relu1_1, relu2_1, relu3_1, relu4_1, relu5_1


def engine_shape_ok(H, W):
    """Image sizes the fp32 engine takes: both sides multiples of 16 (four even poolings, then conv5_1 on H / 16 x W / 16 maps of any size)
    and at least 64.  Below 64 the last maps are 2 x 2 and 1 x 1, and the 32-pixel model test holds the contrastive loss's gradient to a
    bound that the library's arithmetic meets and the Winograd transform's does not: those sizes stay on the library."""
    return H % 16 == 0 and W % 16 == 0 and H >= 64 and W >= 64


def engine16_shape_ok(H, W):
    """Image sizes the VGG16[:16] stack of the perceptual loss takes (dehaze_hip/perceptual.py): two poolings only, so sides that are multiples
    of 16 and at least 32 - the last maps are then 8 x 8 and larger (FFA's own blocked path asks for multiples of 16 too)."""
    return H % 16 == 0 and W % 16 == 0 and H >= 32 and W >= 32


def engine16_any_shape_ok(H, W):
    """Whole images (FFA_model/data_utils.py:21): the VGG16[:16] stack on any H x W with both sides at least 32.  The convolutions take any map
    (dhz_conv3x3_in3_blocked, dhz_winograd_conv3x3_any, dhz_thin_conv3x3_dgrad_blocked), the two poolings run in floor mode on odd maps
    (dhz_maxpool2x2_blocked_*_any).  The floor is engine16_shape_ok's: the last maps are 8 x 8 and larger."""
    return H >= 32 and W >= 32


def _fixed_tiling(H, W):
    """map sizes dhz_winograd_conv3x3 takes (multiples of 16, or 8x8: four images per block); every other size runs dhz_winograd_conv3x3_any"""
    return (H % 16 == 0 and W % 16 == 0) or (H == 8 and W == 8)


def any_blocks(B, H, W):
    """dhz_winograd_any_blocks, restated for the host tests: the 16 x 16 blocks a dhz_winograd_conv3x3_any launch walks (0: bad arguments)"""
    if B <= 0 or H < 1 or W < 1:
        return 0
    if H == 4 and W == 4:
        return (B + 15) // 16
    if H == 8 and W == 8:
        return (B + 3) // 4
    return B * ((H + 15) // 16) * ((W + 15) // 16)


def to_blocked(x, bias=None, relu=False):
    """NCHW -> NCHW8c; optionally max(x + bias[c], 0) on the way (the bias + ReLU behind a library convolution)."""
    B, C, H, W = x.shape
    out = torch.empty((B, C // 8, H, W, 8), device=x.device, dtype=torch.float32)
    _lib.call("dhz_layout_blocked8", _p(x.contiguous()), _p(out), B, C, H * W, 1, _p(bias), int(relu), _stream())
    return out


def to_plain(xb):
    B, CG, H, W, _ = xb.shape
    out = torch.empty((B, CG * 8, H, W), device=xb.device, dtype=torch.float32)
    _lib.call("dhz_layout_blocked8", _p(xb), _p(out), B, CG * 8, H * W, 0, None, 0, _stream())
    return out


def _pool_sfx(H, W):
    """an odd side: the `_any` pooling entries (floor mode, the dropped row / column written too); even maps keep the entries they always ran"""
    return "_any" if (H % 2 or W % 2) else ""


def pool_fwd(xb):
    B, CG, H, W, _ = xb.shape
    yb = torch.empty((B, CG, H // 2, W // 2, 8), device=xb.device, dtype=torch.float32)
    _lib.call("dhz_maxpool2x2_blocked_fwd" + _pool_sfx(H, W), _p(xb), _p(yb), B * CG, H, W, _stream())
    return yb


def pool_bwd_relu(gb, actb):
    """gradient w.r.t. the pre-activation below the post-ReLU map `actb` whose 2x2 max pooling received gradient gb."""
    B, CG, H, W, _ = actb.shape
    gx = torch.empty_like(actb)
    _lib.call("dhz_maxpool2x2_blocked_bwd" + _pool_sfx(H, W), _p(gb.contiguous()), _p(actb), _p(gx), B * CG, H, W, _stream())
    return gx


def pool_bwd_relu_add(gb, actb, addb):
    """pool_bwd_relu for a map that is a loss tap as well: + the tap's own gradient addb, both through the ReLU (actb > 0), in one launch."""
    B, CG, H, W, _ = actb.shape
    gx = torch.empty_like(actb)
    _lib.call("dhz_maxpool2x2_blocked_bwd_add" + _pool_sfx(H, W), _p(gb.contiguous()), _p(actb), _p(addb.contiguous()), _p(gx), B * CG, H, W,
              _stream())
    return gx


def _timing_end(ev, B, H, W, Cin, Kout, f43=False):
    direct = 2.0 * 9 * B * H * W * Cin * Kout                                 # direct-convolution FLOPs of this launch
    # ISSUED matrix FLOPs: F(2x2,3x3) multiplies 16 / 4 per output and tap-sum instead of 9 (direct / 2.25), F(4x4,3x3) 36 / 16 (/ 4)
    ops._timed_end(ev, direct, direct / (4.0 if f43 else 2.25))


# Which Winograd form a layer takes: F(4x4,3x3) (csrc/winograd43_conv.hip, 1.78 x fewer matrix products) or F(2x2,3x3)
# (csrc/winograd_conv.hip).  Measured per layer (tools/bench_wino.py): F(4x4) is 1.14 - 1.22 x faster whenever its grid - one workgroup
# per four 16 x 16 blocks and 32 output channels - fills the CUs in whole rounds: always on the 128 / 64 / 32-pixel maps (thousands of
# workgroups), on the 16-pixel maps only for some batches (64 images x 512 channels = 256 workgroups = one round: faster; 96 images = 1.5
# rounds: 0.91 x; 32 images = half a round: slower still) - hence the occupancy rule below.  DHZ_WINO_F43=0 disables the F(4x4) form.
F43_ON = os.environ.get("DHZ_WINO_F43", "1") != "0"


# F(4x4) also in the DIFFERENTIATED forward pass (the pass whose roundings decide the ReLU masks of the backward pass).  Rounds 4 - 5 kept that
# pass on F(2x2) by an argument (three times the near-zero units flip); round 6 measured it (tools/wino_f43_diff.py, profiles/
# r06_wino_f43_diff.txt): over 50 training steps the loss differs from the all-F(2x2)-forward run by <= 1.6e-4 - inside the run-to-run spread of
# the F(2x2) step itself (atomics) -, d(loss)/d(restored) at equal weights by 9e-4 of its mean, every kernel- and model-level tolerance of
# tests/ holds unchanged with it, and the step gains 0.13 - 0.28 ms.  DHZ_WINO_F43_DIFF=0 restores the F(2x2) forward.
F43_DIFF = os.environ.get("DHZ_WINO_F43_DIFF", "1") != "0"
POOL_FUSED = os.environ.get("DHZ_WINO_POOL", "1") != "0"    # A/B switch: the pooling of the no-gradient pass inside the F(4x4) launch


def use_f43(B, H, W, Cin, Kout):
    if not F43_ON or H % 16 or W % 16 or H < 16 or W < 16 or Cin % 16 or Kout % 32:
        return False
    wgs = (B * (H // 16) * (W // 16) + 3) // 4 * (Kout // 32)
    cus = _lib.load().dhz_grid_cus() + _lib.load().dhz_get_reserved_cus()      # PHYSICAL CUs: this grid is not persistent, a reservation does not shrink it
    rounds = (wgs + cus - 1) // cus
    return wgs >= 0.92 * rounds * cus          # the last round of workgroups nearly full


# Channel slices (csrc/winograd_conv.hip RAW, csrc/winograd43_conv.hip SL): a launch whose grid leaves CUs idle - the 8 x 8 and 16 x 16 maps of
# 32 or 64 images - costs the serial walk of ONE workgroup over all input-channel groups.  Such a launch runs as S copies of its grid, each over
# 1 / S of the channel groups, into a workspace, and a small kernel adds the parts in a fixed order and applies the store epilogue.  Where
# use_f43 refuses F(4x4) only because its grid is half a round or less, S parallel chain links fill the round (use_f43_slices); what is left
# asks the library (dhz_winograd_slices) for the F(2x2) launch.  DHZ_WINO_SLICES=0 restores the plain launches (A/B switch).
SLICES_ON = os.environ.get("DHZ_WINO_SLICES", "1") != "0"


def _physical_cus():
    return _lib.load().dhz_grid_cus() + _lib.load().dhz_get_reserved_cus()


def f43_slices_rule(B, H, W, Cin, Kout, cus):
    """Slice count (2 or 4; 0 = none) at which the F(4x4) kernel's parallel chain links fill one round of `cus` CUs where its plain grid is
    half a round or less: the shape preconditions and the 0.92 rule of use_f43 on S x wgs <= cus workgroups, equal slices of SLICE_MIN_GROUPS
    to 32 channel groups (one accumulation chain at the most).  The smallest such S: fewer parts to add, and S = 2 on 512 channels is the chained launch bit for bit."""
    if H % 16 or W % 16 or H < 16 or W < 16 or Cin % 16 or Kout % 32:
        return 0
    wgs = (B * (H // 16) * (W // 16) + 3) // 4 * (Kout // 32)
    rounds = (wgs + cus - 1) // cus
    if wgs >= 0.92 * rounds * cus:                 # use_f43's own case: the plain launch
        return 0
    CBn = Cin // 8
    for S in (2, 4):
        # one round at the most: the parts travel through memory, which only pays for the small maps whose launch time is the serial walk
        if CBn % S == 0 and SLICE_MIN_GROUPS <= CBn // S <= 32 and 0.92 * cus <= S * wgs <= cus:
            return S
    return 0


def use_f43_slices(B, H, W, Cin, Kout):
    return f43_slices_rule(B, H, W, Cin, Kout, _physical_cus()) if (F43_ON and SLICES_ON) else 0


SLICE_MIN_GROUPS = 16         # csrc/winograd_conv.hip: the shortest slice measured to win


def wino_slices_rule(B, H, W, C, K, cus):
    """The rule of dhz_winograd_slices (the F(2x2) launch), restated for the host tests: the largest S in {1, 2, 4} whose S copies of the
    plain grid fit `cus` CUs with at least SLICE_MIN_GROUPS channel groups per slice.  The dispatch asks the library."""
    q8 = H == 8 and W == 8
    if B <= 0 or not ((H % 16 == 0 and W % 16 == 0 and H > 0) or q8) or C % 8 or K % 32:
        return 1
    nblk = (B + 3) // 4 if q8 else B * (H // 16) * (W // 16)
    grid = (nblk + 1) // 2 * (K // 32)
    for S in (4, 2):
        if S * grid <= cus and (C // 8) // S >= SLICE_MIN_GROUPS:
            return S
    return 1


def wino_slices_any_rule(B, H, W, C, K, cus):
    """The rule of dhz_winograd_slices_any, restated for the host tests: wino_slices_rule on the block count of the any-size launch."""
    if B <= 0 or H < 1 or W < 1 or C <= 0 or K <= 0 or C % 8 or K % 32:
        return 1
    grid = (any_blocks(B, H, W) + 1) // 2 * (K // 32)
    for S in (4, 2):
        if S * grid <= cus and (C // 8) // S >= SLICE_MIN_GROUPS:
            return S
    return 1


class VggEngine:
    def __init__(self, convs, pool_after=POOL_AFTER, taps=TAPS):
        """convs: the nn.Conv2d modules of the stack - by default the 13 of vgg19.features[0:30]; pool_after: the convolutions a 2 x 2 max
        pooling follows; taps: the convolutions whose post-ReLU maps are returned, the last tap being the last convolution.  The 7
        convolutions of vgg16.features[0:16] with pool_after (1, 3) and taps (1, 3, 6) are the perceptual loss's stack (perceptual.py)."""
        self.convs = list(convs)
        self.conv_shapes = tuple((int(c.weight.shape[1]), int(c.weight.shape[0])) for c in self.convs)
        self.pool_after = tuple(pool_after)
        self.taps = tuple(taps)
        if not self.taps or self.taps[-1] != len(self.convs) - 1 or list(self.taps) != sorted(set(self.taps)):
            raise ValueError(f"VggEngine: taps {self.taps} must ascend and end at the last of the {len(self.convs)} convolutions")
        if self.conv_shapes[0] != (3, 64) or any(c % 8 or k % 32 for c, k in self.conv_shapes[1:]):
            raise ValueError(f"VggEngine: unsupported convolution shapes {self.conv_shapes}")
        self._packed = {}
        self._packed43 = {}

    def packed(self, i, device):
        key = (i, str(device), self.convs[i].weight.data_ptr(), self.convs[i].weight._version)
        hit = self._packed.get(i)
        if hit is None or hit[0] != key:
            w = self.convs[i].weight.detach().contiguous()
            K, C = w.shape[0], w.shape[1]
            uf = torch.empty(16 * K * C, device=device, dtype=torch.float32)
            ub = torch.empty(16 * K * C, device=device, dtype=torch.float32)
            _lib.call("dhz_winograd_prepack", _p(w), _p(uf), K, C, 0, _stream())
            _lib.call("dhz_winograd_prepack", _p(w), _p(ub), C, K, 1, _stream())
            hit = (key, uf, ub)
            self._packed[i] = hit
        return hit[1], hit[2]

    def packed43(self, i, device):
        """F(4x4,3x3) filters of layer i (forward and backward-data forms, 36 K C floats each), built at first use"""
        key = (i, str(device), self.convs[i].weight.data_ptr(), self.convs[i].weight._version)
        hit = self._packed43.get(i)
        if hit is None or hit[0] != key:
            w = self.convs[i].weight.detach().contiguous()
            K, C = w.shape[0], w.shape[1]
            uf = torch.empty(36 * K * C, device=device, dtype=torch.float32)
            ub = torch.empty(36 * K * C, device=device, dtype=torch.float32)
            _lib.call("dhz_winograd43_prepack", _p(w), _p(uf), K, C, 0, _stream())
            _lib.call("dhz_winograd43_prepack", _p(w), _p(ub), C, K, 1, _stream())
            hit = (key, uf, ub)
            self._packed43[i] = hit
        return hit[1], hit[2]

    # ---- one Winograd layer
    def conv(self, i, xb, allow43=True, pool=False):
        """conv i + bias + ReLU; pool=True: + the 2 x 2 max pooling behind it, in the same launch when the layer runs the F(4x4) kernel (the
        un-pooled map is then never written: only for layers whose output is no tap and is not saved)."""
        B, CG, H, W, _ = xb.shape
        C, K = self.conv_shapes[i]
        f43 = allow43 and use_f43(B, H, W, C, K)
        s43 = use_f43_slices(B, H, W, C, K) if (allow43 and not f43) else 0
        sfx = "" if _fixed_tiling(H, W) else "_any"             # (F(4x4) never applies to the `_any` shapes: use_f43 wants multiples of 16)
        s22 = getattr(_lib.load(), "dhz_winograd_slices" + sfx)(B, H, W, C, K) if (SLICES_ON and not f43 and not s43) else 1
        uf, _ = self.packed43(i, xb.device) if (f43 or s43) else self.packed(i, xb.device)
        if pool and f43:
            yp = torch.empty((B, K // 8, H // 2, W // 2, 8), device=xb.device, dtype=torch.float32)
            scratch = torch.empty((B, K // 8, H, W, 8), device=xb.device, dtype=torch.float32) if C > 256 else None
            ev = ops._timed("dhz_winograd_conv3x3")
            _lib.call("dhz_winograd43_conv3x3_pool", _p(xb), _p(uf), _p(self.convs[i].bias), _p(yp), _p(scratch) if scratch is not None else None,
                      B, H, W, C, K, _stream())
            _timing_end(ev, B, H, W, C, K, f43)
            return yp
        yb = torch.empty((B, K // 8, H, W, 8), device=xb.device, dtype=torch.float32)
        ev = ops._timed("dhz_winograd_conv3x3")
        if s43 or s22 > 1:
            ws = torch.empty((s43 or s22, B, K // 8, H, W, 8), device=xb.device, dtype=torch.float32)
            _lib.call("dhz_winograd43_conv3x3_slices" if s43 else f"dhz_winograd_conv3x3{sfx}_slices", _p(xb), _p(uf), _p(self.convs[i].bias), 1,
                      None, None, _p(yb), _p(ws), s43 or s22, B, H, W, C, K, _stream())
        else:
            _lib.call("dhz_winograd43_conv3x3" if f43 else "dhz_winograd_conv3x3" + sfx, _p(xb), _p(uf), _p(self.convs[i].bias), 1, None, None,
                      _p(yb), B, H, W, C, K, _stream())
        _timing_end(ev, B, H, W, C, K, f43 or bool(s43))
        return pool_fwd(yb) if pool else yb

    def conv_dgrad(self, i, gb, below_act=None, addend=None):
        """gb: gradient w.r.t. the pre-activation of conv i.  Returns the gradient w.r.t. conv i's input; with
        `below_act` (the saved post-ReLU map that IS that input) the tap gradient `addend` is added and the ReLU below
        applied in the kernel's store, i.e. the result is the gradient w.r.t. the pre-activation of conv i-1."""
        B, KG, H, W, _ = gb.shape
        C, K = self.conv_shapes[i]
        f43 = use_f43(B, H, W, K, C)                       # the backward-data form: K input channels, C outputs
        s43 = 0 if f43 else use_f43_slices(B, H, W, K, C)
        sfx = "" if _fixed_tiling(H, W) else "_any"
        s22 = getattr(_lib.load(), "dhz_winograd_slices" + sfx)(B, H, W, K, C) if (SLICES_ON and not f43 and not s43) else 1
        _, ub = self.packed43(i, gb.device) if (f43 or s43) else self.packed(i, gb.device)
        dxb = torch.empty((B, C // 8, H, W, 8), device=gb.device, dtype=torch.float32)
        mask = _p(below_act) if below_act is not None else None
        add = addend.contiguous() if addend is not None else None
        ev = ops._timed("dhz_winograd_conv3x3")
        if s43 or s22 > 1:
            ws = torch.empty((s43 or s22, B, C // 8, H, W, 8), device=gb.device, dtype=torch.float32)
            _lib.call("dhz_winograd43_conv3x3_slices" if s43 else f"dhz_winograd_conv3x3{sfx}_slices", _p(gb), _p(ub), None, 0, mask,
                      _p(add) if add is not None else None, _p(dxb), _p(ws), s43 or s22, B, H, W, K, C, _stream())
        else:
            _lib.call("dhz_winograd43_conv3x3" if f43 else "dhz_winograd_conv3x3" + sfx, _p(gb), _p(ub), None, 0, mask,
                      _p(add) if add is not None else None, _p(dxb), B, H, W, K, C, _stream())
        _timing_end(ev, B, H, W, K, C, f43 or bool(s43))
        return dxb

    # ---- full stack, forward only
    def forward_taps(self, x, save=None):
        """x: [B,3,H,W] NCHW.  Returns the tap features, blocked [B,C/8,H,W,8].  `save` (dict) receives what the backward needs."""
        c0 = self.convs[0]
        # first layer (3 -> 64): thin on the input side - convolution + bias + ReLU straight into the blocked layout
        xc = x.contiguous()
        cur = torch.empty((xc.shape[0], 8, xc.shape[2], xc.shape[3], 8), device=x.device, dtype=torch.float32)
        _lib.call("dhz_conv3x3_in3_blocked", _p(xc), _p(c0.weight.contiguous()), _p(c0.bias), _p(cur), xc.shape[0], xc.shape[2],
                  xc.shape[3], 64, 1, _stream())
        acts = {0: cur}
        taps = [cur] if 0 in self.taps else []
        for i in range(1, len(self.convs)):
            # F(4x4,3x3) carries ~3 x the rounding error of F(2x2,3x3) (1.1 - 2.1e-6 rms on O(1) features against 3.7 - 6.7e-7): harmless for
            # feature VALUES and backward-data products; for the differentiated pass see F43_DIFF above (measured, on by default)
            if POOL_FUSED and save is None and i in self.pool_after and i not in self.taps:
                cur = self.conv(i, cur, pool=True)          # no-gradient pass, the un-pooled map has no other reader (a tap has one: the loss)
                continue
            cur = self.conv(i, cur, allow43=(save is None or F43_DIFF))
            acts[i] = cur
            if i in self.taps:
                taps.append(cur)
            if i in self.pool_after:
                cur = pool_fwd(cur)
        if save is not None:
            save.update(x=x, acts=acts)
        return taps

    def backward_taps(self, saved, grads, last_masked=False):
        """gradient w.r.t. the image from the gradients of the taps (None where a tap received none).  last_masked: the last tap's gradient
        has passed that map's ReLU already (dhz_mse_pair_bwd with relu_mask)."""
        acts = saved["acts"]
        last = len(self.convs) - 1
        tap_grad = dict(zip(self.taps[:-1], grads[:-1]))
        g_last = grads[-1]
        c0 = self.convs[0]
        # G = gradient w.r.t. the PRE-activation of conv i (None while nothing has arrived from above)
        G = None
        if g_last is not None:
            G = g_last if last_masked else g_last * (acts[last] > 0)
        for i in range(last, 0, -1):
            below = i - 1                                                # conv i's input is a_{i-1} (pooled if i-1 in pool_after)
            tg = tap_grad.get(below)
            if G is None:
                if tg is not None:                                       # the first gradient enters at this tap
                    G = tg * (acts[below] > 0)
                continue
            if below in self.pool_after:
                if tg is not None:                                       # a tap that is pooled too: its gradient joins on the un-pooled map
                    G = pool_bwd_relu_add(self.conv_dgrad(i, G), acts[below], tg)
                else:
                    G = pool_bwd_relu(self.conv_dgrad(i, G), acts[below])
            else:
                G = self.conv_dgrad(i, G, below_act=acts[below], addend=tg)
        if G is None:
            return None
        # first layer (3 -> 64): its backward-data is a thin 64 -> 3 convolution - straight from the blocked gradient
        x0 = saved["x"]
        gx = torch.empty_like(x0, memory_format=torch.contiguous_format)
        _lib.call("dhz_thin_conv3x3_dgrad_blocked", _p(G.contiguous()), _p(c0.weight.contiguous()), _p(gx), x0.shape[0],
                  x0.shape[2], x0.shape[3], 64, _stream())
        return gx


class _VggTaps(Function):
    """taps(x) with gradient w.r.t. x only (frozen weights)."""

    @staticmethod
    def forward(ctx, engine, x):
        saved = {}
        with torch.no_grad():
            taps = engine.forward_taps(x, save=saved)
        ctx.engine, ctx.saved = engine, saved
        return tuple(taps)

    @staticmethod
    def backward(ctx, *grads):
        with torch.no_grad():
            gx = ctx.engine.backward_taps(ctx.saved, grads)
        ctx.saved = None
        return None, gx


# ------------------------------------------------------------------------------------------------ bf16 feature maps
class VggEngineBF16:
    """The same stack for BASELINE config 4: feature maps in bf16, NHWC ([N, H, W, C]), every 64+-channel convolution an implicit
    GEMM on the bf16 matrix pipe (csrc/vgg_bf16.hip), conv 0 on the input-projection kernel (3 -> 64, bias + ReLU, bf16 tokens out)
    and its backward-data on the output-projection kernel (64 -> 3 from bf16 tokens) with the rotated filter.  The tap features
    leave in NHWC - the L1 means do not care about element order as long as a / p / n agree."""

    dtype = torch.bfloat16

    def __init__(self, convs):
        self.convs = convs
        self._packed = {}

    def packed(self, i, device):
        wt = self.convs[i].weight
        key = (i, str(device), wt.data_ptr(), wt._version)
        hit = self._packed.get(i)
        if hit is None or hit[0] != key:
            w = wt.detach().float().contiguous()
            K, C = w.shape[0], w.shape[1]
            if i == 0:
                # backward-data of conv 0 as a thin 64 -> 3 convolution: filter [3][64][3][3], taps rotated
                hit = (key, w, w.flip(2, 3).transpose(0, 1).contiguous())
            else:
                wf = torch.empty(K * 9 * C, device=device, dtype=torch.bfloat16)
                wb = torch.empty(K * 9 * C, device=device, dtype=torch.bfloat16)
                _lib.call("dhz_vgg_prepack_bf16", _p(w), _p(wf), K, C, 0, _stream())
                _lib.call("dhz_vgg_prepack_bf16", _p(w), _p(wb), K, C, 1, _stream())
                hit = (key, wf, wb)
            self._packed[i] = hit
        return hit[1], hit[2]

    def conv(self, i, x):
        N, H, W, C = x.shape
        K = CONVS[i][1]
        wf, _ = self.packed(i, x.device)
        y = torch.empty((N, H, W, K), device=x.device, dtype=torch.bfloat16)
        ev = ops._timed("dhz_vgg_conv3x3_bf16")
        _lib.call("dhz_vgg_conv3x3_bf16", _p(x), _p(wf), _p(self.convs[i].bias), 1, None, None, _p(y), N, H, W, C, K, _stream())
        _timing_end(ev, N, H, W, C, K)
        return y

    def conv_dgrad(self, i, g, below_act=None, addend=None):
        """as VggEngine.conv_dgrad, on NHWC bf16 maps"""
        g = g.contiguous()                     # (a tap gradient may arrive as a permuted view of an NCHW tensor)
        N, H, W, K = g.shape
        C = CONVS[i][0]
        _, wb = self.packed(i, g.device)
        dx = torch.empty((N, H, W, C), device=g.device, dtype=torch.bfloat16)
        ev = ops._timed("dhz_vgg_conv3x3_bf16")
        _lib.call("dhz_vgg_conv3x3_bf16", _p(g), _p(wb), None, 0, _p(below_act) if below_act is not None else None,
                  _p(addend.contiguous()) if addend is not None else None, _p(dx), N, H, W, K, C, _stream())
        _timing_end(ev, N, H, W, K, C)
        return dx

    @staticmethod
    def pool_fwd(x):
        N, H, W, C = x.shape
        y = torch.empty((N, H // 2, W // 2, C), device=x.device, dtype=torch.bfloat16)
        _lib.call("dhz_maxpool2x2_nhwc_bf16_fwd", _p(x), _p(y), N, H, W, C, _stream())
        return y

    @staticmethod
    def pool_bwd_relu(g, act):
        N, H, W, C = act.shape
        gx = torch.empty_like(act)
        _lib.call("dhz_maxpool2x2_nhwc_bf16_bwd", _p(g.contiguous()), _p(act), _p(gx), N, H, W, C, _stream())
        return gx

    def forward_taps(self, x, save=None):
        """x: [N,3,H,W] NCHW fp32.  Returns the 5 tap features [N,H,W,C] bf16."""
        c0 = self.convs[0]
        xc = x.contiguous().float()
        N, _, H, W = xc.shape
        w0, _ = self.packed(0, x.device)
        cur = torch.empty((N, H, W, 64), device=x.device, dtype=torch.bfloat16)
        # LeakyReLU with slope 0 = the ReLU behind conv 0
        _lib.call("dhz_input_proj_fwd_dt", _p(xc), _p(w0), _p(c0.bias), _p(cur), N, H, W, 64, 0.0, 1, _stream())
        acts = {0: cur}
        taps = [cur]
        for i in range(1, 13):
            cur = self.conv(i, cur)
            acts[i] = cur
            if i in TAPS:
                taps.append(cur)
            if i in POOL_AFTER:
                cur = self.pool_fwd(cur)
        if save is not None:
            save.update(x=xc, acts=acts)
        return taps

    def backward_taps(self, saved, grads):
        """gradient w.r.t. the image from the gradients of the five taps (None where a tap received none)"""
        acts = saved["acts"]
        g1, g2, g3, g4, g5 = grads
        tap_grad = {0: g1, 2: g2, 4: g3, 8: g4}
        G = g5 * (acts[12] > 0) if g5 is not None else None
        for i in range(12, 0, -1):
            below = i - 1
            tg = tap_grad.get(below)
            if G is None:
                if tg is not None:
                    G = tg * (acts[below] > 0)
                continue
            if below in POOL_AFTER:
                G = self.pool_bwd_relu(self.conv_dgrad(i, G), acts[below])
            else:
                G = self.conv_dgrad(i, G, below_act=acts[below], addend=tg)
        if G is None:
            return None
        x0 = saved["x"]
        N, _, H, W = x0.shape
        _, w0r = self.packed(0, x0.device)
        gx = torch.empty_like(x0)
        _lib.call("dhz_thin_conv3x3_fwd_dt", _p(G.contiguous()), _p(w0r), None, _p(gx), N, H, W, 64, 1, _stream())
        return gx


class _VggTapsBF16(Function):
    @staticmethod
    def forward(ctx, engine, x):
        saved = {}
        with torch.no_grad():
            taps = engine.forward_taps(x, save=saved)
        ctx.engine, ctx.saved, ctx.xdtype = engine, saved, x.dtype
        return tuple(taps)

    @staticmethod
    def backward(ctx, *grads):
        with torch.no_grad():
            gx = ctx.engine.backward_taps(ctx.saved, grads)
        ctx.saved = None
        return None, (gx.to(ctx.xdtype) if gx is not None else None)


def vgg_taps(engine, x):
    if torch.is_grad_enabled() and x.requires_grad:
        return list((_VggTapsBF16 if isinstance(engine, VggEngineBF16) else _VggTaps).apply(engine, x))
    with torch.no_grad():
        return engine.forward_taps(x)


class _ToPlain(Function):
    @staticmethod
    def forward(ctx, xb):
        return to_plain(xb)

    @staticmethod
    def backward(ctx, g):
        return to_blocked(g)


def to_plain_tap(t):
    """tap feature -> NCHW (differentiable)"""
    return _ToPlain.apply(t)


def _sfx(t):
    """entry-point suffix for the storage type of a feature map (the fp32 and the bf16 L1 kernels)"""
    if t.dtype == torch.bfloat16:
        return "_bf16"
    return ""


def _l1_sfx(t):
    """_sfx for l1_pair: an fp32 tensor whose element count is no multiple of 4 (the image-space L1 of FFA-Net's recipe on whole images, e.g.
    3 x 413 x 550) takes dhz_l1_pair_*_any; every other tensor the entry it always took"""
    if t.dtype != torch.bfloat16 and t.numel() % 4:
        return "_any"
    return _sfx(t)


class _L1Pair(Function):
    """(mean|a - p|, mean|a - n|) of one feature tap in one pass; gradient w.r.t. a only (p, n carry none, My_CR.py:102)."""

    @staticmethod
    def forward(ctx, a, p, n):
        a, p = a.contiguous(), p.contiguous()
        n = n.contiguous() if n is not None else None
        sums = torch.zeros(2, device=a.device, dtype=torch.float32)
        if a.dtype == torch.bfloat16:
            ops._refuse_bf16_deterministic("contrast sums")
        _lib.call("dhz_l1_pair_fwd" + _l1_sfx(a), _p(a), _p(p), _p(n) if n is not None else None, _p(sums), a.numel(), _stream())
        ctx.save_for_backward(a, p, n) if n is not None else ctx.save_for_backward(a, p)
        ctx.has_n = n is not None
        return sums / a.numel()

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        a, p = saved[0], saved[1]
        n = saved[2] if ctx.has_n else None
        da = torch.empty_like(a)
        _lib.call("dhz_l1_pair_bwd" + _l1_sfx(a), _p(a), _p(p), _p(n) if n is not None else None, _p(g.contiguous()), _p(da),
                  a.numel(), _stream())
        return da, None, None


def l1_pair(a, p, n=None):
    return _L1Pair.apply(a, p, n)


_TAP_CONST = {}


class _ContrastTaps(Function):
    """The scalar side of ContrastLoss.forward (My_CR.py:104-123) for ALL taps as one autograd node:
        loss = sum_i w_i * ap_i / (an_i + 1e-7)   (ablation: sum_i w_i * ap_i),  all_ap = sum_i ap_i,  all_an = sum_i an_i
    with ap_i / an_i the L1 means of tap i (dhz_l1_pair_fwd, one pass over a, p, n per tap).  As separate autograd scalars the
    five taps cost ~100 launches of 4-8 us per step (0-dim add / div / mul / neg, select_backward, zero fills); here the
    combination and the ten backward coefficients are one small kernel each way (dhz_contrast_combine_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, weights, ablation, B, *feats):
        k = len(feats) // 2
        a = [f.contiguous() for f in feats[:k]]
        dev = a[0].device
        key = (str(dev), tuple(f.numel() for f in a), tuple(weights))
        if key not in _TAP_CONST:
            _TAP_CONST[key] = (torch.tensor([1.0 / f.numel() for f in a], dtype=torch.float32).view(k, 1).to(dev),
                               torch.tensor(list(weights), dtype=torch.float32).to(dev))
        inv_cnt, w = _TAP_CONST[key]
        sums = ops.zeros_f32((k, 2), dev)          # (accumulation target of this pass: the optimizer's zeroed scratch when there is one)
        ps, ns = [], []
        for i in range(k):
            p = feats[k + i][:B].contiguous()
            n = None if ablation else feats[k + i][B:].contiguous()
            if a[i].dtype == torch.bfloat16:
                ops._refuse_bf16_deterministic("contrast sums")
            _lib.call("dhz_l1_pair_fwd" + _sfx(a[i]), _p(a[i]), _p(p), _p(n) if n is not None else None, sums.data_ptr() + 8 * i,
                      a[i].numel(), _stream())
            ps.append(p)
            ns.append(n)
        d = torch.empty((k, 2), device=dev, dtype=torch.float32)       # [k, 2] means
        out = torch.empty(3, device=dev, dtype=torch.float32)
        _lib.call("dhz_contrast_combine_fwd", _p(sums), _p(inv_cnt), _p(w), k, int(ablation), _p(d), _p(out), _stream())
        ctx.set_materialize_grads(False)
        ctx.k, ctx.ablation = k, ablation
        ctx.save_for_backward(d, w, *a, *ps, *([] if ablation else ns))
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_loss, g_ap, g_an):
        k, ablation = ctx.k, ctx.ablation
        saved = ctx.saved_tensors
        d, w = saved[0], saved[1]
        a, ps = saved[2:2 + k], saved[2 + k:2 + 2 * k]
        ns = [None] * k if ablation else saved[2 + 2 * k:2 + 3 * k]
        g = torch.empty((k, 2), device=d.device, dtype=torch.float32)          # d loss / d (ap_i, an_i)
        # converted copies stay referenced until the launch is enqueued (a temporary's pointer would dangle when the incoming
        # gradient is not already a contiguous fp32 scalar)
        gl, gp, gn = (None if t is None else t.to(torch.float32).contiguous() for t in (g_loss, g_ap, g_an))
        _lib.call("dhz_contrast_combine_bwd", _p(d), _p(w), k, int(ablation), None if gl is None else _p(gl),
                  None if gp is None else _p(gp), None if gn is None else _p(gn), _p(g), _stream())
        del gl, gp, gn
        das = []
        for i in range(k):
            da = torch.empty_like(a[i])
            _lib.call("dhz_l1_pair_bwd" + _sfx(a[i]), _p(a[i]), _p(ps[i]), _p(ns[i]) if ns[i] is not None else None, g.data_ptr() + 8 * i,
                      _p(da), a[i].numel(), _stream())
            das.append(da)
        return (None, None, None) + tuple(das) + (None,) * k


def contrast_taps(a_taps, pn_taps, B, weights, ablation):
    """(loss, all_ap, all_an) of ContrastLoss from the feature taps of a (grad) and of cat([p, n]) / p (no grad)."""
    return _ContrastTaps.apply(tuple(weights), bool(ablation), int(B), *a_taps, *pn_taps)
