"""FFA-Net, the second CNN baseline the reference measures against (FFA_model/models/FFA.py:9-110; get_arch 'FFA').  Module tree,
attribute names, registration order and init stream are the reference's, so seeded construction draws the same parameters and its
checkpoints load; there are no buffers.  CPU tensors run the plain-torch path.  On a HIP device (fp32, a map size blocked_shape_ok takes)
every layer runs the hand-written kernels and the maps stay channel-blocked [B][8][H][W][8] from `pre` to `post[0]`:

  pre[0] 3 -> 64                        dhz_conv3x3_in3_blocked (relu = 0); weight gradient dhz_input_proj_bwd with slope 1
  Block.conv1 + act1                    Winograd convolution with the ReLU in its store; a1 is saved, its sign is the backward's mask
  res = a1 + x                          dhz_ffa_add
  Block.conv2, gp[-1], post[0]          Winograd convolution, no activation
  calayer, palayer, `res += x`          dhz_ffa_ca_fwd + dhz_ffa_gate_pa_fwd, G = 1          (csrc/ffa_attn.hip)
  self.ca over the three group outputs, the weighted sum, self.palayer     the same two entries, G = 3: nothing is concatenated
  group residual                        dhz_ffa_add
  post[1] 64 -> 3, + x1                 dhz_blocked8_to_tokens, ops.thin_conv3x3, dhz_ffa_add (dhz_ffa_add_any where 3 B H W % 4 != 0)
  every 3x3 weight gradient             dhz_conv3x3_wgrad

A block keeps x, a1, c2 (conv2's output) and the small vectors mean, hid, ca for its backward; res = a1 + x is formed again there (the
same bits) rather than stored, and the gated map, the pixel gate and the block output are recomputed by the backward kernels.

Whole images (FFA_model/test.py:49-61, data_utils.py:21-23: `size='whole img'`, 620 x 460 on SOTS-indoor) have sides that are no
multiples of 16.  On such a ragged map the same layers call the `_any` entries: dhz_winograd_conv3x3_any (ragged 16 x 16 blocks),
dhz_conv3x3_wgrad_any (ragged 4 x 16 chunks), dhz_ffa_*_any (bounded tails); the other entries in the table take any H, W as they
are.  dhz_winograd_conv3x3_any is F(2x2) only - the F(4x4) kernel has no ragged mode - so FWD_F43 / BWD_F43 are ignored on ragged
maps.  On a multiple-of-16 map every helper calls exactly what it called before those entries existed.  DHZ_FFA_ANY=0 (A/B switch)
keeps ragged maps on the library path.
Any other input (another dtype, a ragged map with a side below 32) runs the library convolutions through ops.warn_library_fallback."""
import os

import torch
import torch.nn as nn
from torch.autograd import Function

DIM = 64
# Winograd variant per direction: F(2x2,3x3) (dhz_winograd_conv3x3) or F(4x4,3x3) (dhz_winograd43_conv3x3, ~2x the rounding error)
FWD_F43 = False
BWD_F43 = False
ANY = os.environ.get("DHZ_FFA_ANY", "1") != "0"      # A/B switch: ragged maps on the `_any` entries (off: on the library path, with the warning)
ANY_MIN = 32


def blocked_shape_ok(H, W):
    """map sizes the blocked path takes: both sides multiples of 16 (from 16 up), as ever; or, with ANY, any other H x W with both sides
    at least ANY_MIN = 32.  The floor is deliberate: 32 is LossNetwork's smallest patch too, no dehazing set has smaller images, and
    ragged maps below it (24 x 40 ...) keep the library path they have always had."""
    if H % 16 == 0 and W % 16 == 0:
        return H >= 16 and W >= 16
    return ANY and H >= ANY_MIN and W >= ANY_MIN


def _ragged(H, W):
    """a map only the `_any` entries take"""
    return H % 16 != 0 or W % 16 != 0


def _lib():
    from . import _lib as L
    return L


def _conv64(xb, w, transposed, bias, relu, addend, f43):
    """y = conv3x3(xb, w) [+ bias] [ReLU]   or, with transposed, the backward-data product conv(xb, w') [+ addend]; blocked maps"""
    from . import ops
    L = _lib()
    B, _, H, W, _ = xb.shape
    st = ops._stream()
    ragged = _ragged(H, W)
    f43 = f43 and not ragged                                         # the F(4x4) kernel has no ragged mode
    up = torch.empty((36 if f43 else 16) * DIM * DIM, device=xb.device, dtype=torch.float32)
    L.call("dhz_winograd43_prepack" if f43 else "dhz_winograd_prepack", ops._p(w), ops._p(up), DIM, DIM, int(transposed), st)
    y = torch.empty_like(xb)
    entry = "dhz_winograd_conv3x3_any" if ragged else ("dhz_winograd43_conv3x3" if f43 else "dhz_winograd_conv3x3")
    L.call(entry, ops._p(xb), ops._p(up), ops._p(bias), int(relu), None, ops._p(addend), ops._p(y), B, H, W, DIM, DIM, st)
    return y


def _wgrad64(xb, dyb, w):
    from . import ops
    L = _lib()
    B, _, H, W, _ = xb.shape
    dw = torch.empty_like(w)
    db = torch.empty(DIM, device=xb.device, dtype=torch.float32)
    sfx = "_any" if _ragged(H, W) else ""
    need = getattr(L.load(), "dhz_conv3x3_wgrad_workspace_bytes" + sfx)(B, H, W, DIM, DIM)
    ws = None if ops.DETERMINISTIC else torch.empty(need // 4, device=xb.device, dtype=torch.float32)
    L.call("dhz_conv3x3_wgrad" + sfx, ops._p(xb), ops._p(dyb), ops._p(dw), ops._p(db), ops._p(ws), need, B, H, W, DIM, DIM, ops._stream())
    return dw, db


def _add(a, x):
    from . import ops
    # a batch slice of an image whose 3 H W is no multiple of 4 starts off the 16 bytes the kernels load by: a copy of it does not
    a, x = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (a, x))
    y = torch.empty_like(a)
    # an image's 3 B H W floats need not come in fours (413 x 550); a blocked map's 64 B H W always do
    _lib().call("dhz_ffa_add" if a.numel() % 4 == 0 else "dhz_ffa_add_any", ops._p(a), ops._p(x), ops._p(y), a.numel(), ops._stream())
    return y


def _workspace(B, H, W, G, device):
    from . import ops
    need = getattr(_lib().load(), "dhz_ffa_workspace_bytes" + ("_any" if _ragged(H, W) else ""))(B, H, W, G)
    return (None if ops.DETERMINISTIC else torch.empty(need // 4, device=device, dtype=torch.float32)), need


def _attn_fwd(maps, attn, res):
    """channel attention + pixel attention (+ res) over G = len(maps) maps; returns out and (mean, hid, ca)"""
    from . import ops
    L = _lib()
    Wa, ba, Wb, bb, Wp1, bp1, wp2, bp2 = attn
    G = len(maps)
    B, _, H, W, _ = maps[0].shape
    dev = maps[0].device
    st = ops._stream()
    m = [ops._p(t) for t in maps] + [None] * (3 - G)
    hc = Wa.shape[0]
    mean = torch.empty((B, DIM * G), device=dev, dtype=torch.float32)
    hid = torch.empty((B, hc), device=dev, dtype=torch.float32)
    ca = torch.empty((B, DIM * G), device=dev, dtype=torch.float32)
    ws, need = _workspace(B, H, W, G, dev)
    sfx = "_any" if _ragged(H, W) else ""
    L.call("dhz_ffa_ca_fwd" + sfx, *m, ops._p(Wa), ops._p(ba), ops._p(Wb), ops._p(bb), ops._p(mean), ops._p(hid), ops._p(ca), ops._p(ws), need,
           B, H, W, G, st)
    out = torch.empty_like(maps[0])
    L.call("dhz_ffa_gate_pa_fwd" + sfx, *m, ops._p(ca), ops._p(Wp1), ops._p(bp1), ops._p(wp2), ops._p(bp2), ops._p(res), ops._p(out), B, H, W, G,
           st)
    return out, (mean, hid, ca)


def _attn_bwd(maps, attn, vecs, dout):
    """gradients of the maps and of the eight attention parameters"""
    from . import ops
    L = _lib()
    Wa, ba, Wb, bb, Wp1, bp1, wp2, bp2 = attn
    mean, hid, ca = vecs
    G = len(maps)
    B, _, H, W, _ = maps[0].shape
    dev = maps[0].device
    st = ops._stream()
    m = [ops._p(t) for t in maps] + [None] * (3 - G)
    ws, need = _workspace(B, H, W, G, dev)
    sfx = "_any" if _ragged(H, W) else ""
    dt = torch.empty_like(maps[0])
    L.call("dhz_ffa_gate_pa_bwd_a" + sfx, *m, ops._p(ca), ops._p(Wp1), ops._p(bp1), ops._p(wp2), ops._p(bp2), ops._p(dout), ops._p(dt), ops._p(ws),
           need, B, H, W, G, st)
    grads = [torch.empty_like(p) for p in attn]
    dmean = torch.empty_like(mean)
    dWa, dba, dWb, dbb, dWp1, dbp1, dwp2, dbp2 = grads
    L.call("dhz_ffa_ca_bwd" + sfx, ops._p(ws), need, ops._p(Wa), ops._p(Wb), ops._p(mean), ops._p(hid), ops._p(ca), ops._p(dWa), ops._p(dba),
           ops._p(dWb), ops._p(dbb), ops._p(dmean), ops._p(dWp1), ops._p(dbp1), ops._p(dwp2), ops._p(dbp2), B, H, W, G, st)
    dm = [torch.empty_like(maps[0]) for _ in range(G)]
    L.call("dhz_ffa_gate_pa_bwd_b" + sfx, ops._p(dt), ops._p(ca), ops._p(dmean), *([ops._p(t) for t in dm] + [None] * (3 - G)), B, H, W, G, st)
    return dm, grads


class _BlockFn(Function):
    """FFA.py:50-57 on blocked maps: out = palayer(calayer(conv2(relu(conv1(x)) + x))) + x"""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, *attn):
        a1 = _conv64(x, w1, False, b1, True, None, FWD_F43)
        res = _add(a1, x)
        c2 = _conv64(res, w2, False, b2, False, None, FWD_F43)
        out, vecs = _attn_fwd([c2], attn, x)
        ctx.save_for_backward(x, a1, c2, w1, w2, *vecs, *attn)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import ops
        x, a1, c2, w1, w2, mean, hid, ca = ctx.saved_tensors[:8]
        attn = ctx.saved_tensors[8:]
        dout = dout.contiguous()
        (dc2,), dattn = _attn_bwd([c2], attn, (mean, hid, ca), dout)
        res = _add(a1, x)                                            # the forward's bits again
        dw2, db2 = _wgrad64(res, dc2, w2)
        dr = _conv64(dc2, w2, True, None, False, None, BWD_F43)
        del res, dc2
        dpre1, s = torch.empty_like(dr), torch.empty_like(dr)
        _lib().call("dhz_ffa_relu_bwd_add", ops._p(a1), ops._p(dr), ops._p(dout), ops._p(dpre1), ops._p(s), dr.numel(), ops._stream())
        dw1, db1 = _wgrad64(x, dpre1, w1)
        dx = _conv64(dpre1, w1, True, None, False, s, BWD_F43)       # + s (= dout + dr) in the store
        return (dx, dw1, db1, dw2, db2, *dattn)


class _HeadFn(Function):
    """FFA.py:105-108 on blocked maps: the channel gates of cat(r1, r2, r3), the weighted sum and the pixel attention"""

    @staticmethod
    def forward(ctx, r1, r2, r3, *attn):
        out, vecs = _attn_fwd([r1, r2, r3], attn, None)
        ctx.save_for_backward(r1, r2, r3, *vecs, *attn)
        return out

    @staticmethod
    def backward(ctx, dout):
        r1, r2, r3, mean, hid, ca = ctx.saved_tensors[:6]
        dm, dattn = _attn_bwd([r1, r2, r3], ctx.saved_tensors[6:], (mean, hid, ca), dout.contiguous())
        return (*dm, *dattn)


class _ConvFn(Function):
    """y = conv3x3(x, w) + b [+ addend] on blocked maps (the group's last convolution with its residual, post[0])"""

    @staticmethod
    def forward(ctx, x, w, b, addend):
        y = _conv64(x, w, False, b, False, None, FWD_F43)
        if addend is not None:
            y = _add(y, addend)
        ctx.save_for_backward(x, w)
        ctx.has_addend = addend is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dw, db = _wgrad64(x, dy, w)
        dx = _conv64(dy, w, True, None, False, None, BWD_F43)
        return dx, dw, db, (dy if ctx.has_addend else None)


class _PreFn(Function):
    """pre[0]: Conv2d(3, 64, 3x3, pad 1) from the NCHW image to a blocked map"""

    @staticmethod
    def forward(ctx, img, w, b):
        from . import ops
        B, _, H, W = img.shape
        y = torch.empty((B, DIM // 8, H, W, 8), device=img.device, dtype=torch.float32)
        _lib().call("dhz_conv3x3_in3_blocked", ops._p(img), ops._p(w), ops._p(b), ops._p(y), B, H, W, DIM, 0, ops._stream())
        ctx.save_for_backward(img, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        L = _lib()
        img, w = ctx.saved_tensors
        B, _, H, W = img.shape
        st = ops._stream()
        dy = dy.contiguous()
        tok = torch.empty((B, H * W, DIM), device=dy.device, dtype=torch.float32)
        L.call("dhz_blocked8_to_tokens", ops._p(dy), None, 0, ops._p(tok), DIM, B, H * W, DIM, st)
        dw = torch.zeros_like(w)
        db = torch.zeros(DIM, device=dy.device, dtype=torch.float32)
        # slope 1: the activation mask (second argument) decides nothing
        L.call("dhz_input_proj_bwd", ops._p(tok), ops._p(tok), ops._p(img), ops._p(dw), ops._p(db), B, H, W, DIM, 1.0, st)
        dimg = None
        if ctx.needs_input_grad[0]:
            dimg = torch.empty_like(img)
            L.call("dhz_thin_conv3x3_dgrad_blocked", ops._p(dy), ops._p(w), ops._p(dimg), B, H, W, DIM, st)
        return dimg, dw, db


class _ToTokensFn(Function):
    @staticmethod
    def forward(ctx, xb):
        from . import ops
        B, _, H, W, _ = xb.shape
        tok = torch.empty((B, H * W, DIM), device=xb.device, dtype=torch.float32)
        _lib().call("dhz_blocked8_to_tokens", ops._p(xb), None, 0, ops._p(tok), DIM, B, H * W, DIM, ops._stream())
        ctx.geom = (B, H, W)
        return tok

    @staticmethod
    def backward(ctx, g):
        from . import ops
        B, H, W = ctx.geom
        g = g.contiguous()
        blk = torch.empty((B, DIM // 8, H, W, 8), device=g.device, dtype=torch.float32)
        _lib().call("dhz_tokens_to_blocked8", ops._p(g), DIM, None, ops._p(blk), B, H * W, DIM, ops._stream())
        return blk


class _AddFn(Function):
    @staticmethod
    def forward(ctx, a, x):
        return _add(a, x)

    @staticmethod
    def backward(ctx, g):
        return g, g


def default_conv(in_channels, out_channels, kernel_size, bias=True):
    """a stride-1 convolution that keeps the map size (odd kernel_size): the `conv` argument of Block, Group and FFA"""
    same = (kernel_size - 1) // 2
    return nn.Conv2d(in_channels, out_channels, kernel_size, stride=1, padding=same, bias=bias)


class PALayer(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.pa = nn.Sequential(nn.Conv2d(channel, channel // 8, 1, padding=0, bias=True), nn.ReLU(inplace=True),
                                nn.Conv2d(channel // 8, 1, 1, padding=0, bias=True), nn.Sigmoid())

    def forward(self, x):
        return x * self.pa(x)


class CALayer(nn.Module):
    def __init__(self, channel):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.ca = nn.Sequential(nn.Conv2d(channel, channel // 8, 1, padding=0, bias=True), nn.ReLU(inplace=True),
                                nn.Conv2d(channel // 8, channel, 1, padding=0, bias=True), nn.Sigmoid())

    def forward(self, x):
        return x * self.ca(self.avg_pool(x))


def _attn_params(ca_a, ca_b, pa):
    """the eight tensors of a channel gate (its two 1x1 convolutions) and a PALayer, in the kernels' argument order"""
    return (ca_a.weight, ca_a.bias, ca_b.weight, ca_b.bias, pa.pa[0].weight, pa.pa[0].bias, pa.pa[2].weight, pa.pa[2].bias)


class Block(nn.Module):
    def __init__(self, conv, dim, kernel_size):
        super().__init__()
        self.conv1 = conv(dim, dim, kernel_size, bias=True)
        self.act1 = nn.ReLU(inplace=True)
        self.conv2 = conv(dim, dim, kernel_size, bias=True)
        self.calayer = CALayer(dim)
        self.palayer = PALayer(dim)

    def forward(self, x):
        res = self.act1(self.conv1(x)) + x
        res = self.palayer(self.calayer(self.conv2(res)))
        return res + x

    def forward_blocked(self, x):
        return _BlockFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                              *_attn_params(self.calayer.ca[0], self.calayer.ca[2], self.palayer))


class Group(nn.Module):
    def __init__(self, conv, dim, kernel_size, blocks):
        super().__init__()
        self.gp = nn.Sequential(*[Block(conv, dim, kernel_size) for _ in range(blocks)], conv(dim, dim, kernel_size))

    def forward(self, x):
        return self.gp(x) + x

    def forward_blocked(self, x):
        y = x
        for blk in self.gp[:-1]:
            y = blk.forward_blocked(y)
        return _ConvFn.apply(y, self.gp[-1].weight, self.gp[-1].bias, x)


class FFA(nn.Module):
    def __init__(self, gps, blocks, conv=default_conv):
        super().__init__()
        assert gps == 3
        self.gps = gps
        self.dim = DIM
        kernel_size = 3
        pre = conv(3, self.dim, kernel_size)              # drawn first, registered after palayer: the reference's init stream and key order
        self.g1 = Group(conv, self.dim, kernel_size, blocks=blocks)
        self.g2 = Group(conv, self.dim, kernel_size, blocks=blocks)
        self.g3 = Group(conv, self.dim, kernel_size, blocks=blocks)
        self.ca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(self.dim * gps, self.dim // 16, 1, padding=0), nn.ReLU(inplace=True),
                                nn.Conv2d(self.dim // 16, self.dim * gps, 1, padding=0, bias=True), nn.Sigmoid())
        self.palayer = PALayer(self.dim)
        self.pre = nn.Sequential(pre)
        self.post = nn.Sequential(conv(self.dim, self.dim, kernel_size), conv(self.dim, 3, kernel_size))

    def _forward_torch(self, x1):
        x = self.pre(x1)
        r1 = self.g1(x)
        r2 = self.g2(r1)
        r3 = self.g3(r2)
        w = self.ca(torch.cat([r1, r2, r3], dim=1)).view(-1, self.gps, self.dim, 1, 1)
        out = self.palayer(w[:, 0] * r1 + w[:, 1] * r2 + w[:, 2] * r3)
        return self.post(out) + x1

    def forward(self, x1):
        if not x1.is_cuda:
            return self._forward_torch(x1)
        B, C, H, W = x1.shape
        if x1.dtype != torch.float32 or C != 3 or not blocked_shape_ok(H, W):
            from . import ops
            ops.warn_library_fallback("FFA", (C, H, W, str(x1.dtype)))
            return self._forward_torch(x1)
        return self._forward_blocked(x1)

    def _forward_blocked(self, x1):
        from . import ops
        B, _, H, W = x1.shape
        x1 = x1.contiguous()
        x = _PreFn.apply(x1, self.pre[0].weight, self.pre[0].bias)
        r1 = self.g1.forward_blocked(x)
        r2 = self.g2.forward_blocked(r1)
        r3 = self.g3.forward_blocked(r2)
        out = _HeadFn.apply(r1, r2, r3, *_attn_params(self.ca[1], self.ca[3], self.palayer))
        p0 = _ConvFn.apply(out, self.post[0].weight, self.post[0].bias, None)
        y = ops.thin_conv3x3(_ToTokensFn.apply(p0), self.post[1].weight, self.post[1].bias, H, W)
        return _AddFn.apply(y, x1)
