"""UNet baseline exported by the reference next to Uformer (M1:22-140, get_arch 'UNet').  Module tree, parameter names, registration
order and init stream are the reference's; CPU tensors run the plain-torch path.  On a HIP device the layers run the hand-written
kernels, with the token layout [B, H*W, C] as the interchange between layers:

  ConvBlock1.block[0] (3 -> dim, + LeakyReLU)   ops.input_proj                      (csrc/input_proj.hip)
  every other 3x3 (+ LeakyReLU, + conv11(x))    _Conv3x3Leaky: Winograd forward / backward-data + dhz_conv3x3_wgrad
  conv11                                        ops.linear_tokens                   (3 input channels padded to 16)
  pool1..4                                      ops.conv4s2_tokens                  (csrc/conv_gemm.hip)
  upv6..9 + skip concatenation                  ops.linear_tokens + model._ShuffleConcat (strided stores into the concatenated buffer)
  conv10 (dim -> 3)                             ops.thin_conv3x3                    (32 channels padded to 64)

A layer whose shape the kernels do not tile (dim 16, maps below 8 x 8, more than 512 channels, non-fp32 input) runs the library
convolution through ops.warn_library_fallback, layer by layer."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

SLOPE = 0.01


def _lib():
    from . import _lib as L
    return L


def conv3x3_supported(B, C, K, s):
    """shape contract shared by dhz_winograd_conv3x3(_act) (forward and backward-data, the channel roles swap) and dhz_conv3x3_wgrad"""
    return C % 32 == 0 and K % 32 == 0 and 32 <= C <= 512 and 32 <= K <= 512 and (s == 8 or (s >= 16 and s % 16 == 0))


class _Conv3x3Leaky(Function):
    """y = leaky(conv3x3(x, w) + b) [+ res] on tokens.  The maps cross into the channel-blocked layout of the Winograd kernels once per
    direction; `+ res` (the block's conv11 branch, M1:40) is folded into the copy back to tokens, the LeakyReLU derivative (sign of the
    saved activation) into the copy of the gradient towards the blocked layout: no elementwise pass of its own in either direction."""

    @staticmethod
    def forward(ctx, x, w, b, res, s):
        from . import ops
        L = _lib()
        B, HW, C = x.shape
        K = w.shape[0]
        st = ops._stream()
        x = x.contiguous()
        xb = torch.empty((B, C // 8, s, s, 8), device=x.device, dtype=torch.float32)
        L.call("dhz_tokens_to_blocked8", ops._p(x), C, None, ops._p(xb), B, HW, C, st)
        up = torch.empty(16 * K * C, device=x.device, dtype=torch.float32)
        wc = w.contiguous()
        L.call("dhz_winograd_prepack", ops._p(wc), ops._p(up), K, C, 0, st)
        act = torch.empty((B, K // 8, s, s, 8), device=x.device, dtype=torch.float32)
        L.call("dhz_winograd_conv3x3_act", ops._p(xb), ops._p(up), ops._p(b), 0, None, None, ops._p(act), B, s, s, C, K, st)
        y = torch.empty((B, HW, K), device=x.device, dtype=torch.float32)
        if res is not None:
            res = res.contiguous()
        L.call("dhz_blocked8_to_tokens", ops._p(act), ops._p(res), K, ops._p(y), K, B, HW, K, st)
        ctx.save_for_backward(xb, act, wc)
        ctx.dims = (B, HW, C, K, s, res is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        from . import ops
        L = _lib()
        xb, act, w = ctx.saved_tensors
        B, HW, C, K, s, has_res = ctx.dims
        st = ops._stream()
        g = g.contiguous()
        d = torch.empty_like(act)                                   # gradient at the pre-activation, blocked
        L.call("dhz_tokens_to_blocked8", ops._p(g), K, ops._p(act), ops._p(d), B, HW, K, st)
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw = torch.empty_like(w)
            db = torch.empty(K, device=g.device, dtype=torch.float32)
            need = L.load().dhz_conv3x3_wgrad_workspace_bytes(B, s, s, C, K)
            ws = None if ops.DETERMINISTIC else torch.empty(need // 4, device=g.device, dtype=torch.float32)
            L.call("dhz_conv3x3_wgrad", ops._p(xb), ops._p(d), ops._p(dw), ops._p(db), ops._p(ws), need, B, s, s, C, K, st)
        if ctx.needs_input_grad[0]:
            upt = torch.empty(16 * K * C, device=g.device, dtype=torch.float32)
            L.call("dhz_winograd_prepack", ops._p(w), ops._p(upt), C, K, 1, st)      # backward-data filters: Kout = C, Cin = K
            dxb = torch.empty_like(xb)
            L.call("dhz_winograd_conv3x3", ops._p(d), ops._p(upt), None, 0, None, None, ops._p(dxb), B, s, s, K, C, st)
            dx = torch.empty((B, HW, C), device=g.device, dtype=torch.float32)
            L.call("dhz_blocked8_to_tokens", ops._p(dxb), None, 0, ops._p(dx), C, B, HW, C, st)
        return dx, dw, db, (g if has_res else None), None


def _tokens_to_map(x, s):
    B, L, C = x.shape
    return x.contiguous().view(B, s, s, C).permute(0, 3, 1, 2)


def _map_to_tokens(y):
    B, C, H, W = y.shape
    return y.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _conv3x3_leaky_tokens(conv, x, res, s):
    """tokens -> leaky(conv(x)) [+ res] -> tokens, on the kernels where they tile the shape"""
    from . import ops
    B, HW, C = x.shape
    K = conv.out_channels
    if x.dtype == torch.float32 and conv3x3_supported(B, C, K, s):
        return _Conv3x3Leaky.apply(x, conv.weight, conv.bias, res, s)
    ops.warn_library_fallback("UNet Conv3x3", (C, K, s))
    y = _map_to_tokens(F.leaky_relu(conv(_tokens_to_map(x, s)), SLOPE))
    return y if res is None else y + res


def _conv11_tokens(conv, x):
    """1x1 convolution as a token-Linear; 3 input channels (ConvBlock1) are padded to 16 zero channels"""
    from . import ops
    B, HW, C = x.shape
    K = conv.out_channels
    w = conv.weight.view(K, C)
    if x.dtype != torch.float32 or K % 16 != 0 or (C % 16 != 0 and C != 3) or (B * HW) % 16 != 0:
        ops.warn_library_fallback("UNet conv11", (C, K, HW))
        return F.linear(x, w, conv.bias)
    if C == 3:
        x, w = F.pad(x, (0, 13)), F.pad(w, (0, 13))
    return ops.linear_tokens(x.reshape(B * HW, -1), w, conv.bias).view(B, HW, K)


class ConvBlock(nn.Module):
    def __init__(self, in_channel, out_channel, strides=1):
        super().__init__()
        self.strides, self.in_channel, self.out_channel = strides, in_channel, out_channel
        self.block = nn.Sequential(
            nn.Conv2d(in_channel, out_channel, kernel_size=3, stride=strides, padding=1), nn.LeakyReLU(inplace=True),
            nn.Conv2d(out_channel, out_channel, kernel_size=3, stride=strides, padding=1), nn.LeakyReLU(inplace=True))
        self.conv11 = nn.Conv2d(in_channel, out_channel, kernel_size=1, stride=strides, padding=0)

    def forward(self, x):
        return self.block(x) + self.conv11(x)

    def forward_tokens(self, x, s, img=None):
        """device path: x tokens [B, s*s, Cin] (img: the NCHW image behind them, for the 3-channel first block)"""
        from . import ops
        c1, c2 = self.block[0], self.block[2]
        r = _conv11_tokens(self.conv11, x)
        if img is not None and self.in_channel == 3 and self.out_channel in (16, 32, 64) and img.dtype == torch.float32 and not img.requires_grad:
            a = ops.input_proj(img.contiguous(), c1.weight, c1.bias, SLOPE)
        elif img is not None:
            ops.warn_library_fallback("UNet Conv3x3 (image)", (self.in_channel, self.out_channel, s))
            a = _map_to_tokens(F.leaky_relu(c1(img), SLOPE))
        else:
            a = _conv3x3_leaky_tokens(c1, x, None, s)
        return _conv3x3_leaky_tokens(c2, a, r, s)


def _pool_tokens(conv, x, s):
    from . import ops
    need_grad = torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad)
    if ops.conv4s2_supported(x, s, s, need_grad) and conv.out_channels % 32 == 0:
        return ops.conv4s2_tokens(x, conv.weight, conv.bias, s, s)
    ops.warn_library_fallback("UNet pool", (conv.in_channels, conv.out_channels, s))
    return _map_to_tokens(conv(_tokens_to_map(x, s)))


def _up_concat_tokens(dc, x, skip, s):
    """ConvTranspose2d(k2, s2) as a token-Linear Cin -> 4 Cout + pixel shuffle, stored straight into cat([up, skip], channels)"""
    from . import ops
    from .model import _ShuffleConcat
    B, L, Cin = x.shape
    Co = dc.out_channels
    if x.dtype != torch.float32 or Cin % 16 != 0 or Co % 4 != 0 or (B * L) % 16 != 0:
        ops.warn_library_fallback("UNet upv", (Cin, Co, s))
        return torch.cat([_map_to_tokens(dc(_tokens_to_map(x, s))), skip], -1)
    w4 = dc.weight.permute(2, 3, 1, 0).reshape(4 * Co, Cin)
    y = ops.linear_tokens(x.reshape(B * L, Cin), w4, dc.bias.repeat(4))
    return _ShuffleConcat.apply(y, skip.contiguous(), B, s, Co)


class UNet(nn.Module):
    def __init__(self, block=ConvBlock, dim=32):
        super().__init__()
        self.dim = dim
        chans = [dim, dim * 2, dim * 4, dim * 8, dim * 16]
        self.ConvBlock1 = ConvBlock(3, dim, strides=1)
        self.pool1 = nn.Conv2d(dim, dim, kernel_size=4, stride=2, padding=1)
        for i in range(1, 4):
            setattr(self, f"ConvBlock{i + 1}", block(chans[i - 1], chans[i], strides=1))
            setattr(self, f"pool{i + 1}", nn.Conv2d(chans[i], chans[i], kernel_size=4, stride=2, padding=1))
        self.ConvBlock5 = block(chans[3], chans[4], strides=1)
        for j, i in enumerate(range(6, 10)):
            cin = chans[4 - j]
            setattr(self, f"upv{i}", nn.ConvTranspose2d(cin, cin // 2, 2, stride=2))
            setattr(self, f"ConvBlock{i}", block(cin, cin // 2, strides=1))
        self.conv10 = nn.Conv2d(dim, 3, kernel_size=3, stride=1, padding=1)

    def _forward_torch(self, x):
        skips, y = [], x
        for i in range(1, 5):
            y = getattr(self, f"ConvBlock{i}")(y)
            skips.append(y)
            y = getattr(self, f"pool{i}")(y)
        y = self.ConvBlock5(y)
        for j, i in enumerate(range(6, 10)):
            y = torch.cat([getattr(self, f"upv{i}")(y), skips[3 - j]], 1)
            y = getattr(self, f"ConvBlock{i}")(y)
        return x + self.conv10(y)

    def forward(self, x):
        B, C, H, W = x.shape
        blocks_ok = all(hasattr(getattr(self, f"ConvBlock{i}"), "forward_tokens") for i in range(1, 10))
        if not x.is_cuda:
            return self._forward_torch(x)
        if x.dtype != torch.float32 or H != W or H % 16 != 0 or not blocks_ok:
            from . import ops
            ops.warn_library_fallback("UNet", (C, H, W, str(x.dtype)))
            return self._forward_torch(x)
        return self._forward_tokens(x)

    def _forward_tokens(self, x):
        from . import ops
        B, _, s, _ = x.shape
        skips = []
        y = self.ConvBlock1.forward_tokens(_map_to_tokens(x), s, img=x)
        for i in range(1, 5):
            if i > 1:
                y = getattr(self, f"ConvBlock{i}").forward_tokens(y, s)
            skips.append(y)
            y = _pool_tokens(getattr(self, f"pool{i}"), y, s)
            s //= 2
        y = self.ConvBlock5.forward_tokens(y, s)
        for j, i in enumerate(range(6, 10)):
            y = _up_concat_tokens(getattr(self, f"upv{i}"), y, skips[3 - j], s)
            s *= 2
            y = getattr(self, f"ConvBlock{i}").forward_tokens(y, s)
        c10 = self.conv10
        C = y.shape[-1]
        if C in (64, 128):
            out = ops.thin_conv3x3(y, c10.weight, c10.bias, s, s)
        elif C == 32:                       # the thin-convolution kernels work in 64-channel chunks: 32 zero channels (OutputProj's way)
            out = ops.thin_conv3x3(F.pad(y, (0, 32)), F.pad(c10.weight, (0, 0, 0, 0, 0, 32)), c10.bias, s, s)
        else:
            ops.warn_library_fallback("UNet conv10", (C, 3, s))
            out = c10(_tokens_to_map(y, s))
        return x + out
