#!/usr/bin/env python3
"""Times dhz_conv3x3_wgrad (csrc/conv3x3_wgrad.hip) on the 3x3 layer shapes of the UNet baseline at dim 32, 128 x 128, batch 32, beside
the library's weight gradient (torch.nn.grad.conv2d_weight) on the same data, and one UNet training step (forward, Charbonnier,
backward, AdamW): dehaze_hip/unet.py on the kernels with FlatAdamW, beside the same module's plain-torch path (library convolution)
with torch.optim.AdamW.  Prints one line per shape and one for the step.

usage:  python tools/bench_unet.py [--batch 32] [--iters 20]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402


def layer_shapes(dim=32, ps=128):
    """(Cin, Kout, H) of every dense 3x3 convolution of UNet(dim) at ps x ps (M1:48-115), without the 3-channel ends"""
    ch = [dim, 2 * dim, 4 * dim, 8 * dim, 16 * dim]
    out = [(ch[0], ch[0], ps)]
    for i in range(1, 5):
        out += [(ch[i - 1], ch[i], ps >> i), (ch[i], ch[i], ps >> i)]
    for i in range(3, -1, -1):
        out += [(ch[i + 1], ch[i], ps >> i), (ch[i], ch[i], ps >> i)]
    return out


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    B = a.batch
    for Cin, Kout, H in layer_shapes():
        x = torch.randn(B, Cin, H, H, device="cuda")
        dy = torch.randn(B, Kout, H, H, device="cuda")
        xb = x.view(B, Cin // 8, 8, H, H).permute(0, 1, 3, 4, 2).contiguous()
        dyb = dy.view(B, Kout // 8, 8, H, H).permute(0, 1, 3, 4, 2).contiguous()
        need = lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, H, Cin, Kout)
        ws = torch.empty(need // 4, device="cuda")
        dw, db = torch.empty(Kout, Cin, 3, 3, device="cuda"), torch.empty(Kout, device="cuda")
        us = timed(lambda: _lib.call("dhz_conv3x3_wgrad", xb.data_ptr(), dyb.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), need,
                                     B, H, H, Cin, Kout, s), a.iters)
        us_lib = timed(lambda: torch.nn.grad.conv2d_weight(x, (Kout, Cin, 3, 3), dy, padding=1), a.iters)
        flop = 2.0 * 9 * Cin * Kout * B * H * H
        print(f"wgrad {Cin:4d} -> {Kout:4d} @ {H:3d}x{H:<3d} batch {B}: hip {us:9.1f} us ({flop / us * 1e-6:6.1f} TFLOP/s, "
              f"{lib.dhz_conv3x3_wgrad_parts(B, H, H, Cin, Kout)} slabs, ws {need / 2**20:.1f} MB)   library {us_lib:9.1f} us")
    if a.no_step:
        return
    import warnings
    from dehaze_hip.unet import UNet
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    from losses import CharbonnierLoss
    gt, hazy = synthetic_batch(B, 128, seed=1)
    gt, hazy = gt.cuda(), hazy.cuda()
    crit = CharbonnierLoss()
    torch.manual_seed(0)
    model = UNet(dim=32).cuda()
    opt = FlatAdamW(model)
    us = timed(lambda: train_step(model, crit, None, opt, None, hazy, gt, w_cr=0.0), a.iters)
    print(f"UNet dim 32, 128 x 128, batch {B}: training step on the kernels {us / 1e3:.2f} ms")
    torch.manual_seed(0)
    ref = UNet(dim=32).cuda()
    ropt = torch.optim.AdamW(ref.parameters(), lr=2e-4, weight_decay=0.02)

    def step():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ropt.zero_grad(set_to_none=True)
            loss, _ = crit.forward_clamped(ref._forward_torch(hazy), gt)
            loss.backward()
            ropt.step()
    print(f"UNet dim 32, 128 x 128, batch {B}: training step, library convolution {timed(step, a.iters) / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
