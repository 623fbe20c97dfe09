#!/usr/bin/env python3
"""Cost of the deterministic mode (dehaze_hip.ops.set_deterministic): the headline training step (Uformer E = 32, 256 x 256, batch 8, fp32
storage, Charbonnier + CR + FlatAdamW) and three token-Linear weight-gradient shapes on their own, each with the mode off and on, same
process, same box.  Protocol: warm-up iterations first (code objects loaded, clocks up), then `--repeats` timed blocks per setting,
INTERLEAVED off / on / off / on so that drift hits both alike; a block is `--iters` (the step) or `--wgrad-iters` (a weight gradient)
back-to-back iterations between two device events - windows of more than half a second and of about 0.2 s; reported: the median block and
the min..max spread, per iteration, with the iteration count of the row.  Writes the table to --out (default profiles/det_mode_cost.txt).

    python tools/bench_deterministic.py [--batch 8] [--size 256] [--repeats 5] [--iters 20] [--wgrad-iters 2000] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
sys.path[:0] = [PKG, ROOT]

import torch  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(fn, ops, warmup, repeats, iters):
    """{False: [ms per iteration of each block], True: [...]}"""
    out = {False: [], True: []}
    for on in (False, True):
        ops.set_deterministic(on)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for on in (False, True):
            ops.set_deterministic(on)
            out[on].append(timed(fn, iters))
    ops.set_deterministic(False)
    return out


def row(name, r, iters, unit="ms"):
    k = 1.0 if unit == "ms" else 1000.0
    off, on = statistics.median(r[False]) * k, statistics.median(r[True]) * k
    return (f"{name:<44} off {off:9.3f} {unit} [{min(r[False]) * k:.3f} .. {max(r[False]) * k:.3f}]   "
            f"on {on:9.3f} {unit} [{min(r[True]) * k:.3f} .. {max(r[True]) * k:.3f}]   on/off {on / off:5.2f}x   ({iters} iterations per block)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="training steps per timed block")
    ap.add_argument("--wgrad-iters", type=int, default=2000, help="weight-gradient launches per timed block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_mode_cost.txt"))
    a = ap.parse_args()
    from dehaze_hip import _lib, ops
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    import My_CR
    import My_model_1 as M1
    from losses import CharbonnierLoss
    dev = torch.device("cuda:0")
    lines = [f"deterministic-mode cost  (device: {torch.cuda.get_device_name(0)}, library {_lib.load().dhz_build_id().decode()})",
             f"protocol: {a.warmup} warm-up iterations per setting, {a.repeats} interleaved blocks per setting (iterations per block: at the end of each row); median [min .. max] per iteration", ""]

    torch.manual_seed(1234)
    model = M1.Uformer(img_size=a.size, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev).train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cr = My_CR.ContrastLoss().to(dev)
    opt = FlatAdamW(model)
    gt, hazy = synthetic_batch(a.batch, a.size, seed=5)
    gt, hazy = gt.to(dev), hazy.to(dev)
    crit = CharbonnierLoss()
    lines.append(row(f"training step E=32 {a.size}x{a.size} batch {a.batch}",
                     interleaved(lambda: train_step(model, crit, cr, opt, None, hazy, gt), ops, a.warmup, a.repeats, a.iters), a.iters))
    del model, cr, opt

    for T, K, nper in ((131072, 128, 128), (524288, 32, 32), (32768, 256, 256)):          # (T, K, N = 3 nper): the packed Q / K / V gradients
        N = 3 * nper
        dy, x = torch.randn(T, N, device=dev), torch.randn(T, K, device=dev)
        dws = [torch.zeros(nper, K, device=dev) for _ in range(3)]
        dbs = [torch.zeros(nper, device=dev) for _ in range(3)]
        pw = ctypes.cast((ctypes.c_void_p * 3)(*[t.data_ptr() for t in dws]), ctypes.c_void_p)
        pb = ctypes.cast((ctypes.c_void_p * 3)(*[t.data_ptr() for t in dbs]), ctypes.c_void_p)
        if K % 64 == 0:
            fn = lambda: _lib.call("dhz_linear_wgrad_split", dy.data_ptr(), N, x.data_ptr(), K, T, 3, nper, K, pw, pb, None, 0, 6, ops._stream())  # noqa: E731
        else:
            fn = lambda: _lib.call("dhz_linear_wgrad_multi", dy.data_ptr(), N, x.data_ptr(), K, T, 3, nper, K, pw, pb, ops._stream())  # noqa: E731
        lines.append(row(f"weight gradient T={T} K={K} N={N}", interleaved(fn, ops, a.warmup, a.repeats, a.wgrad_iters), a.wgrad_iters, unit="us"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
