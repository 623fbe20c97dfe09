#!/usr/bin/env python3
"""FFA-Net's perceptual loss on whole images: what the any-size route of the VGG16[:16] engine (ragged Winograd blocks, floor-mode poolings;
dehaze_hip/perceptual.py, perceptual.ANY) buys over the library path that such sizes took before (DHZ_PERLOSS_ANY=0: three VGG16 passes on
library convolutions, and F.l1_loss where 3 B H W is no multiple of 4), and what the ragged edges cost next to the next multiple-of-16 shape.
fp32, one process; per shape three alternated passes of
  kernels     the shape itself, perceptual.ANY on
  library     the shape itself, perceptual.ANY off (the warning silenced); the network stays on its own `_any` kernels
  kernels/16  the next multiple-of-16 shape on the kernels
each pass timed by device events over --iters calls after --warmup calls of that very pass's shape and route.
  PerLoss fwd+bwd   LossNetwork()(x, gt).backward() with x requiring a gradient      1 x 460 x 620, 4 x 250 x 250      /16: 464 x 624, 256 x 256
  training step     ffa_train_step(FFA(3, --blocks), PerLoss, w_per 0.04)            the same shapes
The dispatch rule the numbers are read by: a shape class moves to the kernels only if the kernels' SLOWEST pass beats the
library's FASTEST pass; the last lines of the output say so per shape.  Writes profiles/perloss_any_size.txt.

usage:  python tools/bench_perloss_any.py [--iters 30] [--warmup 3] [--rounds 3] [--blocks 19] [--out profiles/perloss_any_size.txt]
"""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [((1, 460, 620), (1, 464, 624)), ((4, 250, 250), (4, 256, 256))]


def timed(fn, warmup, iters):
    """ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def pair(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(H * W + B)
    gt = torch.rand(B, 3, H, W, generator=g).cuda()
    return (0.6 * gt + 0.3).clamp(0, 1), gt


def bench(kind, shape, shape16, model, opt, per, a, say):
    from dehaze_hip import perceptual
    from dehaze_hip.train import ffa_train_step
    data = {shape: pair(shape), shape16: pair(shape16)}

    def call(s):
        hazy, gt = data[s]
        if kind == "PerLoss fwd+bwd":
            x = hazy.detach().requires_grad_()
            per(x, gt).backward()
        else:
            ffa_train_step(model, per, opt, None, hazy, gt, w_per=0.04)

    routes = [("kernels", shape, True), ("library", shape, False), ("kernels/16", shape16, True)]
    times = {name: [] for name, *_ in routes}
    try:
        for _ in range(a.rounds):                            # alternated: a drift of the machine hits all routes alike
            for name, s, on in routes:
                perceptual.ANY = on
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    assert (per.engine_for(data[s][0]) is not None) == on, (name, s)
                    times[name].append(timed(lambda: call(s), a.warmup, a.iters))
    finally:
        perceptual.ANY = True
    for name, s, _ in routes:
        ts = times[name]
        say(f"  {kind:15s} {'%d x %d x %d' % s:14s} {name:11s} " + "  ".join(f"{t:8.2f}" for t in ts) + f"  ms   (median {sorted(ts)[len(ts) // 2]:.2f})")
    slow, fast = max(times["kernels"]), min(times["library"])
    verdict = "kernels" if slow < fast else "library"
    return f"  {kind:15s} {'%d x %d x %d' % shape:14s} kernels' slowest pass {slow:.2f} ms, library's fastest pass {fast:.2f} ms -> {verdict}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perloss_any_size.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_perloss_any.py measures on the GPU"
    from dehaze_hip import ffa
    from dehaze_hip.perceptual import LossNetwork
    from dehaze_hip.train import FlatAdamW
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_perloss_any.py on {torch.cuda.get_device_name(0)}: PerLoss (VGG16[:16], seeded weights), FFA(3, {a.blocks}), fp32; ms per call "
        f"by device events, {a.rounds} alternated passes of {a.iters} calls each after {a.warmup} calls of warm-up per pass")
    torch.manual_seed(0)
    model = ffa.FFA(3, a.blocks)
    opt = FlatAdamW(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.cuda().train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        per = LossNetwork().cuda()
    verdicts = []
    for kind in ("PerLoss fwd+bwd", "training step"):
        for shape, shape16 in SHAPES:
            verdicts.append(bench(kind, shape, shape16, model, opt, per, a, say))
    say("dispatch rule (kernels only where their slowest pass beats the library's fastest):")
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
