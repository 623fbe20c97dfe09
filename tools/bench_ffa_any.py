#!/usr/bin/env python3
"""FFA-Net on whole images: what the `_any` entries (ragged maps on the HIP kernels, dehaze_hip/ffa.py) buy over the library path that
such sizes took before (DHZ_FFA_ANY=0), and what the ragged edges cost next to the nearest multiple-of-16 shape.  FFA(3, 19), fp32, one
process, one model; per shape three alternated passes of
  kernels     the shape itself, ffa.ANY on
  library     the shape itself, ffa.ANY off (library convolutions + ATen attention, the warning silenced)
  kernels/16  the nearest multiple-of-16 shape on the kernels
each pass timed by device events over --iters calls after --warmup calls of that very pass's shape and route.
  eval forward   (torch.no_grad, eval mode)  1 x 460 x 620 (SOTS-indoor), 1 x 413 x 550      /16: 464 x 624, 416 x 560
  training step  (ffa_train_step, L1 only)   1 x 460 x 620, 4 x 250 x 250                    /16: 464 x 624, 256 x 256
The dispatch rule the numbers are read by: a shape class moves to the kernels only if the kernels' SLOWEST pass beats the library's
FASTEST pass; the last lines of the output say so per shape.  Writes profiles/ffa_any_size.txt.

usage:  python tools/bench_ffa_any.py [--iters 30] [--warmup 3] [--rounds 3] [--blocks 19] [--out profiles/ffa_any_size.txt]
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

EVAL = [((1, 460, 620), (1, 464, 624)), ((1, 413, 550), (1, 416, 560))]
TRAIN = [((1, 460, 620), (1, 464, 624)), ((4, 250, 250), (4, 256, 256))]


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


def bench(kind, shape, shape16, model, opt, a, say):
    from dehaze_hip import ffa
    from dehaze_hip.train import ffa_train_step
    data = {shape: pair(shape), shape16: pair(shape16)}

    def call(s):
        hazy, gt = data[s]
        if kind == "eval forward":
            with torch.no_grad():
                model(hazy)
        else:
            ffa_train_step(model, None, opt, None, hazy, gt)

    model.eval() if kind == "eval forward" else model.train()
    routes = [("kernels", shape, True), ("library", shape, False), ("kernels/16", shape16, True)]
    times = {name: [] for name, *_ in routes}
    try:
        for _ in range(a.rounds):                            # alternated: a drift of the machine hits all routes alike
            for name, s, on in routes:
                ffa.ANY = on
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    times[name].append(timed(lambda: call(s), a.warmup, a.iters))
    finally:
        ffa.ANY = True
    for name, s, _ in routes:
        ts = times[name]
        say(f"  {kind:14s} {'%d x %d x %d' % s:14s} {name:11s} " + "  ".join(f"{t:8.2f}" for t in ts) + f"  ms   (median {sorted(ts)[len(ts) // 2]:.2f})")
    slow, fast = max(times["kernels"]), min(times["library"])
    verdict = "kernels" if slow < fast else "library"
    return f"  {kind:14s} {'%d x %d x %d' % shape:14s} kernels' slowest pass {slow:.2f} ms, library's fastest pass {fast:.2f} ms -> {verdict}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffa_any_size.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ffa_any.py measures on the GPU"
    from dehaze_hip import ffa
    from dehaze_hip.train import FlatAdamW
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_ffa_any.py on {torch.cuda.get_device_name(0)}: FFA(3, {a.blocks}), fp32; ms per call by device events, {a.rounds} alternated "
        f"passes of {a.iters} calls each after {a.warmup} calls of warm-up per pass")
    torch.manual_seed(0)
    model = ffa.FFA(3, a.blocks)
    opt = FlatAdamW(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.cuda()
    verdicts = []
    for shape, shape16 in EVAL:
        verdicts.append(bench("eval forward", shape, shape16, model, opt, a, say))
    for shape, shape16 in TRAIN:
        verdicts.append(bench("training step", shape, shape16, model, opt, a, say))
    say("dispatch rule (kernels only where their slowest pass beats the library's fastest):")
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
