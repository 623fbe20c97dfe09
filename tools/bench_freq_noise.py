#!/usr/bin/env python3
"""The frequency-band noise (dhz_band_noise, dehaze_hip/freq_noise.py): the kernel route against the reference's ATen formula
(freq_noise.KERNELS = False, what DHZ_FREQ_NOISE=0 sets), both on the device, in one process, the two routes alternated.

  1. band_noise(x, draw, w1, w2, scale=eps, take_sign=True) on [32, 3, 128, 128], [8, 3, 256, 256] and [1, 3, 512, 512], fp32, for a
     narrow band (f = pi / 2, s = 0.2) and the costliest one (w1 = n, w2 = 0): ms per call by device events over --iters calls per
     pass, --passes passes after a warm-up, the two routes alternated pass by pass; median and spread (min .. max) of the passes
  2. the gap between the two routes' x_adv at those shapes (the ATen arm is fp32 torch.fft)
  3. one band pass of My_robustness.py's loop for the default Uformer at 128 x 128, batch 32: noise + eval forward + clamp + scoring, and
     the noise alone; the share of the pass that the noise takes
  4. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 30 --warmup 10` there and here, alternated, each
     in a fresh child process; the result lines as printed
No threshold: the numbers are the result.  Writes profiles/freq_noise.txt.

usage:  python tools/bench_freq_noise.py [--iters 5] [--passes 20] [--parent DIR] [--runs 2] [--out profiles/freq_noise.txt]
"""
import argparse
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(32, 3, 128), (8, 3, 256), (1, 3, 512)]              # (B, C, n)
ATEN = "ATen formula (DHZ_FREQ_NOISE=0)"
EPS = 0.007


def events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stats(ts):
    s = sorted(ts)
    return s[len(s) // 2], s[0], s[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: part 4")
    ap.add_argument("--runs", type=int, default=2, help="part 4: bench.py runs per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "freq_noise.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_freq_noise.py measures on the GPU"
    from dehaze_hip import _lib, freq_noise
    from dehaze_hip.metrics import Scores
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def route(kernels, fn):
        def run():
            freq_noise.KERNELS = kernels
            try:
                return fn()
            finally:
                freq_noise.KERNELS = True
        return run

    say(f"tools/bench_freq_noise.py on {torch.cuda.get_device_name(0)}, library {lib.dhz_build_id().decode()}")
    say(f"1. band_noise(x, draw, w1, w2, scale={EPS}, take_sign=True), fp32, ms per call (device events over {a.iters} calls per pass; {a.passes} "
        "passes after 3 warm-up passes, the two routes alternated pass by pass): median, min .. max of the passes")
    gaps = []
    for B, C, n in SHAPES:
        g = torch.Generator().manual_seed(n)
        x = torch.rand(B, C, n, n, generator=g).to(dev)
        draw = torch.randn(B, C, n, n, generator=g).to(dev)
        need = lib.dhz_band_noise_workspace_bytes(B * C, n)
        say(f"  [{B}, {C}, {n}, {n}]   (input {x.numel() * 4 / 1e6:.1f} MB, workspace {need / 1e6:.1f} MB)")
        for label, (w1, w2) in (("f = pi/2, s = 0.2", freq_noise.band_widths(math.pi / 2, 0.2, n)), ("whole spectrum", (n, 0))):
            rows = [("kernel route", route(True, lambda: freq_noise.band_noise(x, draw, w1, w2, scale=EPS, take_sign=True))),
                    (ATEN, route(False, lambda: freq_noise.band_noise(x, draw, w1, w2, scale=EPS, take_sign=True)))]
            times = {name: [] for name, _ in rows}
            for i in range(3 + a.passes):
                for name, fn in rows:
                    t = events(fn, a.iters)
                    if i >= 3:
                        times[name].append(t)
            say(f"    {label}: w1 = {w1}, w2 = {w2}")
            med = {}
            for name, _ in rows:
                med[name], lo, hi = stats(times[name])
                say(f"      {name:34s} median {med[name]:8.3f}   min {lo:8.3f}   max {hi:8.3f}")
            flops = 2.0 * (2 if w2 == 0 else 4) * 2 * B * C * n ** 3
            say(f"      ATen / kernel = {med[ATEN] / med['kernel route']:.2f};  kernel route: {flops / med['kernel route'] / 1e9:.2f} TFLOP/s of its "
                "float64 multiply-adds")
            gaps.append(f"  [{B}, {C}, {n}, {n}] ({w1}, {w2}): max |x_adv gap| {(rows[0][1]() - rows[1][1]()).abs().max().item():.3e}")
        del x, draw
    say("2. the two routes' results")
    for gp in gaps:
        say(gp)

    say("3. one band pass of My_robustness.py's loop, default Uformer (embed_dim 32, ProbSparse), [32, 3, 128, 128], band f = pi/2: ms per pass")
    import My_model_1
    from dehaze_hip.train import synthetic_batch
    torch.manual_seed(1234)
    model = My_model_1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection="linear", token_mlp="leff").to(dev).eval()
    gt, hazy = synthetic_batch(32, 128, seed=1234, device=dev)
    draw = torch.randn(hazy.shape, generator=torch.Generator().manual_seed(1234)).to(dev)
    w1, w2 = freq_noise.band_widths(math.pi / 2, 0.2, 128)

    def noise_only():
        return freq_noise.band_noise(hazy, draw, w1, w2, scale=EPS, take_sign=True)

    def band_pass():
        sc = Scores()
        torch.manual_seed(1234)
        sc.add_uniform(model(noise_only()).clamp(0, 1), gt)
        return sc

    with torch.no_grad():
        rows = [("noise + forward + scoring", band_pass), ("noise alone", noise_only)]
        times = {name: [] for name, _ in rows}
        for i in range(3 + a.passes):
            for name, fn in rows:
                t = events(fn, 1)
                if i >= 3:
                    times[name].append(t)
    med = {}
    for name, _ in rows:
        med[name], lo, hi = stats(times[name])
        say(f"    {name:34s} median {med[name]:8.3f}   min {lo:8.3f}   max {hi:8.3f}")
    say(f"    the noise is {100 * med['noise alone'] / med['noise + forward + scoring']:.1f} % of the band pass")
    del model

    if a.parent:
        torch.cuda.synchronize()
        say(f"4. python bench.py --gpus 1 --steps 30 --warmup 10, the parent commit's build and this tree's alternated, {a.runs} runs each, "
            "a fresh process per run")
        for i in range(a.runs):
            for label, where in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "30", "--warmup", "10"], cwd=where, capture_output=True,
                                   text=True, timeout=900)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                say(f"{label}, run {i + 1}:")
                say(out[-1] if r.returncode == 0 and out else f"  FAILED rc={r.returncode}: {r.stderr[-500:]}")
                if r.returncode != 0:
                    write()
                    raise SystemExit("bench_freq_noise.py: bench.py failed; nothing more is started")
    write()


if __name__ == "__main__":
    main()
