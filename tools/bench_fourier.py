#!/usr/bin/env python3
"""The Fourier / variance analysis of a latent (dhz_fourier_diag, dehaze_hip/analysis.py): the kernel route against the notebooks' ATen
formula (analysis.KERNELS = False, what DHZ_FOURIER=0 sets), both on the device - without the notebooks' .cpu() - in one process, the two
routes alternated.

  1. diag_log_amplitude(x) (the sums over maps) on token latents [32, 128^2, 32], [32, 32^2, 128] and [8, 256^2, 64], fp32: ms per call by
     device events over --iters calls after a warm-up, --rounds rounds, the two rows of a shape alternated; and the achieved GB/s of the
     ONE read of the latent (its bytes over the kernel route's median time: the three launches, workspace traffic included in the time);
     the same on NCHW latents [32, 512, 8, 8], [32, 128, 32, 32] and [4, 64, 240, 240]
  2. the gap between the two routes' results at those shapes (the ATen arm is fp32 torch.fft)
  3. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 30 --warmup 10` there and here, alternated, each
     in a fresh child process; the result lines as printed
No threshold: the numbers are the result.  Writes profiles/fourier_analysis.txt.

usage:  python tools/bench_fourier.py [--iters 20] [--rounds 5] [--parent DIR] [--passes 2] [--out profiles/fourier_analysis.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(32, 128, 32), (32, 32, 128), (8, 256, 64)]          # (B, n, C) of tokens [B, n n, C]
NCHW_SHAPES = [(32, 8, 512), (32, 32, 128), (4, 240, 64)]       # (B, n, C) of NCHW [B, C, n, n]
ATEN = "ATen formula (DHZ_FOURIER=0)"


def events(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def row(name, ts, fmt="9.3f"):
    s = sorted(ts)
    return f"    {name:34s} " + "  ".join(format(t, fmt) for t in ts) + f"   median {s[len(s) // 2]:.3f}  min {s[0]:.3f}  max {s[-1]:.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: part 3")
    ap.add_argument("--passes", type=int, default=2, help="part 3: bench.py runs per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_analysis.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fourier.py measures on the GPU"
    from dehaze_hip import _lib, analysis
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
            analysis.KERNELS = kernels
            try:
                return fn()
            finally:
                analysis.KERNELS = True
        return run

    say(f"tools/bench_fourier.py on {torch.cuda.get_device_name(0)}, library {lib.dhz_build_id().decode()}")
    say(f"1. diag_log_amplitude(x), fp32 tokens, ms per call (device events over {a.iters} calls after 3 warm-up calls; {a.rounds} rounds, the two "
        "rows of a shape alternated)")
    gaps = []
    for layout, (B, n, C) in [("tokens", s) for s in SHAPES] + [("nchw", s) for s in NCHW_SHAPES]:
        if layout == "nchw" and (B, n, C) == NCHW_SHAPES[0]:
            say("   ... and NCHW latents [B, C, n, n] (CNN maps taken with ordinary hooks): small maps share a workgroup")
        shape = (B, n * n, C) if layout == "tokens" else (B, C, n, n)
        x = torch.randn(shape, generator=torch.Generator().manual_seed(n)).to(dev)
        rows = [("kernel route", route(True, lambda: analysis.diag_log_amplitude(x, layout))),
                (ATEN, route(False, lambda: analysis.diag_log_amplitude(x, layout)))]
        times = {name: [] for name, _ in rows}
        for _ in range(a.rounds):
            for name, fn in rows:
                times[name].append(events(fn, a.iters))
        need = lib.dhz_fourier_diag_workspace_bytes(B, C, n, analysis.LAYOUTS[layout])
        label = f"[{B}, {n}^2, {C}]" if layout == "tokens" else f"[{B}, {C}, {n}, {n}] NCHW"
        say(f"  {label}   (latent {x.numel() * 4 / 1e6:.1f} MB, workspace {need / 1e6:.1f} MB)")
        for name, _ in rows:
            say(row(name, times[name]))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        say(f"    kernel route: {x.numel() * 4 / med['kernel route'] / 1e6:.0f} GB/s of the one read;  ATen / kernels = {med[ATEN] / med['kernel route']:.2f}")
        (ka, kv), (ta, tv) = rows[0][1](), rows[1][1]()
        m = B * C
        gaps.append(f"  {label}: max |mean A gap| {((ka - ta).abs().max() / m).item():.3e}, mean V: kernels {kv.item() / m:.9f}, "
                    f"ATen {tv.item() / m:.9f}")
        del x
    say("2. the two routes' results (means over the maps)")
    for g in gaps:
        say(g)

    if a.parent:
        torch.cuda.synchronize()
        say(f"3. python bench.py --gpus 1 --steps 30 --warmup 10, the parent commit's build and this tree's alternated, {a.passes} passes each, "
            "a fresh process per run")
        for i in range(a.passes):
            for label, where in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "30", "--warmup", "10"], cwd=where, capture_output=True,
                                   text=True, timeout=900)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                say(f"{label}, run {i + 1}:")
                say(out[-1] if r.returncode == 0 and out else f"  FAILED rc={r.returncode}: {r.stderr[-500:]}")
                if r.returncode != 0:
                    write()
                    raise SystemExit("bench_fourier.py: bench.py failed; nothing more is started")
    write()


if __name__ == "__main__":
    main()
