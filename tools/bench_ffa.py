#!/usr/bin/env python3
"""Times the FFA-Net attention entries (csrc/ffa_attn.hip) at B = 2, 240 x 240 (FFA-Net's own crop and batch) and B = 8, 128 x 128: us per
launch by device events, beside the bytes the formulas of include/dehaze_hip.h (K13) move and the resulting GB/s; then one training step
(train_step, Charbonnier, FlatAdamW) of FFA(3, 19) at the same two shapes on the kernels and on the same module's _forward_torch on the
device (the library convolutions and ATen elementwise operations), alternated in one process after warm-up.  Writes
profiles/ffa_kernels.txt.

usage:  python tools/bench_ffa.py [--iters 50] [--steps 4] [--rounds 3] [--blocks 19] [--out profiles/ffa_kernels.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(2, 240, 240), (8, 128, 128)]


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


def formula_bytes(B, H, W, G):
    """bytes each entry moves by its formulas: whole maps read and written once, the small vectors and the workspace partials counted too"""
    m = 4.0 * B * 64 * H * W
    n, hc = 64 * G, 8 if G == 1 else 4
    chunks = H * W // 128
    slot = 4.0 * (n + 532)
    vec = 4.0 * B * n
    part = B * chunks * slot
    seg = B * ((chunks + 15) // 16) * slot
    return {
        "dhz_ffa_ca_fwd": G * m + 2 * 4.0 * B * G * ((H * W + 1023) // 1024) * 64 + 2 * vec + 4.0 * B * hc,
        "dhz_ffa_gate_pa_fwd": (G + (2 if G == 1 else 1)) * m + vec,            # G = 1: + the residual
        "dhz_ffa_gate_pa_bwd_a": (G + 2) * m + part + vec,                      # the maps' second read (dca) comes from the cache
        "dhz_ffa_ca_bwd": part + 2 * seg + 4 * vec,
        "dhz_ffa_gate_pa_bwd_b": (1 + G) * m + 2 * vec,
        "dhz_ffa_add": 3 * m,
        "dhz_ffa_relu_bwd_add": 5 * m,
    }


def bench_entries(B, H, W, G, iters, say):
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    n, hc = 64 * G, 8 if G == 1 else 4
    dev = "cuda"
    maps = [torch.randn(B, 8, H, W, 8, device=dev) for _ in range(G)]
    mp = [t.data_ptr() for t in maps] + [None] * (3 - G)
    res = torch.randn(B, 8, H, W, 8, device=dev) if G == 1 else None
    dout, out, dt = (torch.randn(B, 8, H, W, 8, device=dev) for _ in range(3))
    dm = [torch.empty(B, 8, H, W, 8, device=dev) for _ in range(G)]
    dmp = [t.data_ptr() for t in dm] + [None] * (3 - G)
    Wa, ba, Wb, bb = torch.randn(hc, n, device=dev) / n ** 0.5, torch.randn(hc, device=dev), torch.randn(n, hc, device=dev), torch.randn(n, device=dev)
    Wp1, bp1, wp2, bp2 = torch.randn(8, 64, device=dev) / 8, torch.randn(8, device=dev), torch.randn(8, device=dev), torch.randn(1, device=dev)
    mean, hid, ca, dmean = torch.empty(B, n, device=dev), torch.empty(B, hc, device=dev), torch.empty(B, n, device=dev), torch.empty(B, n, device=dev)
    g = [torch.empty_like(t) for t in (Wa, ba, Wb, bb, Wp1, bp1, wp2, bp2)]
    need = lib.dhz_ffa_workspace_bytes(B, H, W, G)
    ws = torch.empty(need // 4, device=dev)
    P = lambda *ts: [t.data_ptr() for t in ts]  # noqa: E731
    calls = {
        "dhz_ffa_ca_fwd": lambda: _lib.call("dhz_ffa_ca_fwd", *mp, *P(Wa, ba, Wb, bb, mean, hid, ca, ws), need, B, H, W, G, s),
        "dhz_ffa_gate_pa_fwd": lambda: _lib.call("dhz_ffa_gate_pa_fwd", *mp, *P(ca, Wp1, bp1, wp2, bp2), res.data_ptr() if G == 1 else None,
                                                 out.data_ptr(), B, H, W, G, s),
        "dhz_ffa_gate_pa_bwd_a": lambda: _lib.call("dhz_ffa_gate_pa_bwd_a", *mp, *P(ca, Wp1, bp1, wp2, bp2, dout, dt, ws), need, B, H, W, G, s),
        "dhz_ffa_ca_bwd": lambda: _lib.call("dhz_ffa_ca_bwd", ws.data_ptr(), need, *P(Wa, Wb, mean, hid, ca, g[0], g[1], g[2], g[3], dmean,
                                                                                      g[4], g[5], g[6], g[7]), B, H, W, G, s),
        "dhz_ffa_gate_pa_bwd_b": lambda: _lib.call("dhz_ffa_gate_pa_bwd_b", *P(dt, ca, dmean), *dmp, B, H, W, G, s),
    }
    if G == 1:
        nel = maps[0].numel()
        calls["dhz_ffa_add"] = lambda: _lib.call("dhz_ffa_add", *P(maps[0], res, out), nel, s)
        calls["dhz_ffa_relu_bwd_add"] = lambda: _lib.call("dhz_ffa_relu_bwd_add", *P(maps[0], dout, res, out, dt), nel, s)
    nbytes = formula_bytes(B, H, W, G)
    total_us = total_b = 0.0
    for name, fn in calls.items():
        us = timed(fn, iters)
        total_us += us
        total_b += nbytes[name]
        say(f"  {name:24s} G={G}  {us:8.1f} us   {nbytes[name] / 2**20:8.2f} MiB by the formulas   {nbytes[name] / us * 1e-3:7.0f} GB/s")
    say(f"  {'all of the above':24s} G={G}  {total_us:8.1f} us   {total_b / 2**20:8.2f} MiB")


def bench_step(B, H, W, blocks, steps, rounds, say):
    import warnings
    from dehaze_hip import ffa
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(B, 3, H, W, generator=g).cuda()
    hazy = (0.6 * gt + 0.3).clamp(0, 1)
    crit = CharbonnierLoss()
    torch.manual_seed(0)
    model = ffa.FFA(3, blocks).cuda()
    torch.manual_seed(0)
    ref = ffa.FFA(3, blocks).cuda()
    ref.forward = ref._forward_torch                     # the same module on the library path
    opt, ropt = FlatAdamW(model), FlatAdamW(ref)

    def run(net, o, f43):
        ffa.FWD_F43 = ffa.BWD_F43 = f43
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return timed(lambda: train_step(net, crit, None, o, None, hazy, gt, w_cr=0.0), steps) / 1e3

    paths = [("kernels, F(2x2) Winograd", model, opt, False), ("kernels, F(4x4) Winograd", model, opt, True), ("library path", ref, ropt, False)]
    times = {name: [] for name, *_ in paths}
    for _ in range(rounds):                              # alternated: a drift of the machine hits all paths alike
        for name, net, o, f43 in paths:
            times[name].append(run(net, o, f43))
    ffa.FWD_F43 = ffa.BWD_F43 = False
    for name, ts in times.items():
        say(f"  FFA(3, {blocks}) training step, B = {B}, {H} x {W}, {name:26s} " + "  ".join(f"{t:7.2f}" for t in ts)
            + f"  ms   (median {sorted(ts)[len(ts) // 2]:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffa_kernels.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ffa.py measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_ffa.py on {torch.cuda.get_device_name(0)}: us per launch (device events, {a.iters} launches after 3 of warm-up)")
    for B, H, W in SHAPES:
        say(f"B = {B}, {H} x {W} (one map = {4 * B * 64 * H * W / 2**20:.1f} MiB)")
        for G in (1, 3):
            bench_entries(B, H, W, G, a.iters, say)
    if not a.no_step:
        say(f"training step, {a.rounds} alternated rounds of {a.steps} steps each after 3 steps of warm-up")
        for B, H, W in SHAPES:
            bench_step(B, H, W, a.blocks, a.steps, a.rounds, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
