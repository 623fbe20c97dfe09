"""The four Downsample convolutions of the headline step (E = 32, 128 x 128, bs 32, fp32), us per call: the fp32-pipe entries
(dhz_conv4s2_fwd, and dhz_conv4s2_dgrad = four launches, one per parity class) against the six-term entries (dhz_conv4s2_fwd6,
dhz_conv4s2_dgrad6 = one launch), and the weight-plane launch (dhz_conv4s2_prepack6) against the two ATen permute copies it replaces.
Device events around 10 calls, 5 alternated rounds (fp32, six-term, fp32, ...); minimum and spread (max - min) over the rounds.  A level
enters ops.CONV4S2_SPLIT6_FWD / _DGRAD only if the six-term entry wins by more than the larger spread.
    python tools/bench_conv4s2.py [check]          check: compare the results of both routes before timing"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd"), ROOT]
import torch
from dehaze_hip import _lib
dev = torch.device("cuda:0")
BS, ROUNDS, CALLS = 32, 5, 10
CHECK = "check" in sys.argv[1:]
LEVELS = [(128, 32, 64), (64, 64, 128), (32, 128, 256), (16, 256, 512)]          # (map side, Cin, Cout)
lib = _lib.load()


def once(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3


def alternate(fa, fb):
    """(min a, spread a, min b, spread b) over alternated rounds"""
    for _ in range(3): fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(once(fa)); tb.append(once(fb))
    return min(ta), max(ta) - min(ta), min(tb), max(tb) - min(tb)


print(f"{'map':>4} {'Cin':>4} {'Cout':>4} {'product':>8} | {'fp32':>7} (+-) | {'six':>7} (+-) tile | gain us  TFLOP/s fp32 -> six")
wins = {"fwd": [], "dgrad": []}
for S, Cin, Cout in LEVELS:
    B, H, W = BS, S, S
    s = torch.cuda.current_stream().cuda_stream
    x = torch.randn(B, H * W, Cin, device=dev)
    w = torch.randn(Cout, Cin, 4, 4, device=dev) * 0.05
    b = torch.randn(Cout, device=dev)
    dy = torch.randn(B, H * W // 4, Cout, device=dev)
    y, y6, dx, dx6 = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(x), torch.empty_like(x)
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).contiguous()
    wq = w.permute(2, 3, 0, 1).contiguous()
    pf = torch.empty((3, 16 * Cin * Cout), device=dev, dtype=torch.int16)
    pb = torch.empty_like(pf)
    p = lambda t: t.data_ptr()
    prepack = lambda: _lib.call("dhz_conv4s2_prepack6", p(w), p(pf), p(pb), Cin, Cout, s)
    prepack()
    routes = {
        "fwd": (lambda: _lib.call("dhz_conv4s2_fwd", p(x), p(wp), p(b), p(y), B, H, W, Cin, Cout, s),
                lambda: _lib.call("dhz_conv4s2_fwd6", p(x), p(pf), p(b), p(y6), B, H, W, Cin, Cout, s), 1, (y, y6)),
        "dgrad": (lambda: _lib.call("dhz_conv4s2_dgrad", p(dy), p(wq), p(dx), B, H, W, Cin, Cout, s),
                  lambda: _lib.call("dhz_conv4s2_dgrad6", p(dy), p(pb), p(dx6), B, H, W, Cin, Cout, s), 2, (dx, dx6)),
    }
    gflop = 2.0 * B * (H // 2) * (W // 2) * Cout * 16 * Cin / 1e9
    for name, (f32, f6, mode, outs) in routes.items():
        if CHECK:
            f32(); f6(); torch.cuda.synchronize()
            err, scale = (outs[0] - outs[1]).abs().max().item(), outs[0].abs().max().item()
            print(f"    check {name}: max |fp32 - six| = {err:.3e} of max {scale:.3e}")
            assert err <= 1e-4 * scale, (S, Cin, Cout, name)
        t0, s0, t6, s6 = alternate(f32, f6)
        win = t0 - t6 > max(s0, s6)
        if win: wins[name].append((Cin, Cout))
        print(f"{S:4d} {Cin:4d} {Cout:4d} {name:>8} | {t0:7.1f} {s0:4.1f} | {t6:7.1f} {s6:4.1f} {lib.dhz_conv4s2_tile6(mode, B, H, W, Cin, Cout):4d} | "
              f"{t0 - t6:7.1f}  {gflop / t0 * 1e3:6.1f} -> {gflop / t6 * 1e3:6.1f}  {'win' if win else 'no'}")
    copies = lambda: (w.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).contiguous(), w.permute(2, 3, 0, 1).contiguous())
    t0, s0, t6, s6 = alternate(copies, prepack)
    print(f"{S:4d} {Cin:4d} {Cout:4d} {'weights':>8} | {t0:7.1f} {s0:4.1f} | {t6:7.1f} {s6:4.1f}      | {t0 - t6:7.1f}   (two ATen permute copies -> one prepack launch)")
print("levels (Cin, Cout) that win: forward", wins["fwd"], " backward-data", wins["dgrad"])
