#!/usr/bin/env python3
"""Validation scores on the device (dhz_ssim_pair, dehaze_hip/metrics.py) against the host route they are an option to.  Per image, at
1 x 3 x 460 x 620 (SOTS / ITS frames) and 1 x 3 x 1200 x 1600 (NH-HAZE frames), wall time with the device idle before and after:
  host, uniform    what FFA_main.evaluate does per image: D2H copy of the restored image + utils/metrics.py (SSIM and PSNR), on the CPUs
                   this process may use
  host, Gaussian   what eval_any_resolution.py adds per image: utils.SSIM + utils.batch_PSNR (ATen, fp32) on the host copy
  device, uniform  Scores.add_uniform + the single read-back
  device, FFA      Scores.add_ffa + the single read-back
and the kernel alone (the C entry with a preallocated workspace: both launches) by device events, K = 7 valid and K = 11 zero-padded.
Then the validation pass: FFA_main.evaluate of FFA(3, --blocks) over --pairs synthetic 460 x 620 pairs with metrics = host / device /
ffa, alternated.  No threshold: the numbers are the result.  Writes profiles/gpu_metrics.txt.

usage:  python tools/bench_metrics.py [--blocks 19] [--pairs 8] [--rounds 3] [--out profiles/gpu_metrics.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(1, 3, 460, 620), (1, 3, 1200, 1600)]


def wall(fn, iters):
    """ms per call, the device drained before the first call and after the last"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpu_metrics.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py measures on the GPU"
    import FFA_main
    import utils
    from dehaze_hip import _lib, ffa, metrics as DM
    from dehaze_hip.train import synthetic_batch
    from utils.metrics import peak_signal_noise_ratio, structural_similarity
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_metrics.py on {torch.cuda.get_device_name(0)}; host threads: torch {torch.get_num_threads()}, "
        f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
    say("per image, ms (wall time per call; kernel rows: device events over the C entry's two launches)")
    for shape in SHAPES:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(H)
        gt = torch.rand(shape, generator=g).cuda()
        pred = (gt + 0.05 * torch.randn(shape, generator=g).cuda()).clamp(0, 1)
        big = H * W > 10 ** 6

        def host_uniform():
            x, y = gt[0].permute(1, 2, 0).cpu().numpy(), pred[0].permute(1, 2, 0).cpu().numpy()
            return peak_signal_noise_ratio(x, y), structural_similarity(x, y, multichannel=True)

        def host_gauss():
            r, t = pred.cpu(), gt.cpu()
            return utils.SSIM(r, t).item(), utils.batch_PSNR(r, t, False).item()

        def dev_uniform():
            s = DM.Scores()
            s.add_uniform(pred, gt)
            return s.read()

        def dev_ffa():
            s = DM.Scores()
            s.add_ffa(pred, gt)
            return s.read()

        need = lib.dhz_ssim_pair_workspace_bytes(B, C, H, W)
        ws = torch.empty(need // 8, dtype=torch.float64, device="cuda")
        out = torch.empty(2, B * C, dtype=torch.float64, device="cuda")

        def kernel(K, valid, kind, wscale, c1, c2, cov, clamp):
            tab = DM._table(kind, gt.device)
            return lambda: _lib.call("dhz_ssim_pair", out[0].data_ptr(), out[1].data_ptr(), gt.data_ptr(), C * H * W, H * W, pred.data_ptr(),
                                     C * H * W, H * W, B, C, H, W, K, tab.data_ptr(), wscale, valid, c1, c2, cov, clamp, ws.data_ptr(), need,
                                     torch.cuda.current_stream().cuda_stream)

        hu, du = host_uniform(), dev_uniform()
        say(f"  {B} x {C} x {H} x {W}   (device - host: SSIM {du[0][0] - hu[1]:+.2e}, PSNR {du[1][0] - hu[0]:+.2e} dB)")
        rows = [("host, uniform (D2H + utils/metrics.py)", lambda: wall(host_uniform, 2 if big else 5)),
                ("host, Gaussian (D2H + utils.SSIM / batch_PSNR)", lambda: wall(host_gauss, 2 if big else 5)),
                ("device, uniform (Scores + read-back)", lambda: wall(dev_uniform, 20)),
                ("device, FFA form (Scores + read-back)", lambda: wall(dev_ffa, 20)),
                ("kernel, K = 7 valid", lambda: events(kernel(7, 1, "ones", 1 / 49.0, 4e-4, 36e-4, 49 / 48.0, 0), 20)),
                ("kernel, K = 11 zero-padded", lambda: events(kernel(11, 0, "gauss", 1.0, 1e-4, 9e-4, 1.0, 1), 20))]
        times = {name: [] for name, _ in rows}
        for _ in range(a.rounds):
            for name, fn in rows:
                times[name].append(fn())
        for name, _ in rows:
            ts = times[name]
            say(f"    {name:48s} " + "  ".join(f"{t:9.3f}" for t in ts) + f"   (median {sorted(ts)[len(ts) // 2]:.3f})")

    say(f"validation pass: FFA_main.evaluate, FFA(3, {a.blocks}), {a.pairs} synthetic 460 x 620 pairs, ms per pass (wall)")
    torch.manual_seed(0)
    net = ffa.FFA(3, a.blocks).cuda()
    vt, vi = synthetic_batch(a.pairs, (460, 620), seed=4321, device="cuda")
    res = {}
    times = {m: [] for m in ("host", "device", "ffa")}
    for _ in range(a.rounds):
        for m in times:
            times[m].append(wall(lambda: res.__setitem__(m, FFA_main.evaluate(net, vt, vi, m)), 1))
    for m, ts in times.items():
        say(f"    --metrics {m:7s} " + "  ".join(f"{t:9.1f}" for t in ts) + f"   (median {sorted(ts)[len(ts) // 2]:.1f})   ssim {res[m][0]:.9f} psnr {res[m][1]:.9f}")
    say(f"    device - host: SSIM {res['device'][0] - res['host'][0]:+.2e}, PSNR {res['device'][1] - res['host'][1]:+.2e} dB")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
