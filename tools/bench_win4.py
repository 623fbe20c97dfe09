#!/usr/bin/env python3
"""Times the 16-token window-attention kernels (csrc/ps_attn16.hip) and one training step at 64 x 64 patches.

  python tools/bench_win4.py kernels     us per launch and bytes per second of dhz_ps_attn_fwd_w / _bwd_w (win = 4) at
                                         the bottleneck of train_ps 64, batch 32, E = 32 (B_ = 32, H = 16, d = 32) and at the first
                                         level of --win_size 4 at 64 px, batch 32 (B_ = 8192, H = 1, d = 32), beside the HBM floor of
                                         each launch (the bytes of q, k, v, out - backward: + dO, dq, dk, dv - over the device's peak)
  python tools/bench_win4.py step        ms per training step at train_ps 64, batch 32, E = 32, Charbonnier + CR + AdamW

Each mode is one process; run each under its own time limit (`timeout -k 10 300 python tools/bench_win4.py kernels`).  Timing: HIP events
around single launches on a warm device, inputs re-used (they fit the memory-side cache at the small shape: the figure there is launch
latency, not bandwidth), median and minimum of 200 launches after 20 warm-up launches."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, MI355X
REF_FRACTION = 0.358       # of HBM peak: the unfused 64-token forward kernel


def _time(fn, n=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts), min(ts)


def kernels():
    from dehaze_hip import _lib, ops
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"{'shape':<28}{'kernel':<10}{'median us':>10}{'min us':>9}{'floor us':>10}{'TB/s':>8}{'of peak':>9}"]
    for B_, H, d in ((32, 16, 32), (8192, 1, 32)):
        C = H * d
        g = torch.Generator(device=dev).manual_seed(0)
        qkv = torch.randn(B_ * 16, 3 * C, device=dev, generator=g)
        gout = torch.randn(B_ * 16, C, device=dev, generator=g)
        table = 0.3 * torch.randn(49, H, device=dev, generator=g)
        idx = torch.randint(16, (16, 15), device=dev, generator=g).to(torch.uint8)
        bias = ops.bias_tile(table, H, 16)
        out = torch.empty(B_ * 16, C, device=dev)
        rank = torch.empty(B_ * H * 16, device=dev, dtype=torch.uint8)
        dqkv = torch.empty_like(qkv)
        parts = _lib.load().dhz_ps_attn_bwd_parts_w(B_, H, d, 4)
        dpart = torch.empty(parts, 16, 16, device=dev)
        base, gb = qkv.data_ptr(), dqkv.data_ptr()

        def fwd():
            _lib.call("dhz_ps_attn_fwd_w", base, base + 4 * C, base + 8 * C, 3 * C, idx.data_ptr(), bias.data_ptr(), None, out.data_ptr(), C,
                      rank.data_ptr(), B_, H, 1, d, 4, 0, s)

        def bwd():
            _lib.call("dhz_ps_attn_bwd_w", base, base + 4 * C, base + 8 * C, 3 * C, bias.data_ptr(), None, rank.data_ptr(), gout.data_ptr(), C,
                      gb, gb + 4 * C, gb + 8 * C, 3 * C, dpart.data_ptr(), B_, H, 1, d, 4, 0, s)

        for name, fn, tensors in (("forward", fwd, 4), ("backward", bwd, 8)):
            nbytes = tensors * B_ * 16 * C * 4
            med, mn = _time(fn)
            floor = nbytes / HBM_PEAK * 1e6
            bw = nbytes / (med * 1e-6)
            lines.append(f"{f'B_={B_} H={H} d={d}':<28}{name:<10}{med:>10.2f}{mn:>9.2f}{floor:>10.2f}{bw / 1e12:>8.3f}{bw / HBM_PEAK:>9.3f}")
    lines.append(f"(the unfused 64-token forward kernel runs at {REF_FRACTION} of HBM peak, VERDICT.md)")
    print("\n".join(lines))


def step():
    import warnings
    import My_CR
    import My_model_1 as M1
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    from losses import CharbonnierLoss
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev)
    model.train()
    opt = FlatAdamW(model)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cr = My_CR.ContrastLoss().to(dev)
    gt, hazy = synthetic_batch(32, 64, seed=5)
    gt, hazy = gt.to(dev), hazy.to(dev)
    crit = CharbonnierLoss()
    for _ in range(5):
        train_step(model, crit, cr, opt, None, hazy, gt)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        train_step(model, crit, cr, opt, None, hazy, gt)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(f"train_ps 64, batch 32, E = 32, Charbonnier + CR + AdamW: median {statistics.median(ts):.2f} ms per step, min {min(ts):.2f} (20 steps)")


if __name__ == "__main__":
    {"kernels": kernels, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "kernels"]()
