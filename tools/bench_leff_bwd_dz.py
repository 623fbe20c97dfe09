"""LeFF backward, the dz stage, us per call on the nine (C, map) shapes of the headline step (E = 32, 128 x 128, bs 32, fp32): the chain
(backward-data product dz = dy . W2 through ops.gemm_dgrad with a FlatAdamW's W^T planes, as the step runs it, then
dhz_leff_dwconv_bwd_scaled_dt) against dhz_leff_dwconv_bwd_dy (csrc/leff_dwconv_dz.hip), which forms dz itself.  Minimum and spread
(max - min) over 3 rounds of 10 calls.  A width enters fused.LEFF_BWD_DZ_C only if it wins on every map size by more than the spread.
    python tools/bench_leff_bwd_dz.py                              (DHZ_DWZ_PLAIN_ORDER=1: without the XCD renumbering)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd"), ROOT]
import torch
from dehaze_hip import _lib, ops
from dehaze_hip.train import FlatAdamW
dev = torch.device("cuda:0")
s = torch.cuda.current_stream().cuda_stream
BS = 32


def timeit(f, n=10, rounds=3):
    for _ in range(3): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / n * 1e3)
    return min(ts), max(ts) - min(ts)


# (C, map side) of the LeWin levels: encoder 32@128 64@64 128@32 256@16, bottleneck 512@8, decoder 512@16 256@32 128@64 64@128
SHAPES = [(32, 128), (64, 64), (128, 32), (256, 16), (512, 8), (512, 16), (256, 32), (128, 64), (64, 128)]
lins = torch.nn.ModuleList([torch.nn.Linear(4 * C, C) for C in sorted({c for c, _ in SHAPES})]).to(dev)
opt = FlatAdamW(lins)
opt.zero_grad()
opt.enable_split_shadow()
byC = {lin.out_features: lin.weight for lin in lins}
print(f"{'C':>4} {'map':>4} | {'dz GEMM':>8} {'dw bwd':>8} {'chain':>8} (+-) | {'dz in kernel':>12} (+-) | gain us   MB moved  TB/s")
tot = {}
for C, res in SHAPES:
    Ch, T = 4 * C, BS * res * res
    W = byC[C].detach()
    dy = torch.randn(T, C, device=dev)
    u = torch.randn(T, Ch, device=dev); tp = torch.rand(T, Ch, device=dev); du = torch.empty_like(u)
    wd = torch.randn(Ch, 9, device=dev) * 0.3
    dw = torch.zeros(Ch * 9, device=dev); db = torch.zeros(Ch, device=dev)
    sc = torch.ones(BS, device=dev)
    dz0 = ops.gemm_dgrad(dy, W)

    def dwb(dz):
        _lib.call("dhz_leff_dwconv_bwd_scaled_dt", dz.data_ptr(), u.data_ptr(), tp.data_ptr(), wd.data_ptr(), du.data_ptr(), dw.data_ptr(),
                  db.data_ptr(), sc.data_ptr(), BS, res, res, Ch, 0, s)
    t_g, _ = timeit(lambda: ops.gemm_dgrad(dy, W))
    t_d, _ = timeit(lambda: dwb(dz0))
    t_c, s_c = timeit(lambda: dwb(ops.gemm_dgrad(dy, W)))
    if C > 128:
        print(f"{C:4d} {res:4d} | {t_g:8.1f} {t_d:8.1f} {t_c:8.1f} {s_c:4.1f} | {'(no instance)':>12}")
        continue
    pl = ops.split_planes_t(byC[C])
    assert pl is not None
    t_n, s_n = timeit(lambda: _lib.call("dhz_leff_dwconv_bwd_dy", dy.data_ptr(), C, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(),
                                        u.data_ptr(), tp.data_ptr(), wd.data_ptr(), du.data_ptr(), dw.data_ptr(), db.data_ptr(), sc.data_ptr(),
                                        BS, res, res, C, Ch, s))
    mb = (3 * T * Ch + T * C) * 4 / 1e6                       # u, tpre, du and dy once
    win = t_c - t_n > max(s_c, s_n)
    tot[C] = tot.get(C, True) and win
    print(f"{C:4d} {res:4d} | {t_g:8.1f} {t_d:8.1f} {t_c:8.1f} {s_c:4.1f} | {t_n:12.1f} {s_n:4.1f} | {t_c - t_n:7.1f}  {mb:8.1f}  {mb / t_n:5.2f}"
          f"  {'win' if win else 'no'}")
print("widths that win on every map size:", sorted(c for c, w in tot.items() if w))
