#!/usr/bin/env python3
"""Golden vectors for 4 x 4 windows: two LeWin blocks of the REFERENCE, by the recipe of the block fixtures of gen_golden.py (whose
shims and helpers this script uses).  Run by hand where the reference is mounted; no test runs it.

  block_m1_c64_win4_shift2   dim 64, 2 heads, 16 x 16 map, win_size 4, shift_size 2: sixteen shifted 4 x 4 windows per image
  block_m1_c64_res4_clamp    dim 64, 2 heads,  4 x 4 map,  win_size 8, shift_size 4: the clamp of M1:764-766 makes it ONE 4 x 4 window
                             without shift and a [49, 2] bias table - the bottleneck block of a 64-pixel model

usage:  python tests/golden/gen_golden_win4.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import torch  # noqa: E402

CASES = {   # name -> (map side, win_size, shift_size, model seed, data seed, sample seed)
    "block_m1_c64_win4_shift2": (16, 4, 2, 31, 8, 81),
    "block_m1_c64_res4_clamp": (4, 8, 4, 37, 9, 82),
}


def gen_block(M1, name):
    res, win, shift, mseed, dseed, iseed = CASES[name]
    G.seed_all(mseed)
    blk = M1.LeWinTransformerBlock(dim=64, input_resolution=(res, res), num_heads=2, win_size=win, shift_size=shift,
                                   token_mlp='leff', drop_path=0.)
    L = blk.win_size * blk.win_size
    if name.endswith("clamp"):
        assert (blk.win_size, blk.shift_size) == (4, 0) and tuple(blk.attn.relative_position_bias_table.shape) == (49, 2)
    # non-trivial LN affine + biases so that every parameter matters
    g = torch.Generator().manual_seed(dseed)
    with torch.no_grad():
        for p in blk.parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn(2, res * res, 64, generator=g).requires_grad_()
    gout = torch.randn(2, res * res, 64, generator=g)
    torch.manual_seed(iseed)
    idx = torch.randint(L, (L, 15))                   # the draw of ATT:91 for L_Q = L_K = 16: u = 5 ceil(ln 16) = 15
    torch.manual_seed(iseed)                          # the reference draws it itself from the global CPU generator
    y = blk(x)
    (y * gout).sum().backward()
    G.npz(name, x=x, gout=gout, idx=idx.to(torch.int8), y=y, dx=x.grad, **G.sd_arrays(blk), **G.grad_arrays(blk))


def main():
    G.install_shims()
    import warnings
    warnings.simplefilter("ignore")
    import My_model_1 as M1
    for name in CASES:
        gen_block(M1, name)


if __name__ == "__main__":
    main()
