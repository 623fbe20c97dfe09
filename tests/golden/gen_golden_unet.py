#!/usr/bin/env python3
"""Golden vectors for the UNet baseline (M1:22-115) of the REFERENCE at dim 32, through gen_golden.py's shims (as gen_golden_win4.py).
Run by hand where the reference is mounted; no test runs it.

  unet_m1_dim32   seed 41: parameter names, shapes, per-parameter (mean, std, abs-max) of the init; x, gout and y = UNet(x) at
                  1 x 3 x 128 x 128; per-parameter gradient norms of (y * gout).sum() and 32 gradient entries per parameter at
                  seeded positions.  No weights: they follow from the seed.

usage:  python tests/golden/gen_golden_unet.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODEL_SEED, DATA_SEED, POS_SEED, NPOS = 41, 42, 43, 32


def sample_positions(named_shapes):
    """{name: 32 flat indices}, from one generator in registration order - the test draws the same"""
    g = torch.Generator().manual_seed(POS_SEED)
    return {n: torch.randint(int(np.prod(s)), (NPOS,), generator=g) for n, s in named_shapes}


def main():
    G.install_shims()
    import warnings
    warnings.simplefilter("ignore")
    import My_model_1 as M1
    G.seed_all(MODEL_SEED)
    net = M1.UNet(dim=32)
    names = [n for n, _ in net.named_parameters()]
    shapes = [tuple(p.shape) for _, p in net.named_parameters()]
    stats = np.array([[p.mean().item(), p.std().item(), p.abs().max().item()] for p in net.parameters()], dtype=np.float64)
    g = torch.Generator().manual_seed(DATA_SEED)
    x = torch.rand(1, 3, 128, 128, generator=g)
    gout = torch.randn(1, 3, 128, 128, generator=g)
    y = net(x)
    (y * gout).sum().backward()
    pos = sample_positions(list(zip(names, shapes)))
    gnorm = np.array([p.grad.double().norm().item() for p in net.parameters()], dtype=np.float64)
    gsamp = np.stack([p.grad.reshape(-1)[pos[n]].double().numpy() for n, p in net.named_parameters()])
    G.npz("unet_m1_dim32", names=np.array(names), shapes=np.array([",".join(map(str, s)) for s in shapes]), init_stats=stats,
          x=x, gout=gout, y=y.detach(), grad_norm=gnorm, grad_samples=gsamp)


if __name__ == "__main__":
    main()
