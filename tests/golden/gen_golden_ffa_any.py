#!/usr/bin/env python3
"""Golden vectors for FFA-Net of the REFERENCE on a map whose sides are no multiples of 16 (the whole-image use of FFA_model/test.py).
Run by hand where the reference is mounted; no test runs it.  Recipe, seeds and gate scaling are gen_golden_ffa.py's, imported from it.

  ffa_any   seed 41, FFA(gps=3, blocks=2), gates times GATE_SCALE; x, gout at 2 x 3 x 38 x 52 (seed 42): y = FFA(x), per-parameter
            gradient norms of (y * gout).sum(), 32 gradient entries per parameter at positions seeded 43, and the gradient of the image
            dx.  No weights: they follow from the seed.

usage:  python tests/golden/gen_golden_ffa_any.py
"""
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402
import gen_golden_ffa as F  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPE = (2, 3, 38, 52)


def main():
    spec = importlib.util.spec_from_file_location("ref_ffa", F.FFA_PY)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    G.seed_all(F.MODEL_SEED)
    net = ref.FFA(gps=3, blocks=2)
    names = [n for n, _ in net.named_parameters()]
    shapes = [tuple(p.shape) for _, p in net.named_parameters()]
    F.scale_gates(net)
    g = torch.Generator().manual_seed(F.DATA_SEED)
    x = torch.rand(*SHAPE, generator=g)
    gout = torch.randn(*SHAPE, generator=g)
    xr = x.clone().requires_grad_()
    y = net(xr)
    (y * gout).sum().backward()
    pos = F.sample_positions(list(zip(names, shapes)))
    gnorm = np.array([p.grad.double().norm().item() for p in net.parameters()], dtype=np.float64)
    gsamp = np.stack([p.grad.reshape(-1)[pos[n]].double().numpy() for n, p in net.named_parameters()])
    G.npz("ffa_any", names=np.array(names), x=x, gout=gout, y=y.detach(), grad_norm=gnorm, grad_samples=gsamp, dx=xr.grad)


if __name__ == "__main__":
    main()
