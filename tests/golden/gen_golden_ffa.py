#!/usr/bin/env python3
"""Golden vectors for FFA-Net (FFA_model/models/FFA.py:9-110) of the REFERENCE.  Run by hand where the reference is mounted; no test
runs it.  The reference's FFA.py is loaded by file path, so the surrounding package's __init__ and its imports are not pulled in.

  ffa_blocks2   seed 41, FFA(gps=3, blocks=2): parameter names, shapes, per-parameter (mean, std, abs-max) of the UNSCALED init.  Then
                every parameter under a `ca` or `pa` submodule is multiplied by GATE_SCALE (scale_gates below; the tests apply the same),
                and x, gout at 2 x 3 x 32 x 48 (seed 42), y = FFA(x), per-parameter gradient norms of (y * gout).sum() and 32 gradient
                entries per parameter at positions seeded 43 are recorded.  No weights: they follow from the seed.

GATE_SCALE = 4: at the default initialisation the gates of this input stay within 0.35 - 0.63 (channel) and 0.40 - 0.66 (pixel), where a
mis-indexed gate would hardly show.  With every gate parameter times 4 the reference's channel gates span 0.022 - 0.973 and its pixel gates
0.063 - 0.9999 on the fixture input (measured on the CPU over all seven channel and seven pixel gates); times 8 they saturate (1e-5 - 1.0).

usage:  python tests/golden/gen_golden_ffa.py
"""
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODEL_SEED, DATA_SEED, POS_SEED, NPOS = 41, 42, 43, 32
GATE_SCALE = 4.0
SHAPE = (2, 3, 32, 48)
FFA_PY = os.path.join(os.path.dirname(G.REF), "FFA_how-do-vits-work-transformer", "FFA_model", "models", "FFA.py")


def scale_gates(net, k=GATE_SCALE):
    """multiply every parameter of a channel-attention (`ca`) or pixel-attention (`pa`) Sequential by k, in place"""
    with torch.no_grad():
        for n, p in net.named_parameters():
            if {"ca", "pa"} & set(n.split(".")):
                p.mul_(k)
    return net


def sample_positions(named_shapes):
    """{name: 32 flat indices}, from one generator in registration order - the test draws the same"""
    g = torch.Generator().manual_seed(POS_SEED)
    return {n: torch.randint(int(np.prod(s)), (NPOS,), generator=g) for n, s in named_shapes}


def main():
    spec = importlib.util.spec_from_file_location("ref_ffa", FFA_PY)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    G.seed_all(MODEL_SEED)
    net = ref.FFA(gps=3, blocks=2)
    names = [n for n, _ in net.named_parameters()]
    shapes = [tuple(p.shape) for _, p in net.named_parameters()]
    stats = np.array([[p.mean().item(), p.std().item(), p.abs().max().item()] for p in net.parameters()], dtype=np.float64)
    scale_gates(net)
    g = torch.Generator().manual_seed(DATA_SEED)
    x = torch.rand(*SHAPE, generator=g)
    gout = torch.randn(*SHAPE, generator=g)
    y = net(x)
    (y * gout).sum().backward()
    pos = sample_positions(list(zip(names, shapes)))
    gnorm = np.array([p.grad.double().norm().item() for p in net.parameters()], dtype=np.float64)
    gsamp = np.stack([p.grad.reshape(-1)[pos[n]].double().numpy() for n, p in net.named_parameters()])
    G.npz("ffa_blocks2", names=np.array(names), shapes=np.array([",".join(map(str, s)) for s in shapes]), init_stats=stats,
          x=x, gout=gout, y=y.detach(), grad_norm=gnorm, grad_samples=gsamp)


if __name__ == "__main__":
    main()
