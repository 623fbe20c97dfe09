#!/usr/bin/env python
"""Golden vectors for the total-variation losses: value and gradient of the REFERENCE's Uformer_ProbSparse/losses.py `tv_loss(x)` (beta = 0.5,
reg_coeff = 5; form "beta") and `TVLoss()(x)` (weight 1; form "sq").  Run by hand where the reference is mounted; no test runs it.  The
file is loaded by path.

Per case and form the file stores
  <case>_x                          the fp32 input
  <case>_<form>_f64 / _f32          the value by the reference on the input cast to float64 / on the fp32 input
  <case>_<form>_grad                the float64 gradient by autograd of the float64 evaluation, ROUNDED TO fp32 for storage; on a case with zero
                                    sites under "beta" this is the gradient of the masked formula (below): the reference's is NaN there
  <case>_<form>_grad_err_f32        max |gradient of the reference's own fp32 evaluation - float64 gradient|, over the pixels where both are
                                    finite: the reference's own error, the yardstick of the tests' bounds
and for the cases with zero sites (a site is s = (x[i,j+1] - x[i,j])^2 + (x[i+1,j] - x[i,j])^2, a zero site has s == 0), under "beta":
  <case>_beta_nan_mask              uint8: the pixels where the reference's float64 gradient is NaN (0.5 * 0^-0.5 * 2 * 0 = inf * 0)
The masked formula is the reference's with s^beta replaced by 0, value and gradient, at the sites with s == 0.  This script ASSERTS that
its float64 value is the reference's bit for bit and that its gradient equals the reference's wherever the reference's is finite - what
ties the zero-site rule of dehaze_hip/tv_loss.py to the reference - and that the NaN pixels are exactly the pixels of the zero sites.

Cases (seeded):
  one_site    1 x 1 x 2 x 2     a single site
  row         1 x 3 x 2 x 7     one row of sites
  col         1 x 1 x 7 x 2     one column of sites
  odd         2 x 3 x 33 x 65   no side is a multiple of 4
  two_bands   2 x 3 x 70 x 130  several 64 x 64 bands each way plus a remainder; an 8-bit image plus noise on a 1/1024 grid
  clamped     1 x 3 x 32 x 32   clamp(0.5 + 0.6 randn, 0, 1): what a training step hands the term; at least 50 zero sites
  flat        1 x 1 x 6 x 6     noise with a constant 2 x 2 block: one zero site

usage:  python tests/golden/gen_golden_tv_loss.py
"""
import importlib.util
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

LOSSES_PY = os.path.join(G.REF, "losses.py")
SEED = 61
CLAMPED_SEED = 70            # a stream of its own: 60 zero sites (seeds 60 .. 74 give 36 .. 60; the case wants at least 50)
ZERO_SITE_CASES = ("clamped", "flat")


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    g = torch.Generator().manual_seed(SEED)
    out = {}
    for name, shape in (("one_site", (1, 1, 2, 2)), ("row", (1, 3, 2, 7)), ("col", (1, 1, 7, 2)), ("odd", (2, 3, 33, 65))):
        out[name] = torch.rand(shape, generator=g)
    img = torch.randint(0, 256, (2, 3, 70, 130), generator=g).float() / 255
    out["two_bands"] = torch.round((img + 0.05 * torch.randn(img.shape, generator=g)) * 1024) / 1024
    gc = torch.Generator().manual_seed(CLAMPED_SEED)
    out["clamped"] = torch.clamp(0.5 + 0.6 * torch.randn((1, 3, 32, 32), generator=gc), 0, 1)
    flat = torch.rand((1, 1, 6, 6), generator=g)
    flat[0, 0, 2:4, 3:5] = 0.375
    out["flat"] = flat
    return out


def sites(x):
    dh = x[:, :, :-1, 1:] - x[:, :, :-1, :-1]
    dv = x[:, :, 1:, :-1] - x[:, :, :-1, :-1]
    return dh * dh + dv * dv


def masked_beta(x, beta=0.5, reg_coeff=5):
    s = sites(x)
    zero = s == 0
    p = torch.pow(torch.where(zero, torch.ones_like(s), s), beta)
    return reg_coeff * (torch.sum(torch.where(zero, torch.zeros_like(s), p)) / x.numel())


def value_and_grad(fn, x):
    p = x.clone().requires_grad_(True)
    v = fn(p)
    g, = torch.autograd.grad(v, p)
    return v.item(), g


def main():
    ref = load(LOSSES_PY, "ref_losses")
    forms = (("beta", ref.tv_loss), ("sq", ref.TVLoss()))
    blob = {}
    for name, x in cases().items():
        blob[name + "_x"] = x.numpy()
        zero_sites = int((sites(x.double()) == 0).sum())
        assert (zero_sites > 0) == (name in ZERO_SITE_CASES), (name, zero_sites)
        if name == "clamped":
            assert zero_sites >= 50, zero_sites
        for form, fn in forms:
            key = f"{name}_{form}"
            v64, g64 = value_and_grad(fn, x.double())
            v32, g32 = value_and_grad(fn, x)
            nan = torch.isnan(g64)
            if form == "beta" and zero_sites:
                touched = torch.zeros_like(x, dtype=torch.bool)                  # the three pixels of every zero site
                z = sites(x.double()) == 0
                touched[:, :, :-1, :-1] |= z
                touched[:, :, :-1, 1:] |= z
                touched[:, :, 1:, :-1] |= z
                assert torch.equal(nan, touched), name
                vm, gm = value_and_grad(masked_beta, x.double())
                assert vm == v64 and torch.isfinite(gm).all() and torch.equal(gm[~nan], g64[~nan]), name
                blob[key + "_nan_mask"] = nan.numpy().astype(np.uint8)
                g64 = gm
            else:
                assert not nan.any(), key
            ok = torch.isfinite(g32)
            assert torch.equal(~ok, nan), key
            blob[key + "_f64"], blob[key + "_f32"] = np.float64(v64), np.float64(v32)
            blob[key + "_grad"] = g64.float().numpy()
            err = (g32.double() - g64)[ok].abs().max().item()
            blob[key + "_grad_err_f32"] = np.float64(err)
            print(f"{key:16s} {tuple(x.shape)!s:18s} value {v64:.12f}  |f32 - f64| {abs(v32 - v64):.2e}  max|grad| {g64.abs().max():.3e}  "
                  f"grad err f32 {err:.2e} ({err / g64.abs().max().item():.1e} of max)  zero sites {zero_sites}  NaN pixels {int(nan.sum())}")
    path = os.path.join(G.HERE, "tv_loss.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
