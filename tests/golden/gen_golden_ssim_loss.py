#!/usr/bin/env python
"""Golden vectors for SSIM as a training loss: value and gradient d ssim / d img1 of the REFERENCE's two differentiable SSIM functions,
FFA_model/metrics.py `ssim` (zero padding, inputs clamped; rule "ffa") and Uformer_ProbSparse/aaa.py `ssim(..., val_range=1)` (no padding,
no clamp; rule "aaa").  Run by hand where the reference is mounted; no test runs it.  Both files are loaded by path (metrics.py imports
torchvision.transforms.ToPILImage, which it never uses: a stub stands in, as in gen_golden_metrics.py).

Per case and rule the file stores
  <case>_pred, <case>_gt            the fp32 inputs (img1 = pred)
  <case>_<rule>_ssim_f64 / _f32     the value by the reference function on the inputs cast to float64 (with the fp32-built window cast to
                                    float64: the float64 evaluation of the formula) / on the fp32 inputs
  <case>_<rule>_grad                the float64 gradient by autograd of the float64 evaluation, ROUNDED TO fp32 for storage (the float64
                                    arrays of all cases would pass the size limit of a committed file; a test adds 2^-24 max|grad| for it)
  <case>_<rule>_grad_err_f32        max |gradient of the reference's own fp32 evaluation - float64 gradient|: the reference's own error,
                                    the yardstick of the tests' bounds (the fp32 gradient array itself is not stored, for the same reason)
Cases (seeded):
  noise, smooth, range   the three pairs of ffa_metrics.npz (gen_golden_metrics.pairs()); `noise` has 8.5 % of its elements clamped, `range`
                         is a 5 x 9 plane, smaller than the window both ways, with 37 % clamped
  two_tiles              2 x 3 x 70 x 130: more than one tile each way for any tile up to 64 x 128, plus a remainder; an 8-bit image against
                         itself + noise on a 1/1024 grid (compresses well), ~1 % of the predictions exactly at 0.0 and at 1.0, ~4 % outside
  one_pixel              1 x 1 x 11 x 11: under "aaa" the map is a single pixel
  thin                   1 x 3 x 12 x 21
"ffa": noise, smooth, range, two_tiles.  "aaa": noise, two_tiles, one_pixel, thin (`range` is smaller than the 11 x 11 window).

usage:  python tests/golden/gen_golden_ssim_loss.py
"""
import importlib.util
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402
import gen_golden_metrics as GM  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

AAA_PY = os.path.join(G.REF, "aaa.py")
SEED = 52
FFA_CASES = ("noise", "smooth", "range", "two_tiles")
AAA_CASES = ("noise", "two_tiles", "one_pixel", "thin")


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    out = dict(GM.pairs())
    g = torch.Generator().manual_seed(SEED)
    gt = torch.randint(0, 256, (2, 3, 70, 130), generator=g).float() / 255
    pred = torch.round((gt + 0.05 * torch.randn(gt.shape, generator=g)) * 1024) / 1024
    u = torch.rand(gt.shape, generator=g)
    pred = torch.where(u < 0.01, torch.zeros_like(pred), pred)            # exactly at the inclusive clamp bounds
    pred = torch.where(u > 0.99, torch.ones_like(pred), pred)
    out["two_tiles"] = (pred, gt)
    for name, shape in (("one_pixel", (1, 1, 11, 11)), ("thin", (1, 3, 12, 21))):
        a = torch.rand(shape, generator=g)
        out[name] = (a + 0.1 * torch.randn(shape, generator=g), a)
    return out


def value_and_grad(fn, pred, gt):
    p = pred.clone().requires_grad_(True)
    v = fn(p, gt)
    g, = torch.autograd.grad(v, p)
    return v.item(), g


def main():
    if "torchvision" not in sys.modules:
        tv, tf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tf.ToPILImage = object
        tv.transforms = tf
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tf
    ffa = load(GM.METRICS_PY, "ref_metrics")
    aaa = load(AAA_PY, "ref_aaa")

    def aaa_ssim(a, b):          # the window the function would build (aaa.py:44-46), in the inputs' dtype: float64 inputs need it passed in
        return aaa.ssim(a, b, window=aaa.create_window(11, channel=a.shape[1]).to(a.dtype), val_range=1)

    blob = {"window": ffa.create_window(11, 1)[0, 0].numpy()}
    assert np.array_equal(blob["window"], aaa.create_window(11)[0, 0].numpy())
    all_cases = cases()
    for rule, fn, names in (("ffa", ffa.ssim, FFA_CASES), ("aaa", aaa_ssim, AAA_CASES)):
        for name in names:
            pred, gt = all_cases[name]
            blob[name + "_pred"], blob[name + "_gt"] = pred.numpy(), gt.numpy()
            v64, g64 = value_and_grad(fn, pred.double(), gt.double())
            v32, g32 = value_and_grad(fn, pred, gt)
            key = f"{name}_{rule}"
            blob[key + "_ssim_f64"], blob[key + "_ssim_f32"] = np.float64(v64), np.float64(v32)
            blob[key + "_grad"] = g64.float().numpy()
            blob[key + "_grad_err_f32"] = np.float64((g32.double() - g64).abs().max().item())
            print(f"{key:18s} {tuple(pred.shape)!s:18s} ssim {v64:.12f}  |f32 - f64| {abs(v32 - v64):.2e}  max|grad| {g64.abs().max():.3e}  "
                  f"grad err f32 {blob[key + '_grad_err_f32']:.2e} ({blob[key + '_grad_err_f32'] / g64.abs().max().item():.1e} of max)  "
                  f"outside [0,1] {((pred < 0) | (pred > 1)).float().mean().item():.3f}  at bounds "
                  f"{((pred == 0) | (pred == 1)).float().mean().item():.3f}")
    path = os.path.join(G.HERE, "ssim_loss.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
