#!/usr/bin/env python
"""Golden vectors for the validation metrics of FFA-Net's recipe: `ssim` / `psnr` of the REFERENCE's FFA_model/metrics.py.  Run by hand
where the reference is mounted; no test runs it.  The file is loaded by path; it imports torchvision.transforms.ToPILImage, which it never
uses and which need not be installed, so a stub module stands in for it.

For three fp32 pairs the file stores the inputs, the reference's ssim (size_average True and False) and psnr on the fp32 inputs, and the
same functions on the inputs cast to float64: `window.type_as(img1)` (metrics.py:57) makes that the float64 evaluation of the formula with
the fp32-built window - the oracle of the device kernel.
  noise    2 x 3 x 33 x 47   seeded U[0,1) against itself + 0.1 N(0,1)
  smooth   2 x 3 x 33 x 47   products of sines against an affine map of itself + 0.01 N(0,1)
  range    1 x 3 x 5 x 9     values in [-0.2, 1.3]: pins the clamp, on a plane smaller than the window both ways
A near-constant pair is left out on purpose: on it the reference's fp32 value is 4e-5 off its own float64 value, which would only pin
ATen's rounding.

usage:  python tests/golden/gen_golden_metrics.py
"""
import importlib.util
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRICS_PY = os.path.join(os.path.dirname(G.REF), "FFA_how-do-vits-work-transformer", "FFA_model", "metrics.py")
SEED = 51


def pairs():
    g = torch.Generator().manual_seed(SEED)
    out = {}
    a = torch.rand(2, 3, 33, 47, generator=g)
    out["noise"] = (a + 0.1 * torch.randn(a.shape, generator=g), a)
    yy, xx = torch.meshgrid(torch.arange(33.0), torch.arange(47.0), indexing="ij")
    ph = torch.arange(6.0).view(2, 3, 1, 1)
    s = 0.5 + 0.45 * torch.sin(0.21 * yy + ph) * torch.sin(0.13 * xx + 0.5 * ph)
    out["smooth"] = ((0.9 * s + 0.05 + 0.01 * torch.randn(s.shape, generator=g)).float(), s.float())
    r = -0.2 + 1.5 * torch.rand(1, 3, 5, 9, generator=g)
    out["range"] = ((r + 0.2 * torch.randn(r.shape, generator=g)).clamp(-0.2, 1.3), r)
    return out


def main():
    if "torchvision" not in sys.modules:
        tv, tf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
        tf.ToPILImage = object
        tv.transforms = tf
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tf
    spec = importlib.util.spec_from_file_location("ref_metrics", METRICS_PY)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    blob = {"window": ref.create_window(11, 1)[0, 0].numpy()}
    for name, (pred, gt) in pairs().items():
        blob[name + "_pred"], blob[name + "_gt"] = pred.numpy(), gt.numpy()
        for tag, cast in (("f32", torch.float32), ("f64", torch.float64)):
            p, t = pred.to(cast), gt.to(cast)
            blob[f"{name}_ssim_{tag}"] = np.float64(ref.ssim(p, t).item())
            blob[f"{name}_ssim_per_image_{tag}"] = ref.ssim(p, t, size_average=False).double().numpy()
            blob[f"{name}_psnr_{tag}"] = np.float64(ref.psnr(p, t))
    path = os.path.join(G.HERE, "ffa_metrics.npz")
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path), "bytes")
    for k, v in blob.items():
        if "ssim_f" in k or "psnr" in k:
            print(k, v)


if __name__ == "__main__":
    main()
