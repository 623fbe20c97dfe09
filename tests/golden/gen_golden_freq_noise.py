#!/usr/bin/env python
"""Golden vectors for the frequency-band noise: the REFERENCE's how-do-vits-work-transformer/ops/adversarial.py, FreqAttack(Random(eps), f, s)
on CPU tensors in fp32, as the reference runs it.  Run by hand where the reference is mounted; no test runs it.  The module is loaded by
path.

Cases: sides n = 8 (some bands are empty, w1 reaches n), 16 and 34 (n / 2 odd, no multiple of 4), each [B, C] = [2, 3] (the reference's mask
has 3 channels).  Per side, under the seed SEED + n:
  n<n>_seed      the seed: torch.manual_seed(seed) before the attack, so that Random's draw (CPU, global generator) is the first thing drawn
  n<n>_x         the fp32 input, rand in [0, 1)
  n<n>_draw      the draw torch.randn([2, 3, n, n]) under that seed
  n<n>_w         [11, 2] int32: (w1, w2) = clip(int((f +- s) n / (2 pi)) * 2, 0, n) per band centre, restated from adversarial.py:148-149
                 and _center_mask's clamps; this script ASSERTS that the reference's own mask has exactly these widths
  n<n>_x_adv     [11, 2, 3, n, n] fp32: the reference's x_adv per band centre
and once: eps, s, fs = linspace(0, pi, 11) (float64).

usage:  python tests/golden/gen_golden_freq_noise.py
"""
import importlib.util
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF_PY = os.path.join(os.path.dirname(G.REF), "how-do-vits-work-transformer", "ops", "adversarial.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "freq_noise.npz")
SEED = 180
EPS, S, BANDS = 0.007, 0.2, 11
SIDES = (8, 16, 34)


def main():
    spec = importlib.util.spec_from_file_location("ref_adversarial", REF_PY)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    fs = np.linspace(0.0, math.pi, BANDS)
    out = dict(eps=np.float64(EPS), s=np.float64(S), fs=fs)
    for n in SIDES:
        seed = SEED + n
        x = torch.rand(2, 3, n, n, generator=torch.Generator().manual_seed(seed))
        ys = torch.zeros(2)
        torch.manual_seed(seed)
        draw = torch.randn([2, 3, n, n])
        widths, advs = [], []
        for f in fs:
            f = float(f)
            attack = ref.FreqAttack(ref.Random(eps=EPS, gpu=False), f=f, s=S)
            torch.manual_seed(seed)
            x_adv, _ = attack(x, ys)
            assert x_adv.dtype == torch.float32 and x_adv.shape == x.shape
            w = [min(max(int(((c) * n) / (2 * math.pi)) * 2, 0), n) for c in (f + S, f - S)]
            m1 = attack._center_mask(int(((f + S) * n) / (2 * math.pi)) * 2, n)
            m2 = attack._center_mask(int(((f - S) * n) / (2 * math.pi)) * 2, n)
            for m, wi in ((m1, w[0]), (m2, w[1])):                 # a centred square of side wi, rows / columns (n - wi) / 2 .. (n + wi) / 2 - 1
                want = torch.zeros(n, n)
                want[(n - wi) // 2:(n + wi) // 2, (n - wi) // 2:(n + wi) // 2] = 1
                assert m.shape == (1, 3, n, n) and all(torch.equal(m[0, c], want) for c in range(3)), (n, f, wi)
            widths.append(w)
            advs.append(x_adv.numpy())
        torch.manual_seed(seed)
        plain, _ = ref.Random(eps=EPS, gpu=False)(x, ys)             # the draw stored is the draw the attack used
        assert torch.equal(plain, x + EPS * draw.sign())
        out[f"n{n}_seed"] = np.int64(seed)
        out[f"n{n}_x"] = x.numpy()
        out[f"n{n}_draw"] = draw.numpy()
        out[f"n{n}_w"] = np.asarray(widths, dtype=np.int32)
        out[f"n{n}_x_adv"] = np.stack(advs)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
