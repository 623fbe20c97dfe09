#!/usr/bin/env python3
"""The feed for pools of images of any sizes (dhz_crop_augment_pair_ragged) next to the feed it generalises (dhz_crop_augment_pair_rect) on
IDENTICAL uniform data: the same uint8 images, the same (id, r, c, k) per item, outputs compared bit for bit before anything is timed.
  32 crops of 128 x 128 from 256 x 256 patches      4 whole 460 x 620 frames      1 whole 1200 x 1600 frame
Per shape --rounds alternated passes of  rect | ragged | ragged + norm  (and, where the crop is square,  square : dhz_crop_augment_pair on
the rect entry's table); in a pass every launch is timed by its own pair of device events after --warmup launches, and the pass reports
the median launch and the mean over the whole window (first event to last).  Output bytes / time counts the two float32 outputs.  The rect entry's spread from pass to pass is the yardstick: the ragged entry is "no slower" when its
median pass lies within the rect passes' range.
Then the step of FFA_main.py (ffa_train_step, FFA(3, --blocks), 4 x 240 x 240 crops of 256 x 256 patches, L1 only), batch drawn and fed
from PatchStoreHBM and from ImageStoreHBM in alternated passes.  Writes profiles/feed_ragged.txt.

usage:  python tools/bench_feed_ragged.py [--iters 400] [--warmup 20] [--rounds 5] [--steps 20] [--blocks 19] [--out profiles/feed_ragged.txt]
"""
import argparse
import ctypes
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (label, images in the store, H, W, batch, crop or None)
SHAPES = [("32 crops 128 x 128 of 256 x 256", 64, 256, 256, 32, (128, 128)),
          ("4 whole 460 x 620", 8, 460, 620, 4, None),
          ("1 whole 1200 x 1600", 2, 1200, 1600, 1, None)]
NORM = ((0.64, 0.6, 0.58), (0.14, 0.15, 0.152))
NOTE = """reading the lines above: "ragged" is the rect entry's work (same loads, same stores, same value / 255) and is the line the two entries are
compared by.  "ragged + norm" is MORE work than the rect entry does - per hazy value one subtraction and a second correctly rounded fp32
division, which the compiler expands into about ten instructions - so where it comes out above the rect passes
that is the price of the normalisation, not of descriptor loads or 64-bit addresses, which the plain route carries too."""


def median(v):
    return sorted(v)[len(v) // 2]


def timed_launches(fn, warmup, iters):
    """(median ms of one launch, mean ms per launch over the window), every launch between its own two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    each = [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    return median(each), ev[0].elapsed_time(ev[iters]) / iters


def feed_shape(label, N, H, W, n, crop, a, say):
    import dataset
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(H + W)
    gt = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    hazy = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    old = dataset.PatchStoreHBM(gt, hazy, "cuda")
    new = dataset.ImageStoreHBM([(gt[i], hazy[i]) for i in range(N)], "cuda")
    idx = torch.randint(N, (n,), generator=g).tolist()
    np.random.seed(1); random.seed(1)
    c0, n0 = old.batch(idx, crop)
    np.random.seed(1); random.seed(1)
    c1, n1 = new.batch(idx, crop)
    torch.cuda.synchronize()
    assert torch.equal(new._draws, old._table) and torch.equal(c0.view(torch.int32), c1.view(torch.int32)) \
        and torch.equal(n0.view(torch.int32), n1.view(torch.int32)), "the two entries disagree"
    h, w = c0.shape[2:]
    tab_old, tab_new = old._table.cuda(), new._table.cuda()
    norm = (ctypes.c_float * 6)(*(NORM[0] + NORM[1]))
    stream = torch.cuda.current_stream().cuda_stream
    routes = {
        "rect": lambda: _lib.call("dhz_crop_augment_pair_rect", old.gt.data_ptr(), old.hazy.data_ptr(), tab_old.data_ptr(), c0.data_ptr(),
                                  n0.data_ptr(), n, H, W, h, w, stream),
        "ragged": lambda: _lib.call("dhz_crop_augment_pair_ragged", new.gt_pool.data_ptr(), new.hazy_pool.data_ptr(), tab_new.data_ptr(),
                                    c1.data_ptr(), n1.data_ptr(), None, n, h, w, stream),
        "ragged + norm": lambda: _lib.call("dhz_crop_augment_pair_ragged", new.gt_pool.data_ptr(), new.hazy_pool.data_ptr(), tab_new.data_ptr(),
                                           c1.data_ptr(), n1.data_ptr(), norm, n, h, w, stream),
    }
    if h == w:                                               # the square entry reads the rect entry's table
        routes["square"] = lambda: _lib.call("dhz_crop_augment_pair", old.gt.data_ptr(), old.hazy.data_ptr(), tab_old.data_ptr(), c0.data_ptr(),
                                             n0.data_ptr(), n, H, W, h, stream)
    times = {name: [] for name in routes}
    for _ in range(a.rounds):                                # alternated: a drift of the machine hits all routes alike
        for name, fn in routes.items():
            times[name].append(timed_launches(fn, a.warmup, a.iters))
    out_bytes = 2 * n * 3 * h * w * 4
    say(f"{label}: {out_bytes / 1e6:.2f} MB of output per launch")
    for name, ts in times.items():
        med, mean = [t[0] for t in ts], [t[1] for t in ts]
        say(f"  {name:14s} median launch, us  " + " ".join(f"{1e3 * t:8.1f}" for t in med)
            + f"   | median pass {1e3 * median(med):8.1f} us  {out_bytes / median(med) / 1e6:8.1f} GB/s")
        say(f"  {'':14s} window mean,   us  " + " ".join(f"{1e3 * t:8.1f}" for t in mean)
            + f"   | median pass {1e3 * median(mean):8.1f} us  {out_bytes / median(mean) / 1e6:8.1f} GB/s")
    verdicts = []
    for k, what in ((0, "median launch"), (1, "window mean")):
        rect = [t[k] for t in times["rect"]]
        lo, hi = min(rect), max(rect)
        for name in [r for r in routes if r != "rect"]:
            m = median([t[k] for t in times[name]])
            verdicts.append(f"  {label}, {what}: rect passes {1e3 * lo:.1f} .. {1e3 * hi:.1f} us (spread {100 * (hi - lo) / lo:.1f} %), {name} median "
                            f"pass {1e3 * m:.1f} us -> " + ("faster than every rect pass" if m < lo else "within the rect spread" if m <= hi else "SLOWER"))
    return verdicts


def step_time(a, say):
    import dataset
    from dehaze_hip import ffa
    from dehaze_hip.train import FlatAdamW, ffa_train_step
    g = torch.Generator().manual_seed(3)
    gt = torch.randint(0, 256, (16, 256, 256, 3), generator=g, dtype=torch.uint8)
    hazy = (gt.float() * 0.6 + 70).to(torch.uint8)
    stores = {"PatchStoreHBM": dataset.PatchStoreHBM(gt, hazy, "cuda"),
              "ImageStoreHBM": dataset.ImageStoreHBM([(gt[i], hazy[i]) for i in range(16)], "cuda")}
    torch.manual_seed(0)
    model = ffa.FFA(3, a.blocks)
    opt = FlatAdamW(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    model.cuda().train()

    def step(store):
        y, x = store.batch(torch.randint(16, (4,)).tolist(), 240)
        ffa_train_step(model, None, opt, None, x, y)

    times = {name: [] for name in stores}
    for _ in range(a.rounds):
        for name, store in stores.items():
            for _ in range(3):
                step(store)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(store)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    say(f"FFA_main's step (batch draw + feed + ffa_train_step, FFA(3, {a.blocks}), 4 x 240 x 240 of 256 x 256 patches, L1): ms per step, "
        f"{a.rounds} alternated passes of {a.steps} steps after 3")
    for name, ts in times.items():
        say(f"  {name:14s} " + " ".join(f"{t:8.2f}" for t in ts) + f"   | median {median(ts):.2f}, range {min(ts):.2f} .. {max(ts):.2f}")
    old, new = times["PatchStoreHBM"], median(times["ImageStoreHBM"])
    return [f"  step: PatchStoreHBM passes {min(old):.2f} .. {max(old):.2f} ms (spread {100 * (max(old) - min(old)) / min(old):.1f} %), ImageStoreHBM "
            f"median pass {new:.2f} ms -> " + ("faster than every pass" if new < min(old) else "within the spread" if new <= max(old) else "SLOWER")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_ragged.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_feed_ragged.py measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/bench_feed_ragged.py on {torch.cuda.get_device_name(0)}: dhz_crop_augment_pair_rect against dhz_crop_augment_pair_ragged on the same "
        f"uniform data (outputs equal bit for bit); {a.rounds} alternated passes of {a.iters} launches, each launch between its own device events, "
        f"after {a.warmup} launches of warm-up per pass")
    verdicts = []
    for shape in SHAPES:
        verdicts += feed_shape(*shape, a, say)
    verdicts += step_time(a, say)
    say("against the rect entry's own pass-to-pass spread:")
    for v in verdicts:
        say(v)
    say(NOTE)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
