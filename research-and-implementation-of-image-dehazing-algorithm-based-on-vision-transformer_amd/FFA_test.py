"""FFA-Net as it is used: every image of a folder restored in ONE forward at its own size - the counterpart of FFA_model/test.py
(`--task`, `--test_imgs`, the `trained_models/<task>_train_ffa_<gps>_<blocks>.pk` checkpoint, `pred_FFA_<task>/<name>_FFA.png`), on the
HIP kernels.  No padding, no cropping: SOTS-indoor's 620 x 460, or any other size with both sides at least 32, runs the `_any` entries
of dehaze_hip/ffa.py; multiples of 16 run what they always ran.

Differences by design: one process, no DataParallel (checkpoints with or without the `module.` prefix load, utils.load_checkpoint); PNG /
JPEG decode through PIL and utils.load_img, PNGs written by utils.save_img; no matplotlib window per image; `--gt_dir` scores the
restored images with utils/metrics.py (files matched by name, or by the part of the name before the first `_`, the SOTS convention
`1400_1.png` -> `1400.png`); `--normalize` applies the per-channel mean / std of test.py:54 on the device - off by default, because
FFA_main.py trains on unnormalised inputs; `--synthetic N --height H --width W` restores (and scores) N synthetic haze pairs without data.
"""
import argparse
import os
import sys
import time

dir_name = os.path.dirname(os.path.abspath(__file__))
if dir_name not in sys.path:
    sys.path.insert(0, dir_name)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import utils  # noqa: E402
from dehaze_hip.ffa import FFA  # noqa: E402
from utils.metrics import img_as_ubyte, peak_signal_noise_ratio, structural_similarity  # noqa: E402

MEAN, STD = (0.64, 0.6, 0.58), (0.14, 0.15, 0.152)          # test.py:54
IMAGE_EXTS = ('.png', '.jpg', '.jpeg', '.bmp')              # SOTS-indoor is PNG, SOTS-outdoor JPEG hazy with PNG clear images


def is_image(name):
    return name.lower().endswith(IMAGE_EXTS)


def build_parser():
    parser = argparse.ArgumentParser(description="FFA-Net: restore every image of a folder at its own size")
    parser.add_argument('--task', type=str, default='its', help='its or ots')
    parser.add_argument('--test_imgs', type=str, default='test_imgs', help='Test imgs folder')
    parser.add_argument('--weights', type=str, default='', help='.pk / .pth checkpoint (default: trained_models/<task>_train_ffa_<gps>_<blocks>.pk)')
    parser.add_argument('--gps', type=int, default=3, help='residual_groups')
    parser.add_argument('--blocks', type=int, default=19, help='residual_blocks')
    parser.add_argument('--out_dir', type=str, default='', help='where <name>_FFA.png goes (default: pred_FFA_<task>/)')
    parser.add_argument('--gt_dir', type=str, default='', help='clear images: print mean PSNR / SSIM')
    parser.add_argument('--normalize', action='store_true', help='per-channel mean / std of the input as FFA_model/test.py:54')
    parser.add_argument('--synthetic', type=int, default=0, help='restore N synthetic haze pairs instead of --test_imgs')
    parser.add_argument('--height', type=int, default=460)
    parser.add_argument('--width', type=int, default=620)
    return parser


def resolve(args):
    """the defaults that depend on other options"""
    args.weights = args.weights or os.path.join('trained_models', f'{args.task}_train_ffa_{args.gps}_{args.blocks}.pk')
    args.out_dir = args.out_dir or f'pred_FFA_{args.task}/'
    return args


def gt_index(gt_dir):
    """{stem: path} of the clear images of a folder, listed once (of two files with one stem the first in sorted order)"""
    index = {}
    for f in sorted(os.listdir(gt_dir)):
        if is_image(f):
            index.setdefault(os.path.splitext(f)[0], os.path.join(gt_dir, f))
    return index


def find_gt(index, name, gt_dir=''):
    """the clear image of hazy file `name`: the file of the same stem; only if there is none, of the stem before the first `_`"""
    stem = os.path.splitext(name)[0]
    for want in (stem, stem.split('_')[0]):
        if want in index:
            return index[want]
    raise SystemExit(f"FFA_test: no clear image for {name} in {gt_dir}")


def items(args):
    """(name, hazy [3, H, W] float in [0, 1] on the CPU, clear image or None)"""
    if args.synthetic > 0:
        from dehaze_hip.train import synthetic_batch
        for i in range(args.synthetic):
            gt, hazy = synthetic_batch(1, (args.height, args.width), seed=900 + i, device="cpu")
            yield "synthetic_%03d.png" % i, hazy[0], gt[0]
        return
    index = gt_index(args.gt_dir) if args.gt_dir else None
    for name in utils.natsorted([f for f in os.listdir(args.test_imgs) if is_image(f)]):
        hazy = torch.from_numpy(utils.load_img(os.path.join(args.test_imgs, name))).permute(2, 0, 1).contiguous()
        gt = None
        if index is not None:
            gt = torch.from_numpy(utils.load_img(find_gt(index, name, args.gt_dir))).permute(2, 0, 1).contiguous()
        yield name, hazy, gt


def restore(net, hazy, normalize=False):
    """one forward of [3, H, W] at its own size; the output clamped to [0, 1]"""
    x = hazy.unsqueeze(0)
    if normalize:
        mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
        x = (x - mean) / std
    with torch.no_grad():
        return torch.clamp(net(x.contiguous()), 0, 1)[0]


def main(argv=None):
    args = resolve(build_parser().parse_args(argv))
    if not torch.cuda.is_available():
        raise SystemExit("FFA_test.py needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    print("pred_dir:", args.out_dir)
    utils.mkdir(args.out_dir)
    net = FFA(gps=args.gps, blocks=args.blocks)
    utils.load_checkpoint(net, args.weights, map_location="cpu")
    net.to(dev).eval()

    psnrs, ssims, secs = [], [], []
    for name, hazy, gt in items(args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = restore(net, hazy.to(dev), args.normalize)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        out = pred.permute(1, 2, 0).cpu().numpy()
        print(f"{name}: {out.shape[1]} x {out.shape[0]}, {secs[-1] * 1e3:.1f} ms")
        utils.save_img(os.path.join(args.out_dir, os.path.splitext(name)[0] + '_FFA.png'), img_as_ubyte(out))
        if gt is not None:
            ref = gt.permute(1, 2, 0).numpy()
            if ref.shape != out.shape:
                raise SystemExit(f"FFA_test: {name} is {out.shape[1]} x {out.shape[0]}, its clear image {ref.shape[1]} x {ref.shape[0]}")
            psnrs.append(float(peak_signal_noise_ratio(ref, out)))
            ssims.append(float(structural_similarity(ref, out, multichannel=True)))
    if not secs:
        raise SystemExit(f"FFA_test: no image in {args.test_imgs}")
    if psnrs:
        print("PSNR: %f, SSIM: %f over %d image(s)" % (float(np.mean(psnrs)), float(np.mean(ssims)), len(psnrs)))
    steady = secs[1:] if len(secs) > 1 else secs
    print("forward: %.1f ms/image over %d image(s) after warm-up" % (1e3 * sum(steady) / len(steady), len(steady)))
    return (float(np.mean(psnrs)), float(np.mean(ssims))) if psnrs else None


if __name__ == "__main__":
    main()
