"""The noise-robustness half of the reference's "how do ViTs work" argument ("Convs are vulnerable to high-frequency noise, MSAs to
low-frequency noise"; ops/adversarial.py: Random, FreqAttack) for the dehazing models on MI355X: perturb the hazy input with sign noise
restricted to one frequency band at a time, restore it, and score the result against the ground truth.  No plots are made.

  python My_robustness.py --arch Uformer --embed_dim 32 --weights model_best.pth --input_dir <dir with gt/ hazy/> --out logs/probsparse
  python My_robustness.py --attention dense --weights dense_best.pth --input_dir <dir with gt/ hazy/> --out logs/dense
  python My_robustness.py --arch UNet --weights unet_best.pth --input_dir <dir with gt/ hazy/> --out logs/unet
  python My_robustness.py --synthetic 4 --batch_size 2 --train_ps 128 --arch Uformer --bands 3          # synthetic haze, no files needed

--input_dir reads the .png / .jpg / .jpeg files of <dir>/hazy and the files of the same names in <dir>/gt: square images of one size
whose side the model takes.  Per batch ONE draw r = randn (a generator of the script's own, seeded from --seed) serves every band:
x_adv = hazy + eps * band_f(sign(r)), band centres f = linspace(0, pi, --bands), half-width --s (dehaze_hip.freq_noise: the float64 HIP
kernel; DHZ_FREQ_NOISE=0 takes the reference's ATen formula instead).  Everything runs under eval() and no_grad(); every pass scores
clamp(model(x), 0, 1) against gt on the device (metrics.Scores.add_uniform) and reads the scores back once.
PREFIX_robustness.csv, with a header line: band, f, w1, w2, images, psnr, ssim, d_psnr, d_ssim - one row `clean` (f, w1, w2 empty), then
one row per band; psnr / ssim are means over the images, the deltas are against the clean row.
"""
import argparse
import csv
import math
import os
import sys

dir_name = os.path.dirname(os.path.abspath(__file__))
if dir_name not in sys.path:
    sys.path.insert(0, dir_name)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import utils  # noqa: E402
from dehaze_hip import freq_noise  # noqa: E402
from dehaze_hip.metrics import Scores  # noqa: E402
from dehaze_hip.train import synthetic_batch  # noqa: E402


IMAGE_EXTS = (".png", ".jpg", ".jpeg")
UFORMERS = ("Uformer", "Uformer16", "Uformer32")
HEADER = ["band", "f", "w1", "w2", "images", "psnr", "ssim", "d_psnr", "d_ssim"]


def build_model(opt):
    if opt.attention == "dense":
        if opt.arch not in UFORMERS:
            raise SystemExit(f"--attention dense is the twin of the Uformer (My_model.Uformer), not of --arch {opt.arch}")
        import My_model
        if opt.arch == "Uformer":
            return My_model.Uformer(img_size=opt.train_ps, embed_dim=opt.embed_dim, win_size=opt.win_size, token_projection="linear",
                                    token_mlp=opt.token_mlp)
        return My_model.Uformer(img_size=opt.train_ps, embed_dim=int(opt.arch[-2:]), win_size=8, token_projection="linear", token_mlp="leff")
    if opt.arch not in UFORMERS + ("UNet", "FFA"):
        raise SystemExit(f"--arch {opt.arch}: Uformer, Uformer16, Uformer32, UNet or FFA")
    return utils.get_arch(opt)


def side_multiple(opt):
    """the side the model takes.  Uformer: four 2x down-samplings, then whole windows at the bottleneck (a window larger than the bottleneck
    of the construction size shrinks to it, M1:764-766); UNet: four 2x poolings; FFA: any side - the band filter needs an even one"""
    if opt.arch == "UNet":
        return 16
    if opt.arch == "FFA":
        return 2
    win = opt.win_size if opt.arch == "Uformer" else 8
    return 16 * min(win, max(1, opt.train_ps // 16))


def _images(folder, names, mult, first):
    imgs = []
    for f in names:
        img = torch.from_numpy(utils.load_img(os.path.join(folder, f))).permute(2, 0, 1)
        H, W = img.shape[1:]
        if H != W or H % mult:
            raise SystemExit(f"{os.path.join(folder, f)}: {H} x {W} - the experiment takes square images whose side is a multiple of {mult} "
                             "(the padded any-size route is out of its scope); crop or resize first")
        if H != first[0]:
            if first[0]:
                raise SystemExit(f"{os.path.join(folder, f)}: side {H}, the images before it {first[0]} - one run scores images of one size")
            first[0] = H
        imgs.append(img)
    return torch.stack(imgs)


def folders(opt):
    """(gt directory, hazy directory, the image names both hold, sorted), or SystemExit naming what is missing"""
    gt, hazy = os.path.join(opt.input_dir, "gt"), os.path.join(opt.input_dir, "hazy")
    for d, name in ((gt, "gt/"), (hazy, "hazy/")):
        if not os.path.isdir(d):
            raise SystemExit(f"--input_dir {opt.input_dir}: no {name} directory in it")
    files = sorted(f for f in os.listdir(hazy) if f.lower().endswith(IMAGE_EXTS))
    if not files:
        raise SystemExit(f"{hazy}: no images ({', '.join(IMAGE_EXTS)})")
    missing = [f for f in files if not os.path.isfile(os.path.join(gt, f))]
    if missing:
        raise SystemExit(f"{gt}: no ground truth for {missing[0]} ({len(missing)} of {len(files)} hazy images have none)")
    return gt, hazy, files


def batches(opt, dev):
    """(gt, hazy) batches on dev, [B, 3, n, n] fp32 in [0, 1]"""
    mult = side_multiple(opt)
    if opt.synthetic:
        if opt.train_ps % mult:
            raise SystemExit(f"--train_ps {opt.train_ps} is no multiple of {mult}, which this model takes")
        for i in range(0, opt.synthetic, opt.batch_size):
            yield synthetic_batch(min(opt.batch_size, opt.synthetic - i), opt.train_ps, seed=opt.seed + i, device=dev)
        return
    gt, hazy, files = folders(opt)
    first = [0]
    for i in range(0, len(files), opt.batch_size):
        names = files[i:i + opt.batch_size]
        yield _images(gt, names, mult, first).to(dev), _images(hazy, names, mult, first).to(dev)


def write_csv(prefix, rows):
    """PREFIX_robustness.csv: the header, then the rows (dicts keyed by HEADER; floats written with repr).  Returns the path."""
    path = prefix + "_robustness.csv"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(HEADER)
        for r in rows:
            w.writerow([repr(v) if isinstance(v, float) else v for v in (r[k] for k in HEADER)])
    return path


def main(argv=None):
    p = argparse.ArgumentParser(description="robustness of the dehazing models against frequency-band noise")
    p.add_argument("--arch", type=str, default="Uformer", help="Uformer (with --embed_dim / --win_size / --token_mlp), Uformer16, Uformer32, UNet, FFA")
    p.add_argument("--embed_dim", type=int, default=32)
    p.add_argument("--win_size", type=int, default=8)
    p.add_argument("--token_projection", type=str, default="linear")
    p.add_argument("--token_mlp", type=str, default="leff", help="ffn / leff")
    p.add_argument("--ffa_blocks", type=int, default=19, help="blocks per group of --arch FFA")
    p.add_argument("--train_ps", type=int, default=128, help="the size the model is constructed for")
    p.add_argument("--weights", type=str, default="", help="checkpoint to test (none: the initial weights)")
    p.add_argument("--attention", choices=("probsparse", "dense"), default="probsparse", help="My_model_1.Uformer or its dense twin My_model.Uformer")
    p.add_argument("--input_dir", type=str, default="", help="directory with gt/ and hazy/")
    p.add_argument("--synthetic", type=int, default=0, help="test N synthetic haze pairs instead of --input_dir")
    p.add_argument("--batch_size", type=int, default=4)
    p.add_argument("--bands", type=int, default=11, help="band centres f = linspace(0, pi, bands)")
    p.add_argument("--s", type=float, default=0.2, help="half-width of a band, radians")
    p.add_argument("--eps", type=float, default=0.007, help="size of the sign noise before the band filter")
    p.add_argument("--out", type=str, default="robustness", help="PREFIX of PREFIX_robustness.csv")
    p.add_argument("--seed", type=int, default=1234)
    opt = p.parse_args(argv)
    if bool(opt.synthetic) == bool(opt.input_dir):
        raise SystemExit("give --input_dir <dir with gt/ and hazy/> or --synthetic N (one of them)")
    if opt.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    if opt.bands < 1:
        raise SystemExit("--bands must be >= 1")
    if opt.synthetic and opt.train_ps % side_multiple(opt):
        raise SystemExit(f"--train_ps {opt.train_ps} is no multiple of {side_multiple(opt)}, which this model takes")
    if opt.input_dir:
        folders(opt)                                 # refused before the device is touched
    dev = torch.device("cuda", 0)
    torch.manual_seed(opt.seed)

    model = build_model(opt).to(dev)
    if opt.weights:
        utils.load_checkpoint(model, opt.weights)
    model.eval()
    centres = np.linspace(0.0, math.pi, opt.bands).tolist()
    gen = torch.Generator().manual_seed(opt.seed)
    scores = [Scores() for _ in range(1 + opt.bands)]
    widths = None

    def restore(x, i):
        torch.manual_seed(opt.seed + i)              # the ProbSparse blocks sample their keys from the global generator: every pass sees
        return model(x).clamp(0, 1)                  # the sampling the clean pass saw

    with torch.no_grad():
        for i, (gt, hazy) in enumerate(batches(opt, dev)):
            n = hazy.shape[-1]
            if widths is None:
                widths = [freq_noise.band_widths(f, opt.s, n) for f in centres]
            draw = torch.randn(hazy.shape, generator=gen).to(dev)                                       # once per batch, for every band
            scores[0].add_uniform(restore(hazy, i), gt)
            for b, (w1, w2) in enumerate(widths):
                x_adv = freq_noise.band_noise(hazy, draw, w1, w2, scale=opt.eps, take_sign=True)
                scores[1 + b].add_uniform(restore(x_adv, i), gt)

    rows = []
    labels = [("clean", "", "", "")] + [(b, f, w1, w2) for b, (f, (w1, w2)) in enumerate(zip(centres, widths))]
    for (band, f, w1, w2), sc in zip(labels, scores):
        ssims, psnrs = sc.read()                     # one read-back per pass
        row = dict(band=band, f=f, w1=w1, w2=w2, images=len(psnrs), psnr=sum(psnrs) / len(psnrs), ssim=sum(ssims) / len(ssims))
        clean = rows[0] if rows else row
        row["d_psnr"], row["d_ssim"] = row["psnr"] - clean["psnr"], row["ssim"] - clean["ssim"]
        rows.append(row)
    path = write_csv(opt.out, rows)
    print("saved", path)
    return path


if __name__ == "__main__":
    main()
