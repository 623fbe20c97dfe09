"""The reference's fourier_analysis.ipynb and featuremap_variance.ipynb for the dehazing Uformer on MI355X: run the model over hazy
images, reduce every latent where the forward produces it (dehaze_hip.analysis: relative log amplitude of the half diagonal of the
spectrum, and the feature-map variance) and write the two tables the notebooks plot.  No plots are made.

  python My_fourier_analysis.py --arch Uformer --embed_dim 32 --weights model_best.pth --input_dir <dir with hazy/> --out logs/probsparse
  python My_fourier_analysis.py --attention dense --weights dense_best.pth --input_dir <dir with hazy/> --out logs/dense
  python My_fourier_analysis.py --synthetic 4 --batch_size 2 --train_ps 128 --arch Uformer          # synthetic haze, no files needed

--input_dir reads the .png / .jpg / .jpeg files of <dir>/hazy (the folder test_long_GPU.py --input_dir takes): square images of one
size whose side the model takes.
PREFIX_fourier.csv: one row per tap - index, name, kind (proj / msa / mlp / pool / up), side n, channels, maps, then
delta[k] = mean A[k] - mean A[0] for k = 0 .. n/2 - 1 (ragged rows; the last column is the notebooks' high-frequency figure).
PREFIX_variance.csv: index, name, kind, mean variance.  DHZ_FOURIER=0 computes both with the notebooks' ATen formula instead of the kernel.
"""
import argparse
import os
import sys

dir_name = os.path.dirname(os.path.abspath(__file__))
if dir_name not in sys.path:
    sys.path.insert(0, dir_name)

import torch  # noqa: E402

import utils  # noqa: E402
from dehaze_hip import analysis  # noqa: E402
from dehaze_hip.train import synthetic_batch  # noqa: E402


IMAGE_EXTS = (".png", ".jpg", ".jpeg")


def build_model(opt):
    import My_model
    import My_model_1
    mod = My_model_1 if opt.attention == "probsparse" else My_model
    if opt.arch == "Uformer":
        return mod.Uformer(img_size=opt.train_ps, embed_dim=opt.embed_dim, win_size=opt.win_size, token_projection="linear",
                           token_mlp=opt.token_mlp)
    if opt.arch in ("Uformer16", "Uformer32"):
        return mod.Uformer(img_size=opt.train_ps, embed_dim=int(opt.arch[-2:]), win_size=8, token_projection="linear", token_mlp="leff")
    raise SystemExit(f"--arch {opt.arch}: the taps exist for Uformer, Uformer16 and Uformer32 (hook other models on the module path and "
                     "call dehaze_hip.analysis.diag_log_amplitude(x, layout='nchw'))")


def side_multiple(opt):
    """the side the model takes: four 2x down-samplings, then whole windows at the bottleneck (a window larger than the bottleneck of the
    construction size shrinks to it, M1:764-766)"""
    return 16 * min(opt.win_size, max(1, opt.train_ps // 16))


def batches(opt, dev):
    mult = side_multiple(opt)
    if opt.synthetic:
        if opt.train_ps % mult:
            raise SystemExit(f"--train_ps {opt.train_ps} is no multiple of {mult}, which this model takes")
        for i in range(0, opt.synthetic, opt.batch_size):
            yield synthetic_batch(min(opt.batch_size, opt.synthetic - i), opt.train_ps, seed=opt.seed + i, device=dev)[1]
        return
    hazy = os.path.join(opt.input_dir, "hazy")
    if not os.path.isdir(hazy):
        raise SystemExit(f"--input_dir {opt.input_dir}: no hazy/ directory in it")
    # PNG is what the project's folders hold (dataset.py, generate_patches_SIDD.py); JPEG as the reference's own test folders
    files = sorted(f for f in os.listdir(hazy) if f.lower().endswith(IMAGE_EXTS))
    if not files:
        raise SystemExit(f"{hazy}: no images ({', '.join(IMAGE_EXTS)})")
    first = None
    for i in range(0, len(files), opt.batch_size):
        imgs = []
        for f in files[i:i + opt.batch_size]:
            img = torch.from_numpy(utils.load_img(os.path.join(hazy, f))).permute(2, 0, 1)
            H, W = img.shape[1:]
            if H != W or H % mult:
                raise SystemExit(f"{f}: {H} x {W} - the analysis takes square images whose side is a multiple of {mult} (the padded "
                                 "any-size route is out of its scope); crop or resize first")
            first = first or H
            if H != first:
                raise SystemExit(f"{f}: side {H}, the images before it {first} - one run averages maps of one size")
            imgs.append(img)
        yield torch.stack(imgs).to(dev)


def main(argv=None):
    p = argparse.ArgumentParser(description="Fourier and variance analysis of the Uformer's feature maps")
    p.add_argument("--arch", type=str, default="Uformer", help="Uformer (with --embed_dim / --win_size / --token_mlp), Uformer16, Uformer32")
    p.add_argument("--embed_dim", type=int, default=32)
    p.add_argument("--win_size", type=int, default=8)
    p.add_argument("--token_mlp", type=str, default="leff", help="ffn / leff")
    p.add_argument("--train_ps", type=int, default=128, help="the size the model is constructed for")
    p.add_argument("--weights", type=str, default="", help="checkpoint to analyse (none: the initial weights)")
    p.add_argument("--attention", choices=("probsparse", "dense"), default="probsparse", help="My_model_1.Uformer or its dense twin My_model.Uformer")
    p.add_argument("--input_dir", type=str, default="", help="directory with hazy/")
    p.add_argument("--synthetic", type=int, default=0, help="analyse N synthetic hazy images instead of --input_dir")
    p.add_argument("--batch_size", type=int, default=4)
    p.add_argument("--out", type=str, default="fourier_analysis", help="PREFIX of PREFIX_fourier.csv and PREFIX_variance.csv")
    p.add_argument("--seed", type=int, default=1234)
    opt = p.parse_args(argv)
    if bool(opt.synthetic) == bool(opt.input_dir):
        raise SystemExit("give --input_dir <dir with hazy/> or --synthetic N (one of them)")
    if opt.batch_size < 1:
        raise SystemExit("--batch_size must be >= 1")
    dev = torch.device("cuda", 0)
    torch.manual_seed(opt.seed)

    model = build_model(opt).to(dev)
    if opt.weights:
        utils.load_checkpoint(model, opt.weights)
    model.eval()
    with torch.no_grad(), analysis.taps(model) as col:
        for x in batches(opt, dev):
            model(x)
    rows = col.results()
    paths = analysis.write_csv(opt.out, rows)
    print("saved", *paths)
    return paths


if __name__ == "__main__":
    main()
