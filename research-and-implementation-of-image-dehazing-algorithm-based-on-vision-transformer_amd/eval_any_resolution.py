"""Any-size evaluation in batches: test_in_any_resolution.py's evaluation (each image centred in a zero canvas whose side is a multiple of
128, the padding announced to every LeWin block through `mask`, the valid region cut back out, PSNR / SSIM twice) with consecutive images
of equal size restored as ONE forward of up to --batch_size images.  Same arguments, same output lines; --batch_size 1 is that script.

The reference's mask route builds a [B nW, 64, 64] tensor per block and adds the [nW, 64, 64] shift mask to it, which broadcasts for B = 1
only.  Here the padding reaches the kernels as one 64-bit word per window (bit i: token i is padding; Uformer._stage_pad_bits, five small
launches per forward), so a masked forward runs the fused window-attention kernels like a mask-free one, at any batch size.  DHZ_PAD_BITS=0
restores the tensor route (kernel chain, batch 1 only).

--gpu_metrics: the four printed numbers come from the float64 kernel dhz_ssim_pair (dehaze_hip/metrics.py) on the restored batch as it lies
in device memory - PSNR / SSIM in utils/metrics.py's form, PSNR2 / SSIM2 in the Gaussian form of utils.SSIM / utils.myPSNR - and are read
back once at the end; no restored image is copied to the host unless --save_images.  The first pair agrees with the default route to its
six printed decimals, the second to 2e-4 (the default's utils.SSIM is an fp32 evaluation)."""
import os
import sys

dir_name = os.path.dirname(os.path.abspath(__file__))
if dir_name not in sys.path:
    sys.path.insert(0, dir_name)

import torch  # noqa: E402

import test_in_any_resolution as TA  # noqa: E402
import utils  # noqa: E402
from utils.metrics import img_as_ubyte, peak_signal_noise_ratio as psnr_loss, structural_similarity as ssim_loss  # noqa: E402


def restore_any(model, rgb_noisy, factor=128):
    """TA.restore_any for rgb_noisy [B, 3, h, w]: B images of one size share the canvas geometry and go through ONE forward."""
    B, _, h, w = rgb_noisy.shape
    pairs = [TA.expand2square(rgb_noisy[i:i + 1], factor=factor) for i in range(B)]
    sq, mask = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    restored = model(sq, 1 - mask)
    return torch.masked_select(restored, mask.bool()).reshape(B, 3, h, w)


def batches_of_equal_size(items, batch_size):
    """runs of CONSECUTIVE items (gt, noisy, filenames) whose images have the same size, cut into batches of at most batch_size; the order
    of the items is kept"""
    out = []
    for it in items:
        if out and len(out[-1]) < batch_size and out[-1][0][1].shape == it[1].shape:
            out[-1].append(it)
        else:
            out.append([it])
    return out


def build_parser():
    """TA's parser plus --gpu_metrics"""
    parser = TA.build_parser()
    parser.add_argument('--gpu_metrics', action='store_true',
                        help='score on the device in float64 (dhz_ssim_pair): all four printed numbers, no per-image host copy of the restored '
                             'image (unless --save_images), one read-back at the end')
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_any_resolution.py needs a HIP device")
    dev = torch.device("cuda", int(str(args.gpus).split(",")[0]))
    torch.cuda.set_device(dev)
    if args.save_images:
        utils.mkdir(args.result_dir)
    model_restoration = utils.get_arch(args)
    if args.weights:
        utils.load_checkpoint(model_restoration, args.weights)
        print("===>Testing using weights: ", args.weights)
    model_restoration.to(dev).eval()
    if args.synthetic > 0:
        from dehaze_hip.train import synthetic_batch
        items = [synthetic_batch(1, (args.height, args.width), seed=700 + i, device="cpu") + (["synthetic_%03d.png" % i],)
                 for i in range(args.synthetic)]
    else:
        from utils.loader import get_validation_data
        ds = get_validation_data(args.input_dir)
        items = [(ds[i][0][None], ds[i][1][None], [ds[i][2]]) for i in range(len(ds))]

    psnr_val_rgb, ssim_val_rgb, psnr_val_rgb2, ssim_val_rgb2 = [], [], [], []
    if args.gpu_metrics:
        from dehaze_hip.metrics import Scores          # opt-in: a default run never imports it
        first, second = Scores(), Scores()
    with torch.no_grad():
        for batch in batches_of_equal_size(items, max(1, args.batch_size)):
            out = restore_any(model_restoration, torch.cat([it[1] for it in batch]).to(dev), factor=128)
            if args.gpu_metrics:
                restored = torch.clamp(out, 0, 1)
                gts = torch.cat([it[0] for it in batch]).to(dev)
                first.add_uniform(gts, restored)                         # psnr_loss(restored, gt): the restored image is image_true
                second.add_ffa(restored, gts, rmse0=float("inf"))        # utils.SSIM / myPSNR: the clamped pair, no special case at rmse 0
                if args.save_images:
                    for i, (_, _, filenames) in enumerate(batch):
                        utils.save_img(os.path.join(args.result_dir, filenames[0]),
                                       img_as_ubyte(restored[i].permute(1, 2, 0).cpu().numpy()))
                continue
            for i, (gt, _, filenames) in enumerate(batch):
                rgb_gt = gt.numpy().squeeze().transpose((1, 2, 0))
                rgb_restored = torch.clamp(out[i:i + 1], 0, 1).cpu()
                ssim_val_rgb2.append(utils.SSIM(rgb_restored, torch.clamp(gt, 0, 1)).item())
                psnr_val_rgb2.append(utils.batch_PSNR(rgb_restored, torch.clamp(gt, 0, 1), False).item())
                rgb_restored = rgb_restored.numpy().squeeze().transpose((1, 2, 0))
                psnr_val_rgb.append(psnr_loss(rgb_restored, rgb_gt))
                ssim_val_rgb.append(ssim_loss(rgb_restored, rgb_gt, multichannel=True))
                if args.save_images:
                    utils.save_img(os.path.join(args.result_dir, filenames[0]), img_as_ubyte(rgb_restored))
    if args.gpu_metrics:
        ssim_val_rgb, psnr_val_rgb = first.read()
        ssim_val_rgb2, psnr_val_rgb2 = second.read()
    n = len(items)
    out = (sum(psnr_val_rgb) / n, sum(ssim_val_rgb) / n, sum(psnr_val_rgb2) / n, sum(ssim_val_rgb2) / n)
    print("PSNR: %f, SSIM: %f " % out[:2])
    print("PSNR2: %f, SSIM2: %f " % out[2:])
    return out


if __name__ == "__main__":
    main()
