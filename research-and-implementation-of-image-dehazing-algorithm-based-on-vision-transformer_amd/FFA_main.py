"""FFA-Net trained under its OWN recipe (FFA_model/main.py, options of FFA_model/option.py) on the HIP kernels - the recipe the reference
trains its FFA baseline with, as opposed to My_train.py --arch FFA, which trains the same network under Uformer's
(Charbonnier + VGG19 contrastive loss + AdamW + epoch-wise warm-up / cosine):

  * loss = L1(out, y) [+ 0.04 * PerLoss(out, y) with --perloss: VGG16 relu1_2 / relu2_2 / relu3_3 MSE, PerceptualLoss.py], out unclamped
  * Adam, lr 1e-4, betas (0.9, 0.999), eps 1e-8 - FlatAdamW with weight_decay 0 is that update, in one launch
  * per-step cosine decay lr = 0.5 (1 + cos(t pi / T)) lr0 (--no_lr_sche: constant)
  * every --eval_step steps: PSNR / SSIM over the validation pairs (utils/metrics.py, on the host; --metrics device: the same definitions from
    the float64 kernel dhz_ssim_pair, no per-image host copy; --metrics ffa: the reference's own FFA_model/metrics.py, main.py:151-173), a checkpoint
    `<model_dir><name>_<step>_psnr: <p>_ssim: <s>.pk` with the reference's keys (step, max_psnr, max_ssim, ssims, psnrs, losses, model),
    and `<model_dir><name>_best.pk` when both metrics improve.  `model` keys carry DataParallel's `module.` prefix like the reference's;
    utils.load_checkpoint reads either form, so `test_long_GPU.py --arch FFA --weights x.pk` evaluates such a file.
  * --whole_img: batches are whole stored images, no crop - the REFERENCE'S DEFAULT setting (FFA_model/data_utils.py:21-23: crop_size =
    'whole_img' unless --crop is given; SOTS / ITS frames are 620 x 460, NH-HAZE frames 1600 x 1200).  Here it is an explicit option:
    without it the script cuts --crop_size squares as before (and still ignores --crop).  The images of a store share one size
    (PatchStoreHBM.from_dir asserts it); they pass the feed kernel's h x w form (dhz_crop_augment_pair_rect: identity, rot180 and the two
    flips on non-square frames - see PatchStoreHBM.batch), the network's `_any` kernels, the any-size L1 mean and, with --perloss, the
    VGG16 engine's ragged convolutions and floor-mode poolings: no library compute op in the step for sides from 32 up.  With
    --synthetic N the pairs are --height x --width (validation pairs too).
  * --resume [file]: continue from `file`, or without a value from `<model_dir><name>_best.pk` (the reference's rule: only if it exists)

Differences from the reference's script: one process, no DataParallel; data in HBM like My_train.py (--synthetic N, --train_dir / --val_dir
directories of PNG pairs through dataset.PatchStoreHBM and the crop / augment kernel, or `.pt` files); the loss values are fetched every
--log_every steps instead of every step (no host sync inside the step); --deterministic.

The reference's loader (FFA_model/data_utils.py, RESIDE_Dataset) is restated by dataset.ImageStoreHBM and the feed kernel
dhz_crop_augment_pair_ragged: folders whose images differ in size (I-HAZE, O-HAZE), RESIDE's layout with --pairing reside (hazy `1400_1.png` /
`1400_1_0.85.png` -> clear `1400` + --clear_format, many hazy frames per clear frame, the larger clear frame centre-cropped to the hazy
frame's size) and, with --normalize, the input normalisation of data_utils.py:79 (mean 0.64 / 0.6 / 0.58, std 0.14 / 0.15 / 0.152) on the
training batches in the feed kernel and on the validation inputs once at load time.  A checkpoint trained with --normalize has the same
keys as any other; evaluate it with `FFA_test.py --normalize`.  The store is chosen by dataset.train_store: a folder of equally many gt and
hazy PNGs of one size without these options stays on PatchStoreHBM, draw for draw as before; crops are drawn from the items that hold them
(ImageStoreHBM.eligible - the same torch.randint draw when all do) and --whole_img batches of a mixed-size store from one size bucket
(draw_whole_batch).  NOT restated: the reference's redraw loop for images smaller than the crop (data_utils.py:54-56), the zero-padding of a
clear frame smaller than its hazy frame (an error here) and PIL's no-expand 90 degree rotation of non-square frames.  Stores larger than
one device's memory (OTS) are out of scope.
"""
import argparse
import math
import os
import random
import sys
import time

dir_name = os.path.dirname(os.path.abspath(__file__))
if dir_name not in sys.path:
    sys.path.insert(0, dir_name)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import utils  # noqa: E402
from dehaze_hip.ffa import FFA  # noqa: E402
from dehaze_hip.train import FlatAdamW, ffa_train_step, lr_schedule_cosdecay, synthetic_batch  # noqa: E402
from PerceptualLoss import PerLoss  # noqa: E402
from utils.metrics import peak_signal_noise_ratio, structural_similarity  # noqa: E402


def nonneg_float(text):
    v = float(text)
    if not v >= 0:
        raise argparse.ArgumentTypeError(f"a weight >= 0, got {text}")
    return v


def parse(argv=None):
    parser = argparse.ArgumentParser(description="FFA-Net, its own training recipe")
    # FFA_model/option.py
    parser.add_argument('--steps', type=int, default=100000)
    parser.add_argument('--device', type=str, default='Automatic detection')
    parser.add_argument('--resume', nargs='?', const=True, default=False, help='continue from this .pk (no value: <model_dir><name>_best.pk)')
    parser.add_argument('--eval_step', type=int, default=5000)
    parser.add_argument('--lr', default=0.0001, type=float, help='learning rate')
    parser.add_argument('--model_dir', type=str, default='./FFA_pretrain_weight/')
    parser.add_argument('--trainset', type=str, default='its_train')
    parser.add_argument('--testset', type=str, default='its_test')
    parser.add_argument('--net', type=str, default='ffa')
    parser.add_argument('--gps', type=int, default=3, help='residual_groups')
    parser.add_argument('--blocks', type=int, default=20, help='residual_blocks')
    parser.add_argument('--bs', type=int, default=4, help='batch size')
    parser.add_argument('--crop', action='store_true')
    parser.add_argument('--crop_size', type=int, default=240, help='patch side of a training sample')
    parser.add_argument('--no_lr_sche', action='store_true', help='no lr cos schedule')
    parser.add_argument('--perloss', action='store_true', help='perceptual loss')
    # this project's data options (My_train.py)
    parser.add_argument('--train_dir', type=str, default='../datasets/NH_haze/train', help='<dir>/gt, <dir>/hazy PNG pairs, or a .pt file')
    parser.add_argument('--val_dir', type=str, default='../datasets/NH_haze/val')
    parser.add_argument('--synthetic', type=int, default=0, help='train on N synthetic pairs (HBM resident)')
    parser.add_argument('--val_synthetic', type=int, default=8)
    parser.add_argument('--deterministic', action='store_true',
                        help='bit-reproducible steps: fixed-order reductions instead of fp32 atomics (slower)')
    parser.add_argument('--log_every', type=int, default=10, help='host sync cadence for the progress line')
    parser.add_argument('--whole_img', action='store_true',
                        help="train on whole stored images, no crop: the reference's default setting (data_utils.py:21, crop_size = 'whole_img')")
    parser.add_argument('--height', type=int, default=460, help='--whole_img --synthetic: image height (SOTS / ITS frames: 460)')
    parser.add_argument('--width', type=int, default=620, help='--whole_img --synthetic: image width (SOTS / ITS frames: 620)')
    parser.add_argument('--metrics', choices=('host', 'device', 'ffa'), default='host',
                        help="validation scores: host = utils/metrics.py on host copies; device = the same definitions from the float64 HIP "
                             "kernel, read back once per pass; ffa = the reference's FFA_model/metrics.py (11 x 11 Gaussian SSIM, clamped PSNR) "
                             "from that kernel")
    parser.add_argument('--ssimloss', type=nonneg_float, default=0,
                        help="weight of the SSIM loss 1 - ssim(out, y) on the HIP kernels (FFA_model/metrics.py's ssim: 11 x 11 Gaussian "
                             "window, both images clamped); 0: off")
    parser.add_argument('--tvloss', type=nonneg_float, default=0,
                        help="weight of the total-variation term of losses.py on the output, on the HIP kernels; 0: off")
    parser.add_argument('--tv_form', choices=('sq', 'beta'), default='sq',
                        help="--tvloss: sq = TVLoss() (squared differences), beta = tv_loss(x, --tv_beta) (sum of s ** beta, reg_coeff 5)")
    parser.add_argument('--tv_beta', type=float, default=0.5, help="--tv_form beta: the exponent (> 0)")
    parser.add_argument('--pairing', choices=('sorted', 'reside'), default='sorted',
                        help="how <train_dir>/hazy maps to <train_dir>/gt: sorted = one to one in sorted order; reside = hazy `1400_1.png` "
                             "-> gt `1400` + --clear_format (FFA_model/data_utils.py:58-60)")
    parser.add_argument('--clear_format', type=str, default='.png', help="--pairing reside: extension of the clear frames (OTS: .jpg)")
    parser.add_argument('--normalize', action='store_true',
                        help="normalise the hazy input with the mean / std of FFA_model/data_utils.py:79 (evaluate with FFA_test.py --normalize)")
    opt = parser.parse_args(argv)
    opt.model_name = 'My_NH' + '_' + opt.net.split('.')[0] + '_' + str(opt.gps) + '_' + str(opt.blocks)
    opt.model_path = opt.model_dir + opt.model_name          # option.py:38: a prefix, not a directory join
    return opt


def load_pairs(path, device):
    blob = torch.load(path, map_location="cpu")
    return blob["target"].float().to(device), blob["input"].float().to(device)


def evaluate(net, vt, vi, metrics="host"):
    """mean (SSIM, PSNR) over the validation pairs, one image at a time (they may differ in size).  metrics: "host" - utils/metrics.py on
    host copies; "device" - the same two definitions from dhz_ssim_pair, the per-image values read back once; "ffa" - main.py:151-173:
    the unclamped prediction goes to FFA_model/metrics.py's ssim / psnr, which clamp inside"""
    if metrics not in ("host", "device", "ffa"):
        raise ValueError(f"evaluate: metrics={metrics!r}")
    net.eval()
    ssims, psnrs = [], []
    with torch.no_grad():
        if metrics == "host":
            for t, x in zip(vt, vi):
                pred = torch.clamp(net(x.unsqueeze(0)), 0, 1)[0]
                a = t.permute(1, 2, 0).cpu().numpy()
                b = pred.permute(1, 2, 0).cpu().numpy()
                psnrs.append(float(peak_signal_noise_ratio(a, b)))
                ssims.append(float(structural_similarity(a, b, multichannel=True)))
        else:
            from dehaze_hip.metrics import Scores          # opt-in: a default run never imports it
            scores = Scores()
            for t, x in zip(vt, vi):
                pred = net(x.unsqueeze(0))
                if metrics == "ffa":
                    scores.add_ffa(pred, t.unsqueeze(0))
                else:
                    scores.add_uniform(torch.clamp(pred, 0, 1), t.unsqueeze(0))
            ssims, psnrs = scores.read()
    net.train()
    return float(np.mean(ssims)), float(np.mean(psnrs))


def main(argv=None):
    opt = parse(argv)
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    opt.device = str(dev)
    if opt.deterministic:
        from dehaze_hip import ops
        ops.set_deterministic(True)
    print(opt)
    print('model_dir:', opt.model_path)
    os.makedirs(os.path.dirname(os.path.abspath(opt.model_path)), exist_ok=True)

    random.seed(1234)
    np.random.seed(1234)
    torch.manual_seed(1234)
    torch.cuda.manual_seed_all(1234)

    net = FFA(gps=opt.gps, blocks=opt.blocks)
    optimizer = FlatAdamW(net, lr=opt.lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    net.to(dev)
    perloss = None
    if opt.perloss:
        if not os.environ.get("DEHAZE_VGG16_WEIGHTS") and not opt.synthetic and not os.environ.get("DEHAZE_ALLOW_RANDOM_VGG"):
            raise SystemExit("FFA_main: --perloss needs the ImageNet VGG16 checkpoint the reference downloads (main.py:187): set "
                             "DEHAZE_VGG16_WEIGHTS=/path/to/vgg16-397923af.pth, or DEHAZE_ALLOW_RANDOM_VGG=1 to train against SEEDED "
                             "RANDOM VGG features (not the reference's loss)")
        perloss = PerLoss().to(dev)
    ssim_term = None
    if opt.ssimloss > 0:
        from dehaze_hip.ssim_loss import SSIMLoss          # opt-in: a default run never imports it
        ssim_term = SSIMLoss()
    extra = {}                                     # keywords of the opt-in terms: a default run passes none
    if ssim_term is not None:
        extra.update(ssim_loss=ssim_term, w_ssim=opt.ssimloss)
    tv_term = None
    if opt.tvloss > 0:
        from dehaze_hip.tv_loss import TVTerm              # opt-in: a default run never imports it
        tv_term = TVTerm(opt.tv_form, opt.tv_beta)
        extra.update(tv_term=tv_term, w_tv=opt.tvloss)

    losses, ssims, psnrs = [], [], []
    start_step, max_ssim, max_psnr = 0, 0.0, 0.0
    resume = opt.model_path + '_best.pk' if opt.resume is True else opt.resume
    if resume and os.path.exists(resume):
        print(f'resume from {resume}')
        ckp = torch.load(resume, map_location="cpu")
        utils.load_checkpoint(net, resume, map_location=dev)
        losses, ssims, psnrs = list(ckp['losses']), list(ckp['ssims']), list(ckp['psnrs'])
        start_step, max_ssim, max_psnr = int(ckp['step']), float(ckp['max_ssim']), float(ckp['max_psnr'])
        print(f'start_step:{start_step} start training ---')
    else:
        print('train from scratch *** ')

    # ---- data (HBM resident)
    store = tgt_all = inp_all = None
    ragged = False                                 # an ImageStoreHBM: sizes differ, RESIDE pairing or --normalize
    if opt.synthetic > 0:
        size = (opt.height, opt.width) if opt.whole_img else opt.crop_size
        tgt_all, inp_all = synthetic_batch(opt.synthetic, size, seed=1234, device=dev)
        vt, vi = synthetic_batch(opt.val_synthetic, size, seed=4321, device=dev)
    elif os.path.isdir(opt.train_dir):
        from dataset import DataLoaderVal, ImageStoreHBM, train_store
        store = train_store(opt.train_dir, dev, pairing=opt.pairing, clear_format=opt.clear_format, normalize=opt.normalize)
        ragged = isinstance(store, ImageStoreHBM)
        val_set = DataLoaderVal(opt.val_dir)
        items = [val_set[i] for i in range(len(val_set))]
        vt, vi = [v[0].to(dev) for v in items], [v[1].to(dev) for v in items]
    else:
        tgt_all, inp_all = load_pairs(opt.train_dir, dev)
        vt, vi = load_pairs(opt.val_dir, dev)
    norm = None
    if opt.normalize:                              # data_utils.py:79; the store's batches are normalised by the feed kernel
        from dataset import RESIDE_MEAN, RESIDE_STD
        norm = (RESIDE_MEAN, RESIDE_STD)
        mean, std = (torch.tensor(v, device=dev).view(3, 1, 1) for v in norm)
        vi = [(v - mean) / std for v in vi] if isinstance(vi, list) else (vi - mean) / std
        if inp_all is not None:
            inp_all = (inp_all - mean) / std
    n_train = len(store) if store is not None else tgt_all.shape[0]
    pick = None                                    # the item ids a crop batch is drawn from, where not all of them hold the crop
    if store is not None and ragged and not opt.whole_img:
        pick = store.eligible(opt.crop_size, opt.crop_size)
        n_train = len(pick)

    def state(step):
        return {'step': step, 'max_psnr': max_psnr, 'max_ssim': max_ssim, 'ssims': ssims, 'psnrs': psnrs, 'losses': losses,
                'model': {'module.' + k: v for k, v in net.state_dict().items()}}

    net.train()
    t0 = time.time()
    pending = []                                   # device scalars of the steps since the last host sync
    for step in range(start_step + 1, opt.steps + 1):
        lr = opt.lr
        if not opt.no_lr_sche:
            lr = lr_schedule_cosdecay(step, opt.steps, opt.lr)
            for g in optimizer.param_groups:
                g["lr"] = lr
        if ragged and opt.whole_img and store.uniform is None:
            sel = store.draw_whole_batch(opt.bs)         # whole images of mixed sizes: one size per batch
        else:
            sel = torch.randint(n_train, (opt.bs,))      # main.py:84: a fresh shuffled batch every step
            if pick is not None:
                sel = pick[sel]
        if ragged:
            y, x = store.batch(sel.tolist(), None if opt.whole_img else opt.crop_size, normalize=norm)
        elif store is not None:
            y, x = store.batch(sel.tolist(), None if opt.whole_img else opt.crop_size)
        else:
            y, x = tgt_all[sel.to(dev)], inp_all[sel.to(dev)]
        loss, _, _ = ffa_train_step(net, perloss, optimizer, None, x, y, **extra)
        pending.append(loss)
        if step % opt.log_every == 0 or step % opt.eval_step == 0 or step == opt.steps:
            losses += torch.stack(pending).tolist()
            pending = []
            ssim_txt = f'| ssim loss : {ssim_term.last_value.item():.5f}' if ssim_term is not None else ''
            if tv_term is not None:
                ssim_txt += f'| tv loss : {tv_term.last_value.item():.5f}'
            print(f'\rtrain loss : {losses[-1]:.5f}{ssim_txt}| step :{step}/{opt.steps}|lr :{lr :.7f} '
                  f'|time_used :{(time.time() - t0) / 60 :.1f}', end='', flush=True)
        if step % opt.eval_step == 0:
            ssim_eval, psnr_eval = evaluate(net, vt, vi, opt.metrics)
            print(f'\nstep :{step} |ssim:{ssim_eval:.4f}| psnr:{psnr_eval:.4f}')
            ssims.append(ssim_eval)
            psnrs.append(psnr_eval)
            torch.save(state(step), opt.model_path + '_' + str(step) + '_psnr: ' + str(psnr_eval) + '_ssim: ' + str(ssim_eval) + '.pk')
            if ssim_eval > max_ssim and psnr_eval > max_psnr:
                max_ssim, max_psnr = max(max_ssim, ssim_eval), max(max_psnr, psnr_eval)
                torch.save(state(step), opt.model_path + '_best' + '.pk')
                print(f'   model saved at step :{step}| max_psnr:{max_psnr:.4f}|max_ssim:{max_ssim:.4f}')
    if losses and not math.isfinite(losses[-1]):
        raise SystemExit("FFA_main: the loss is not finite")
    for name, vals in (('losses', losses), ('ssims', ssims), ('psnrs', psnrs)):
        np.save(f'{opt.model_path}_{opt.steps}_{name}.npy', np.asarray(vals, dtype=np.float64))
    print()


if __name__ == "__main__":
    main()
