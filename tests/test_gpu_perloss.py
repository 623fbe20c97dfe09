"""FFA-Net's own recipe on the GPU: the squared-error tap kernels (dhz_mse_pair_fwd, dhz_mse_pair_bwd) and the pooling backward of a tap
(dhz_maxpool2x2_blocked_bwd_add) through the raw C-ABI against float64, their deterministic mode, the VGG16[:16] instance of the Winograd
engine against float64 library layers, the loss and its image gradient against the reference fixture tests/golden/ffa_perloss.npz,
ffa_train_step against float64 Adam, the fallback, and FFA_main.py.

Bounds are the project's existing ones, named at each assertion.  The image-gradient bound of the engine path is 8 x the error of the
fp32 LIBRARY path (the module's plain layers on the same GPU) against the same float64 reference, in the max and in the mean norm,
and never looser than mean < 1e-3 mean|ref|, max < 5e-2 max|ref| (tests/test_gpu_winograd.py: the library-tail test).  Measured on
MI355X (profiles/ffa_perloss.txt), image-gradient error against the float64 fixture:
    (2, 3, 32, 32)   library: max 1.026e-06 max|ref|, mean 1.079e-06 mean|ref|     engine: max 1.028e-06, mean 1.064e-06
    (2, 3, 48, 80)   library: max 1.685e-06 max|ref|, mean 1.206e-06 mean|ref|     engine: max 1.270e-06, mean 1.127e-06
so the engine sits at the library's own error, a factor 6 - 8 inside the bound."""
import functools
import glob
import math
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
GOLD = os.path.join(ROOT, "tests", "golden", "ffa_perloss.npz")
COUNTS = [8, 2 * 64 * 16 * 32, 3 * 64 * 32 * 16 + 4]          # one float4, a whole number of grid passes, a tail
GUARD = 64                                                    # NaN floats behind every output that must stay NaN


def _lib():
    from dehaze_hip import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def quiet_net():
    from PerceptualLoss import LossNetwork
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LossNetwork()


def library_warnings(rec):
    return [str(w.message) for w in rec if "library" in str(w.message)]


def make_pair(n, seed):
    """a: a post-ReLU-like map with exact zeros and a few negatives; g: the other map"""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(n, generator=gen).clamp(min=0)
    neg = torch.rand(n, generator=gen) < 0.1
    a = torch.where(neg, -torch.rand(n, generator=gen), a)
    a[0], a[1], a[2] = 1.25, 0.0, -0.5                        # every kind at every size
    g = torch.randn(n, generator=gen).abs()
    return a, g


# ------------------------------------------------------------------------------------------------ 1. kernels against float64
@pytest.mark.parametrize("n", COUNTS)
def test_mse_pair_kernels_against_float64(n):
    L = _lib()
    a, g = make_pair(n, seed=n)
    assert (a == 0).any() and (a < 0).any() and (a > 0).any()
    ad, gd = a.cuda(), g.cuda()
    start = 3.5
    s = torch.full((1,), start, device="cuda")
    L.call("dhz_mse_pair_fwd", ad.data_ptr(), gd.data_ptr(), s.data_ptr(), n, _st())
    want = start + ((a.double() - g.double()) ** 2).sum().item()
    print("mse fwd", n, s.item(), want)
    assert abs(s.item() - want) < 1e-5 * want, (s.item(), want)          # the bound of dhz_l1_pair_fwd's sums (test_gpu_winograd.py)

    gm = torch.tensor([0.37], device="cuda")
    ref = gm.double().cpu() * (2.0 / n) * (a.double() - g.double())
    for mask in (0, 1):
        buf = torch.full((n + GUARD,), float("nan"), device="cuda")
        L.call("dhz_mse_pair_bwd", ad.data_ptr(), gd.data_ptr(), gm.data_ptr(), buf.data_ptr(), n, mask, _st())
        da, tail = buf[:n].cpu(), buf[n:].cpu()
        assert not torch.isnan(da).any(), "an element was not written"
        assert torch.isnan(tail).all(), "written past the end"
        r = torch.where(a <= 0, torch.zeros_like(ref), ref) if mask else ref
        assert torch.allclose(da.double(), r, rtol=1e-6, atol=0), (da.double() - r).abs().max()      # dhz_l1_pair_bwd's bound; three roundings
        if mask:
            assert (da[a <= 0] == 0).all()
            assert (da[a > 0] != 0).any()


@pytest.mark.parametrize("N,H,W", [(2, 2, 4), (16, 32, 32), (3, 12, 20)])
def test_pool_backward_with_tap_gradient_against_float64(N, H, W):
    """gx = act > 0 ? route(gy) + addend : 0 on [N][H][W][8] maps, against float64 autograd of max_pool2d over relu (first-maximum ties:
    act is a post-ReLU map with whole windows of zeros)."""
    L = _lib()
    gen = torch.Generator().manual_seed(N * H + W)
    pre = torch.randn(N, H, W, 8, generator=gen)
    pre[:, 0:2, 0:2] = -1.0                                               # a window that is zero after the ReLU
    act = pre.clamp(min=0)
    gy = torch.randn(N, H // 2, W // 2, 8, generator=gen)
    add = torch.randn(N, H, W, 8, generator=gen)
    p64 = pre.double().permute(0, 3, 1, 2).requires_grad_()               # planes [N, 8, H, W]
    a64 = torch.relu(p64)
    pooled = torch.nn.functional.max_pool2d(a64, 2, 2)
    ((pooled * gy.double().permute(0, 3, 1, 2)).sum() + (a64 * add.double().permute(0, 3, 1, 2)).sum()).backward()
    ref = p64.grad.permute(0, 2, 3, 1)
    buf = torch.full((act.numel() + GUARD,), float("nan"), device="cuda")
    gyd, actd, addd = gy.cuda(), act.cuda(), add.cuda()                   # (referenced until the launch has run)
    L.call("dhz_maxpool2x2_blocked_bwd_add", gyd.data_ptr(), actd.data_ptr(), addd.data_ptr(), buf.data_ptr(), N, H, W, _st())
    torch.cuda.synchronize()
    got = buf[:act.numel()].cpu().view(N, H, W, 8)
    assert not torch.isnan(got).any() and torch.isnan(buf[act.numel():]).all()
    assert torch.allclose(got.double(), ref, rtol=1e-6, atol=0), (got.double() - ref).abs().max()    # one addition of two fp32 values
    assert (got[act <= 0] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. deterministic mode
def test_mse_pair_forward_deterministic_mode():
    from dehaze_hip import ops
    L = _lib()
    n = COUNTS[-1]
    a, g = make_pair(n, seed=2)
    ad, gd = a.cuda(), g.cuda()

    def run():
        s = torch.zeros(1, device="cuda")
        L.call("dhz_mse_pair_fwd", ad.data_ptr(), gd.data_ptr(), s.data_ptr(), n, _st())
        return s.cpu()

    plain = run()
    try:
        ops.set_deterministic(True)
        ops._stream()
        d1, d2 = run(), run()
        try:
            L.call("dhz_set_reserved_cus", 8)
            d3 = run()
        finally:
            L.call("dhz_set_reserved_cus", 0)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(d1, d2) and torch.equal(d1, d3), (d1, d2, d3)
    assert abs(plain.item() - d1.item()) < 1e-6 * abs(d1.item()), (plain.item(), d1.item())
    want = ((a.double() - g.double()) ** 2).sum().item()
    assert abs(d1.item() - want) < 1e-5 * want


# ------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def case_reference(case):
    """fixture inputs, loss and image gradient of the reference; the three taps by float64 conv2d / relu / max_pool2d on the CPU"""
    z = np.load(GOLD)
    x, gt = torch.from_numpy(z[f"x_{case}"]), torch.from_numpy(z[f"gt_{case}"])
    net = quiet_net().double()
    with torch.no_grad():
        taps = net._plain_features(x.double())
    return x, gt, float(z[f"loss_{case}"]), torch.from_numpy(z[f"grad_{case}"]), taps


@functools.lru_cache(maxsize=None)
def gpu_net():
    return quiet_net().cuda()


# ------------------------------------------------------------------------------------------------ 3. VGG16 taps of the engine
@pytest.mark.parametrize("case", [0, 1])
def test_vgg16_engine_taps_against_float64(case):
    x, _, _, _, taps64 = case_reference(case)
    net = gpu_net()
    xd = x.cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert net.engine_for(xd) is not None
        with torch.no_grad():
            feats = net.output_features(xd)
    assert not library_warnings(rec), library_warnings(rec)
    assert len(feats) == 3
    for f, r in zip(feats, taps64):
        assert f.shape == r.shape
        err = (f.cpu().double() - r).abs().max().item()
        print("tap", tuple(r.shape), "max error", err, "of", r.abs().max().item())
        assert err < 1e-4 * r.abs().max().item(), (err, r.abs().max().item())          # the tap bound of test_gpu_winograd.py


# ------------------------------------------------------------------------------------------------ 4. loss and image gradient
def grad_bounds(lib_err, ref):
    """8 x the library path's error, never looser than the existing caps (max 5e-2 max|ref|, mean 1e-3 mean|ref|)"""
    return (min(8 * lib_err.max().item(), 5e-2 * ref.abs().max().item()), min(8 * lib_err.mean().item(), 1e-3 * ref.abs().mean().item()))


@pytest.mark.parametrize("case", [0, 1])
def test_loss_and_image_gradient_against_the_reference_fixture(case):
    x, gt, loss64, grad64, _ = case_reference(case)
    net = gpu_net()
    xl = x.cuda().requires_grad_()
    net.forward_library(xl, gt.cuda()).backward()
    lib_err = (xl.grad.cpu().double() - grad64).abs()

    xe = x.cuda().requires_grad_()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        loss = net(xe, gt.cuda())
        loss.backward()
    assert not library_warnings(rec), library_warnings(rec)
    assert loss.dim() == 0 and loss.is_cuda
    err = (xe.grad.cpu().double() - grad64).abs()
    gmax, gmean = grad64.abs().max().item(), grad64.abs().mean().item()
    print(f"perloss case {case}: loss {loss.item():.9g} ref {loss64:.9g} rel {abs(loss.item() - loss64) / loss64:.3e}")
    print(f"perloss case {case}: gradient error / max|ref|: library {lib_err.max().item() / gmax:.3e} engine {err.max().item() / gmax:.3e}; "
          f"/ mean|ref|: library {lib_err.mean().item() / gmean:.3e} engine {err.mean().item() / gmean:.3e}")
    assert abs(loss.item() - loss64) < 2e-4 * loss64, (loss.item(), loss64)             # the bound of the contrastive-loss values
    bmax, bmean = grad_bounds(lib_err, grad64)
    assert err.max().item() <= bmax, (err.max().item(), bmax, gmax)
    assert err.mean().item() <= bmean, (err.mean().item(), bmean, gmean)
    # without a gradient: the same value, nothing saved
    with torch.no_grad():
        assert abs(net(x.cuda(), gt.cuda()).item() - loss.item()) <= 1e-6 * loss.item()


# ------------------------------------------------------------------------------------------------ 5. a tap that is pooled too
@pytest.mark.parametrize("which", [(0,), (1,), (0, 1, 2)])
def test_gradient_into_pooled_taps_against_float64(which):
    """a gradient into relu1_2 alone, relu2_2 alone (both are taps AND pooled: dhz_maxpool2x2_blocked_bwd_add), then into all three"""
    x, _, _, _, _ = case_reference(1)
    net = gpu_net()
    gen = torch.Generator().manual_seed(17)
    n64 = quiet_net().double()
    x64 = x.double().requires_grad_()
    f64 = n64._plain_features(x64)
    R = [torch.randn(f.shape, generator=gen) / f.numel() for f in f64]
    sum((f64[k] * R[k].double()).sum() for k in which).backward()
    ref = x64.grad

    def run(features):
        xd = x.cuda().requires_grad_()
        f = features(xd)
        sum((f[k] * R[k].cuda()).sum() for k in which).backward()
        return (xd.grad.cpu().double() - ref).abs()

    lib_err = run(net._plain_features)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        err = run(net.output_features)
    assert not library_warnings(rec), library_warnings(rec)
    bmax, bmean = grad_bounds(lib_err, ref)
    print(f"taps {which}: gradient error max library {lib_err.max().item():.3e} engine {err.max().item():.3e} of {ref.abs().max().item():.3e}; "
          f"mean library {lib_err.mean().item():.3e} engine {err.mean().item():.3e} of {ref.abs().mean().item():.3e}")
    assert err.max().item() <= bmax, (err.max().item(), bmax)
    assert err.mean().item() <= bmean, (err.mean().item(), bmean)


# ------------------------------------------------------------------------------------------------ 6. / 7. three steps
def seeded_ffa(seed=1234, blocks=2):
    import random
    from dehaze_hip.ffa import FFA
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return FFA(gps=3, blocks=blocks)


def step_data():
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(2, 3, 32, 32, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    return hazy, gt


def three_steps(deterministic=False):
    from dehaze_hip import ops
    from dehaze_hip.train import FlatAdamW, ffa_train_step
    hazy, gt = step_data()
    try:
        if deterministic:
            ops.set_deterministic(True)
        net = seeded_ffa().cuda()
        per = gpu_net()
        opt = FlatAdamW(net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
        net.train()
        losses, grads1 = [], None
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for s in range(3):
                loss, l1, lp = ffa_train_step(net, per, opt, None, hazy.cuda(), gt.cuda(), w_per=0.04)
                assert loss.is_cuda and l1.is_cuda and lp.is_cuda and loss.dim() == 0
                losses.append((loss.item(), l1.item(), lp.item()))
                if s == 0:
                    grads1 = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}
        assert not library_warnings(rec), library_warnings(rec)
        return losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, grads1
    finally:
        if deterministic:
            ops.set_deterministic(False)


def test_three_ffa_train_steps_against_float64_adam():
    losses, sd, grads1 = three_steps()
    hazy, gt = step_data()
    ref = seeded_ffa().double()
    per = quiet_net().double()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    for step in range(3):
        opt.zero_grad()
        out = ref._forward_torch(hazy.double())
        l1 = (out - gt.double()).abs().mean()
        lp = per.forward_library(out, gt.double())
        loss = l1 + 0.04 * lp
        loss.backward()
        if step == 0:
            worst = ("", 0.0)
            for n, p in ref.named_parameters():
                a, b = grads1[n].double().norm().item(), p.grad.norm().item()
                rel = abs(a - b) / (b + 1e-8)
                worst = max(worst, (n, rel), key=lambda t: t[1])
            print("first step: worst relative error of a parameter's gradient norm", worst)
            assert worst[1] < 5e-3, worst                                       # the bound of the FFA fixture test
        opt.step()
        print("FFA own-recipe step", step, losses[step], (loss.item(), l1.item(), lp.item()))
        assert abs(losses[step][0] - loss.item()) < 5e-5, (step, losses[step], loss.item())
        assert abs(losses[step][0] - (losses[step][1] + 0.04 * losses[step][2])) < 1e-6
    worst = max((sd[k].double() - v.detach()).abs().max().item() for k, v in ref.state_dict().items())
    print("parameters after three steps: worst error", worst)
    assert worst < 2.5e-4, worst                                                # test_gpu_ffa.py's 5e-4 at lr 2e-4; here lr is half


def test_deterministic_ffa_train_steps_are_bit_equal():
    la, sa, _ = three_steps(deterministic=True)
    lb, sb, _ = three_steps(deterministic=True)
    assert la == lb
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_bf16_model_is_refused():
    from dehaze_hip.train import FlatAdamW, ffa_train_step
    net = seeded_ffa(blocks=1).cuda().to(torch.bfloat16)
    hazy, gt = step_data()
    with pytest.raises(NotImplementedError, match="fp32"):
        ffa_train_step(net, None, FlatAdamW(net, lr=1e-4, weight_decay=0.0), None, hazy.cuda().to(torch.bfloat16), gt.cuda().to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ 8. fallback
def test_other_sizes_and_trainable_filters_run_the_plain_layers():
    from dehaze_hip import ops
    net = gpu_net()
    g = torch.Generator().manual_seed(3)
    x, gt = torch.rand(2, 3, 24, 40, generator=g).cuda(), torch.rand(2, 3, 24, 40, generator=g).cuda()
    ops._WARNED.clear()
    xa = x.clone().requires_grad_()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        la = net(xa, gt)
        la.backward()
        with torch.no_grad():
            net(x, gt)
    msgs = library_warnings(rec)
    assert len(msgs) == 1 and "PerLoss" in msgs[0], msgs
    xb = x.clone().requires_grad_()
    lb = net.forward_library(xb, gt)
    lb.backward()
    assert torch.allclose(la, lb, atol=2e-4, rtol=1e-3) and torch.allclose(xa.grad, xb.grad, atol=2e-4, rtol=1e-3)
    # trainable filters: the plain layers, no engine, and the filters receive gradients
    tr = quiet_net().cuda()
    for p in tr.parameters():
        p.requires_grad = True
    x32, gt32 = torch.rand(2, 3, 32, 32, generator=g).cuda(), torch.rand(2, 3, 32, 32, generator=g).cuda()
    assert net.engine_for(x32) is not None and tr.engine_for(x32) is None
    xt = x32.clone().requires_grad_()
    lt = tr(xt, gt32)
    lt.backward()
    assert tr._engine is None and all(p.grad is not None for p in tr.parameters())
    xe = x32.clone().requires_grad_()
    le = net(xe, gt32)
    le.backward()
    assert torch.allclose(lt, le, atol=2e-4, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ 9. command line
def test_ffa_main_command_line(tmp_path):
    mdir = str(tmp_path) + os.sep
    base = [sys.executable, "FFA_main.py", "--blocks", "2", "--bs", "2", "--crop_size", "64", "--synthetic", "4", "--val_synthetic", "2",
            "--eval_step", "2", "--perloss", "--model_dir", mdir, "--log_every", "1"]
    r = subprocess.run(base + ["--steps", "4"], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vals = [float(v) for v in re.findall(r"train loss : ([-+]?(?:nan|inf|[0-9.]+(?:e[-+]?[0-9]+)?))", r.stdout)]
    assert len(vals) == 4 and all(math.isfinite(v) and v > 0 for v in vals), (vals, r.stdout[-2000:])
    pks = sorted(glob.glob(os.path.join(mdir, "My_NH_ffa_3_2_*_psnr: *_ssim: *.pk")), key=os.path.getmtime)
    assert len(pks) == 2, os.listdir(mdir)
    ck = torch.load(pks[-1], map_location="cpu")
    assert set(ck) == {"step", "max_psnr", "max_ssim", "ssims", "psnrs", "losses", "model"}
    assert ck["step"] == 4 and len(ck["losses"]) == 4 and len(ck["psnrs"]) == len(ck["ssims"]) == 2
    assert all(math.isfinite(v) and v > 0 for v in ck["losses"]) and all(k.startswith("module.") for k in ck["model"])
    # --resume continues from the file's step
    r2 = subprocess.run(base + ["--steps", "6", "--resume", pks[-1]], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert "start_step:4" in r2.stdout and "step :5/6" in r2.stdout and "step :6/6" in r2.stdout and "step :4/6" not in r2.stdout
    ck6 = torch.load(glob.glob(os.path.join(mdir, "My_NH_ffa_3_2_6_psnr: *.pk"))[0], map_location="cpu")
    assert ck6["step"] == 6 and len(ck6["losses"]) == 6 and ck6["losses"][:4] == ck["losses"]
    # whole-image evaluation of that checkpoint (test_long_GPU.py has no --blocks: the depth comes from DHZ_FFA_BLOCKS)
    e = subprocess.run([sys.executable, "test_long_GPU.py", "--arch", "FFA", "--weights", pks[-1], "--synthetic", "2", "--height", "96",
                        "--width", "120", "--save_images", "False"], cwd=PKG, env=dict(os.environ, DHZ_FFA_BLOCKS="2"),
                       capture_output=True, text=True, timeout=300)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
    m = re.search(r"PSNR: ([-0-9.naif]+), SSIM: ([-0-9.naif]+)", e.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))), e.stdout[-2000:]
