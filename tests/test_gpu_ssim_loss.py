"""SSIM as a training loss on the device: dhz_ssim_loss_workspace_bytes / dhz_ssim_loss_fwd / dhz_ssim_loss_bwd (csrc/ssim_loss.hip),
dehaze_hip.ssim_loss.SSIMLoss, the term in train_step / ffa_train_step and the two command lines.

The oracle is the reference's own function under float64 autograd (tests/golden/ssim_loss.npz, gen_golden_ssim_loss.py).  The bound on the
value and on max |d grad| is measured against the reference, not the code under test: twice the reference's own fp32 error against its
float64 result on that case (both in the golden; the factor 2 covers another summation order).  The gradient, stored in the golden as
fp32, has a floor of 2^-22 max|grad| for the fp32 roundings of the stored and of the compared result; the value, stored as float64, has
none but the fp32 spacing of the loss the entry writes, which is below twice the reference's error on every case.
"""
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from _grid import reserved_grid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
CASES = [("noise", "ffa"), ("smooth", "ffa"), ("range", "ffa"), ("two_tiles", "ffa"),
         ("noise", "aaa"), ("two_tiles", "aaa"), ("one_pixel", "aaa"), ("thin", "aaa")]
C1, C2 = 0.01 ** 2, 0.03 ** 2


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ssim_loss")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def raw(pred, gt, window, valid, clamp, g=1.0, need_grad=True):
    """the three entries called directly: (loss, dx); dx starts as NaN, so a pixel the backward does not WRITE shows"""
    from dehaze_hip import _lib
    lib = _lib.load()
    B, C, H, W = pred.shape
    nbytes = lib.dhz_ssim_loss_workspace_bytes(B, C, H, W, int(valid))
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=pred.device)
    loss = torch.full((), float("nan"), device=pred.device)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("dhz_ssim_loss_fwd", loss.data_ptr(), pred.data_ptr(), gt.data_ptr(), B, C, H, W, 11, window.data_ptr(), int(valid), C1, C2,
              int(clamp), int(need_grad), ws.data_ptr(), nbytes, s)
    if not need_grad:
        return loss, None
    gl = torch.tensor(float(g), device=pred.device)
    dx = torch.full_like(pred, float("nan"))
    _lib.call("dhz_ssim_loss_bwd", dx.data_ptr(), gl.data_ptr(), pred.data_ptr(), gt.data_ptr(), B, C, H, W, 11, window.data_ptr(), int(valid),
              C1, C2, int(clamp), ws.data_ptr(), nbytes, s)
    return loss, dx


def case(gold, name, rule, dev):
    key = f"{name}_{rule}"
    pred, gt = torch.from_numpy(gold[name + "_pred"]).to(dev), torch.from_numpy(gold[name + "_gt"]).to(dev)
    g64 = gold[key + "_grad"].astype(np.float64)
    v64, v32 = float(gold[key + "_ssim_f64"]), float(gold[key + "_ssim_f32"])
    vbound = max(2 * abs(v32 - v64), float(np.spacing(np.float32(1.0 - v64))))
    gbound = max(2 * float(gold[key + "_grad_err_f32"]), 2.0 ** -22 * np.abs(g64).max())
    return pred, gt, torch.from_numpy(gold["window"]).to(dev), g64, v64, vbound, gbound


# ------------------------------------------------------------------------------------------------ 1. raw ABI against the golden
@pytest.mark.parametrize("name,rule", CASES)
def test_raw_entries_against_the_float64_reference(gold, dev, name, rule):
    pred, gt, window, g64, v64, vbound, gbound = case(gold, name, rule, dev)
    valid, clamp = rule == "aaa", rule == "ffa"
    loss, dx = raw(pred, gt, window, valid, clamp)
    verr = abs((1.0 - float(loss.double().item())) - v64)
    gerr = np.abs(-dx.double().cpu().numpy() - g64).max()              # d loss = - d ssim
    print(f"{name}/{rule}: value err {verr:.3e} (bound {vbound:.3e}); grad err {gerr:.3e} = {gerr / np.abs(g64).max():.2e} of max|grad| "
          f"(bound {gbound:.3e} = {gbound / np.abs(g64).max():.2e})")
    assert torch.isfinite(dx).all()                                    # every pixel written
    assert verr <= vbound
    assert gerr <= gbound
    # the forward alone writes the same bits; the upstream gradient scales dx (a power of two: exactly)
    assert torch.equal(raw(pred, gt, window, valid, clamp, need_grad=False)[0], loss)
    assert torch.equal(raw(pred, gt, window, valid, clamp, g=0.25)[1], 0.25 * dx)


# ------------------------------------------------------------------------------------------------ 2. the clamp's mask
@pytest.mark.parametrize("name", ["noise", "range", "two_tiles"])
def test_gradient_where_the_clamp_masks(gold, dev, name):
    pred, gt, window, g64, *_ = case(gold, name, "ffa", dev)
    _, dx = raw(pred, gt, window, False, True)
    outside = (pred < 0) | (pred > 1)
    assert outside.any() and bool((dx[outside] == 0).all())
    if name == "two_tiles":
        g = torch.from_numpy(g64).to(dev)
        for bound in (0.0, 1.0):
            at = (pred == bound) & (g != 0)
            assert at.sum() > 100 and bool((dx[at] != 0).all())        # the inclusive bounds pass the gradient, as torch.clamp does
    # without the clamp nothing is masked
    _, dx_raw = raw(pred, gt, window, False, False)
    assert bool((dx_raw[outside] != 0).any())


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("rule", ["ffa", "aaa"])
def test_bits_do_not_depend_on_the_grid_or_the_mode(gold, dev, rule):
    from dehaze_hip import ops
    pred, gt, window, *_ = case(gold, "two_tiles", rule, dev)
    valid, clamp = rule == "aaa", rule == "ffa"
    loss0, dx0 = raw(pred, gt, window, valid, clamp)
    for level in (None, 8, 9):
        with reserved_grid(level):
            for _ in range(3):
                loss, dx = raw(pred, gt, window, valid, clamp)
                assert torch.equal(loss, loss0) and torch.equal(dx, dx0), level
    try:
        ops.set_deterministic(True)
        for _ in range(3):
            loss, dx = raw(pred, gt, window, valid, clamp)
            assert torch.equal(loss, loss0) and torch.equal(dx, dx0)
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 4. the module
@pytest.fixture
def spy(monkeypatch):
    from dehaze_hip import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return names


@pytest.mark.parametrize("name,rule", [("noise", "ffa"), ("two_tiles", "ffa"), ("two_tiles", "aaa"), ("thin", "aaa")])
def test_module_against_the_aten_route(gold, dev, spy, monkeypatch, name, rule):
    from dehaze_hip import ssim_loss as SL
    pred, gt, _, g64, v64, vbound, gbound = case(gold, name, rule, dev)
    mod = SL.SSIMLoss() if rule == "ffa" else SL.SSIMLoss(valid=True, clamp=False, val_range=1)
    a = pred.clone().requires_grad_(True)
    la = mod(a, gt)
    assert la.dim() == 0 and la.is_cuda and la.dtype == torch.float32 and torch.equal(mod.last_value, la.detach())
    la.backward()
    assert spy == ["dhz_ssim_loss_fwd", "dhz_ssim_loss_bwd"]
    del spy[:]
    monkeypatch.setattr(SL, "KERNELS", False)                          # what DHZ_SSIM_LOSS=0 sets
    b = pred.clone().requires_grad_(True)
    lb = mod(b, gt)
    lb.backward()
    assert spy == []
    verr, gerr = abs(la.item() - lb.item()), (a.grad - b.grad).abs().max().item()
    print(f"{name}/{rule}: kernels vs ATen: value {verr:.3e} (bound {vbound:.3e}), grad {gerr:.3e} (bound {gbound:.3e})")
    assert verr <= vbound and gerr <= gbound


def test_module_routing(gold, dev, spy, monkeypatch):
    from dehaze_hip import ssim_loss as SL
    pred, gt, *_ = case(gold, "noise", "ffa", dev)
    mod = SL.SSIMLoss()
    # a channel-sliced view gives what its contiguous copy gives
    wide = torch.cat([pred[:, :1], pred], 1)
    view = wide[:, 1:]
    assert not view.is_contiguous() and torch.equal(view, pred)
    a, b = view.detach().requires_grad_(True), pred.clone().requires_grad_(True)
    la, lb = mod(a, gt), mod(b, gt)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert spy == ["dhz_ssim_loss_fwd", "dhz_ssim_loss_fwd", "dhz_ssim_loss_bwd", "dhz_ssim_loss_bwd"]
    del spy[:]
    # the kernel route is once differentiable: a double backward raises instead of treating dx as a constant
    # (with an upstream gradient that itself requires grad, as under a gradient penalty; with a constant one dx simply has no graph)
    c, w = pred.clone().requires_grad_(True), torch.ones((), device=dev, requires_grad=True)
    gc, = torch.autograd.grad(mod(c, gt) * w, c, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gc.sum().backward()
    gc, = torch.autograd.grad(mod(c, gt), c, create_graph=True)
    assert not gc.requires_grad
    del spy[:]
    # no gradient wanted: the forward alone, the same bits
    with torch.no_grad():
        assert torch.equal(mod(pred, gt), lb.detach())
    assert spy == ["dhz_ssim_loss_fwd"]
    del spy[:]
    # bf16, a target that requires grad, a plane smaller than the window under the valid rule: the ATen formula
    l16 = mod(pred.bfloat16().requires_grad_(True), gt.bfloat16())
    assert l16.dtype == torch.bfloat16
    t = gt.clone().requires_grad_(True)
    lt = mod(pred.clone().requires_grad_(True), t)
    lt.backward()
    assert t.grad is not None and abs(lt.item() - lb.item()) < 1e-6
    small = torch.rand(1, 3, 8, 20, device=dev)
    assert torch.isfinite(SL.SSIMLoss(valid=True, clamp=False)(small, small.clone()))
    assert spy == []
    # the switch
    monkeypatch.setattr(SL, "KERNELS", False)
    mod(pred, gt)
    assert spy == []
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from dehaze_hip import ssim_loss; "
                        "assert ssim_loss.KERNELS is False" % PKG], env=dict(os.environ, DHZ_SSIM_LOSS="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 5. the steps
def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def ffa_step(dev, mode):
    """one ffa_train_step on a freshly seeded FFA(3, 1) at 2 x 3 x 32 x 32; mode: "kernels", "aten", "none" (ssim_loss=None) or "plain"
    (without the new keywords)"""
    from dehaze_hip import ssim_loss as SL
    from dehaze_hip.ffa import FFA
    from dehaze_hip.train import FlatAdamW, ffa_train_step
    g = torch.Generator().manual_seed(7)                               # tests/test_gpu_perloss.py's step_data and seeded_ffa(blocks=1)
    gt = torch.rand(2, 3, 32, 32, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    seed_all(1234)
    net = FFA(gps=3, blocks=1).to(dev)
    opt = FlatAdamW(net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    net.train()
    mod = SL.SSIMLoss()
    old = SL.KERNELS
    try:
        SL.KERNELS = mode != "aten"
        if mode == "plain":
            out = ffa_train_step(net, None, opt, None, hazy.to(dev), gt.to(dev))
        elif mode == "none":
            out = ffa_train_step(net, None, opt, None, hazy.to(dev), gt.to(dev), ssim_loss=None, w_ssim=0.1)
        else:
            out = ffa_train_step(net, None, opt, None, hazy.to(dev), gt.to(dev), ssim_loss=mod, w_ssim=0.1)
    finally:
        SL.KERNELS = old
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in net.named_parameters()}
    return out, mod.last_value, grads, params


def uformer_step(dev, mode):
    """one train_step (Charbonnier + the term, w_cr = 0) on a freshly seeded E = 32 model at 1 x 3 x 64 x 64"""
    import My_model_1 as M1
    from losses import CharbonnierLoss
    from dehaze_hip import ssim_loss as SL
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    seed_all(1234)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=4, token_projection='linear', token_mlp='leff', drop_path_rate=0.).to(dev)
    opt = FlatAdamW(model)
    model.train()
    gt, hazy = synthetic_batch(1, 64, seed=5)
    mod = SL.SSIMLoss(clamp=False)
    old = SL.KERNELS
    seed_all(77)                                                       # the sampled keys of the ProbSparse attention
    try:
        SL.KERNELS = mode != "aten"
        args = (model, CharbonnierLoss(), None, opt, None, hazy.to(dev), gt.to(dev))
        if mode == "plain":
            out = train_step(*args, w_char=1.0, w_cr=0)
        elif mode == "none":
            out = train_step(*args, w_char=1.0, w_cr=0, ssim_loss=None, w_ssim=0.1)
        else:
            out = train_step(*args, w_char=1.0, w_cr=0, ssim_loss=mod, w_ssim=0.1)
    finally:
        SL.KERNELS = old
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    return out, mod.last_value, grads, params


@pytest.mark.parametrize("step", [ffa_step, uformer_step], ids=["ffa_train_step", "train_step"])
def test_steps_with_the_term(dev, spy, step):
    from dehaze_hip import ops
    (loss, first, third), term, grads, _ = step(dev, "kernels")
    assert spy.count("dhz_ssim_loss_fwd") == 1 and spy.count("dhz_ssim_loss_bwd") == 1
    assert third is None and term is not None and 0 < term.item() < 1
    print(f"{step.__name__}: loss {loss.item():.6f} = {first.item():.6f} + 0.1 * {term.item():.6f}")
    assert abs(loss.item() - (first.item() + 0.1 * term.item())) < 1e-6
    del spy[:]
    (loss_a, first_a, _), term_a, grads_a, _ = step(dev, "aten")
    assert "dhz_ssim_loss_fwd" not in spy and "dhz_ssim_loss_bwd" not in spy
    assert abs(loss.item() - loss_a.item()) < 1e-5 and abs(term.item() - term_a.item()) < 1e-6
    assert grads.keys() == grads_a.keys() and len(grads) > 10
    for n in grads:                                                    # tests/test_gpu_perloss.py's route comparison: atol 2e-4, rtol 1e-3
        assert torch.allclose(grads[n], grads_a[n], atol=2e-4, rtol=1e-3), (n, (grads[n] - grads_a[n]).abs().max())
    # the term moves the gradients: the comparison above is not one of two steps that ignore it
    (_, _, _), _, grads_p, _ = step(dev, "plain")
    assert any(not torch.allclose(grads[n], grads_p[n], atol=2e-4, rtol=1e-3) for n in grads)
    # ssim_loss=None: the step as it was, bit for bit (deterministic mode: without it the step's own fp32 atomics move the last bits)
    try:
        ops.set_deterministic(True)
        out_n, _, grads_n, params_n = step(dev, "none")
        out_p, _, grads_p, params_p = step(dev, "plain")
        out_k1, term1, _, params_k1 = step(dev, "kernels")
        out_k2, term2, _, params_k2 = step(dev, "kernels")
    finally:
        ops.set_deterministic(False)
    assert all(torch.equal(a, b) for a, b in zip(out_n[:2], out_p[:2])) and out_n[2] is None and out_p[2] is None
    assert all(torch.equal(grads_n[n], grads_p[n]) for n in grads_p) and all(torch.equal(params_n[n], params_p[n]) for n in params_p)
    # and with the term the deterministic mode holds bit for bit
    assert torch.equal(out_k1[0], out_k2[0]) and torch.equal(term1, term2)
    assert all(torch.equal(params_k1[n], params_k2[n]) for n in params_k1)


# ------------------------------------------------------------------------------------------------ 6. command lines
def test_ffa_main_command_line_with_the_term(tmp_path):
    cmd = [sys.executable, "FFA_main.py", "--synthetic", "4", "--val_synthetic", "2", "--steps", "3", "--eval_step", "3", "--blocks", "1",
           "--crop", "--crop_size", "32", "--ssimloss", "0.1", "--log_every", "1", "--model_dir", str(tmp_path) + os.sep]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    num = r"([-+]?(?:nan|inf|[0-9.]+(?:e[-+]?[0-9]+)?))"
    rows = re.findall(r"train loss : %s\| ssim loss : %s" % (num, num), r.stdout)
    assert len(rows) == 3, r.stdout[-2000:]
    assert all(math.isfinite(float(a)) and math.isfinite(float(b)) and 0 < float(b) < 1 and float(a) > 0.1 * float(b) for a, b in rows), rows


def test_my_train_command_line_with_the_term():
    cmd = [sys.executable, os.path.join(PKG, "My_train.py"), "--arch", "Uformer", "--train_ps", "64", "--embed_dim", "32", "--batch_size", "2",
           "--synthetic", "4", "--val_synthetic", "2", "--nepoch", "1", "--w_loss_ssim", "0.1", "--w_loss_vgg7", "0", "--log_every", "1",
           "--env", "_ssim_loss_test"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"loss:([0-9.eE+-]+|nan|inf) = Charbonnier:([0-9.eE+-]+|nan|inf); contrast:[0-9.eE+-]+; ssim:([0-9.eE+-]+|nan|inf)", r.stdout)
    assert len(rows) == 2, r.stdout[-2000:]                            # two steps of two pairs
    for loss, rec, term in rows:
        loss, rec, term = float(loss), float(rec), float(term)
        assert math.isfinite(loss) and 0 < term < 1 and abs(loss - (rec + 0.1 * term)) < 1e-4, rows
