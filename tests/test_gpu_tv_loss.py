"""The total-variation losses on the device: dhz_tv_loss_workspace_bytes / dhz_tv_loss_fwd / dhz_tv_loss_bwd (csrc/tv_loss.hip),
dehaze_hip.tv_loss (tv_loss, TVLoss, TVTerm), the term in train_step / ffa_train_step and the two command lines.

The oracle is the reference's own losses.py under float64 autograd (tests/golden/tv_loss.npz, gen_golden_tv_loss.py); on the cases with
zero sites (`clamped`, `flat`), where the reference's gradient is NaN, it is the masked formula's gradient, which the generator asserts to
equal the reference's wherever that is finite.  The bounds are measured on the reference, not on the code under test: the value within
max(2 |v32_ref - v64|, fp32 spacing of v64), the gradient within max(2 x the reference's own fp32 gradient error, 2^-22 max|g64|) - the
yardsticks of tests/test_gpu_ssim_loss.py (the factor 2 covers another summation order, the floors the fp32 roundings of the stored and of
the compared result).
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
NAMES = ("one_site", "row", "col", "odd", "two_bands", "clamped", "flat")
CASES = [(n, f) for n in NAMES for f in ("beta", "sq")]
FORM = {"beta": 0, "sq": 1}
COEFF = {"beta": 5.0, "sq": 1.0}                 # the reference's defaults: reg_coeff = 5, tv_loss_weight = 1


@pytest.fixture(scope="module")
def gold(golden):
    return golden("tv_loss")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def raw(x, form, g=1.0, backward=True):
    """the three entries called directly: (loss, dx); loss and dx start as NaN, so a pixel the backward does not WRITE shows"""
    from dehaze_hip import _lib
    lib = _lib.load()
    B, C, H, W = x.shape
    nbytes = lib.dhz_tv_loss_workspace_bytes(B, C, H, W)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    loss = torch.full((), float("nan"), device=x.device)
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("dhz_tv_loss_fwd", loss.data_ptr(), x.data_ptr(), B, C, H, W, FORM[form], 0.5, COEFF[form], ws.data_ptr(), nbytes, s)
    if not backward:
        return loss, None
    gl = torch.tensor(float(g), device=x.device)
    dx = torch.full_like(x, float("nan"))
    _lib.call("dhz_tv_loss_bwd", dx.data_ptr(), gl.data_ptr(), x.data_ptr(), B, C, H, W, FORM[form], 0.5, COEFF[form], s)
    return loss, dx


def case(gold, name, form, dev):
    key = f"{name}_{form}"
    x = torch.from_numpy(gold[name + "_x"]).to(dev)
    g64 = gold[key + "_grad"].astype(np.float64)
    v64, v32 = float(gold[key + "_f64"]), float(gold[key + "_f32"])
    vbound = max(2 * abs(v32 - v64), float(np.spacing(np.float32(v64))))
    gbound = max(2 * float(gold[key + "_grad_err_f32"]), 2.0 ** -22 * np.abs(g64).max())
    return x, g64, v64, vbound, gbound


# ------------------------------------------------------------------------------------------------ 1. raw ABI against the golden
@pytest.mark.parametrize("name,form", CASES)
def test_raw_entries_against_the_float64_reference(gold, dev, name, form):
    x, g64, v64, vbound, gbound = case(gold, name, form, dev)
    loss, dx = raw(x, form)
    verr = abs(float(loss.double().item()) - v64)
    assert torch.isfinite(dx).all()                                    # every pixel written, the pixels of the zero sites included
    gerr = np.abs(dx.double().cpu().numpy() - g64).max()               # all pixels: on clamped / flat against the masked formula
    print(f"{name}/{form}: value err {verr:.3e} (bound {vbound:.3e}); grad err {gerr:.3e} = {gerr / np.abs(g64).max():.2e} of max|grad| "
          f"(bound {gbound:.3e} = {gbound / np.abs(g64).max():.2e})")
    assert verr <= vbound
    assert gerr <= gbound
    if name in ("clamped", "flat") and form == "beta":
        assert gold[name + "_beta_nan_mask"].sum() >= 3                # the pixels the literal formula loses are among the compared ones
    # the forward alone writes the same bits; the upstream gradient scales dx (a power of two: exactly)
    assert torch.equal(raw(x, form, backward=False)[0], loss)
    assert torch.equal(raw(x, form, g=0.25)[1], 0.25 * dx)


# ------------------------------------------------------------------------------------------------ 2. reproducibility
@pytest.mark.parametrize("form", ["beta", "sq"])
def test_bits_do_not_depend_on_the_grid_or_the_mode(gold, dev, form):
    from dehaze_hip import ops
    x, *_ = case(gold, "two_bands", form, dev)
    loss0, dx0 = raw(x, form)
    for level in (None, 8, 9):
        with reserved_grid(level):
            for _ in range(3):
                loss, dx = raw(x, form)
                assert torch.equal(loss, loss0) and torch.equal(dx, dx0), level
    try:
        ops.set_deterministic(True)
        for _ in range(3):
            loss, dx = raw(x, form)
            assert torch.equal(loss, loss0) and torch.equal(dx, dx0)
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 3. the module
@pytest.fixture
def spy(monkeypatch):
    from dehaze_hip import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return names


def evaluate(TV, x, form):
    return TV.tv_loss(x) if form == "beta" else TV.TVLoss()(x)


@pytest.mark.parametrize("form", ["beta", "sq"])
def test_module_against_the_aten_route(gold, dev, spy, monkeypatch, form):
    from dehaze_hip import tv_loss as TV
    x, g64, v64, vbound, gbound = case(gold, "odd", form, dev)
    a = x.clone().requires_grad_(True)
    la = evaluate(TV, a, form)
    assert la.dim() == 0 and la.is_cuda and la.dtype == torch.float32
    la.backward()
    assert spy == ["dhz_tv_loss_fwd", "dhz_tv_loss_bwd"]
    del spy[:]
    monkeypatch.setattr(TV, "KERNELS", False)                          # what DHZ_TV_LOSS=0 sets
    b = x.clone().requires_grad_(True)
    lb = evaluate(TV, b, form)
    lb.backward()
    assert spy == []
    verr, gerr = abs(la.item() - lb.item()), (a.grad - b.grad).abs().max().item()
    print(f"odd/{form}: kernels vs ATen: value {verr:.3e} (bound {2 * vbound:.3e}), grad {gerr:.3e} (bound {2 * gbound:.3e})")
    assert verr <= 2 * vbound and gerr <= 2 * gbound                   # each route within its bound of the reference
    # and each of them against the reference
    for l, t in ((la, a), (lb, b)):
        assert abs(float(l.double().item()) - v64) <= vbound and np.abs(t.grad.double().cpu().numpy() - g64).max() <= gbound


def test_module_routing(gold, dev, spy, monkeypatch):
    from dehaze_hip import tv_loss as TV
    x, *_ = case(gold, "clamped", "beta", dev)
    # a column-sliced view gives what its contiguous copy gives; TVTerm keeps the value; a weight scales the sq form
    wide = torch.cat([x[..., :1], x], 3)
    view = wide[..., 1:]
    assert not view.is_contiguous() and torch.equal(view, x)
    term = TV.TVTerm("beta")
    a, b = view.detach().requires_grad_(True), x.clone().requires_grad_(True)
    la, lb = term(a), TV.tv_loss(b)
    assert torch.equal(term.last_value, la.detach())
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad) and torch.isfinite(a.grad).all()
    assert abs(TV.TVLoss(3)(x).item() - 3 * TV.TVTerm("sq")(x).item()) < 1e-6
    assert spy == ["dhz_tv_loss_fwd", "dhz_tv_loss_fwd", "dhz_tv_loss_bwd", "dhz_tv_loss_bwd", "dhz_tv_loss_fwd", "dhz_tv_loss_fwd"]
    del spy[:]
    # the kernel route is once differentiable: a double backward raises instead of treating dx as a constant
    c, w = x.clone().requires_grad_(True), torch.ones((), device=dev, requires_grad=True)
    gc, = torch.autograd.grad(TV.tv_loss(c) * w, c, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gc.sum().backward()
    del spy[:]
    # no gradient wanted: the forward alone, the same bits
    with torch.no_grad():
        assert torch.equal(TV.tv_loss(x), lb.detach())
    assert spy == ["dhz_tv_loss_fwd"]
    del spy[:]
    # bf16, a plane without a site: the ATen formula, without error
    for form in ("beta", "sq"):
        h = x.bfloat16().requires_grad_(True)
        l16 = TV.TVTerm(form)(h)
        l16.backward()
        assert l16.dtype == torch.bfloat16 and torch.isfinite(l16) and torch.isfinite(h.grad).all()
    thin = torch.rand(1, 1, 1, 5, device=dev, requires_grad=True)
    lt = TV.tv_loss(thin)
    lt.backward()
    assert lt.item() == 0 and bool((thin.grad == 0).all()) and torch.isnan(TV.TVLoss()(thin.detach()))
    assert spy == []
    # the switch
    monkeypatch.setattr(TV, "KERNELS", False)
    TV.tv_loss(x)
    TV.TVLoss()(x)
    assert spy == []
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); from dehaze_hip import tv_loss; "
                        "assert tv_loss.KERNELS is False" % PKG], env=dict(os.environ, DHZ_TV_LOSS="0"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 4. the steps
def seed_all(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def ffa_steps(dev, form, mode, steps=1):
    """`steps` ffa_train_step calls on a freshly seeded FFA(3, 1) at 2 x 3 x 32 x 32 (the net of tests/test_gpu_ssim_loss.py); mode:
    "kernels", "aten" or "plain" (without the new keywords)"""
    from dehaze_hip import tv_loss as TV
    from dehaze_hip.ffa import FFA
    from dehaze_hip.train import FlatAdamW, ffa_train_step
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(2, 3, 32, 32, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    seed_all(1234)
    net = FFA(gps=3, blocks=1).to(dev)
    opt = FlatAdamW(net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    net.train()
    term = TV.TVTerm(form)
    old = TV.KERNELS
    try:
        TV.KERNELS = mode != "aten"
        for _ in range(steps):
            if mode == "plain":
                out = ffa_train_step(net, None, opt, None, hazy.to(dev), gt.to(dev))
            else:
                out = ffa_train_step(net, None, opt, None, hazy.to(dev), gt.to(dev), tv_term=term, w_tv=0.1)
    finally:
        TV.KERNELS = old
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in net.named_parameters()}
    return out, term.last_value, grads, params


def uformer_steps(dev, form, mode, steps=1):
    """`steps` train_step calls (Charbonnier + the term on the clamped prediction, w_cr = 0) on a freshly seeded E = 32 model at
    1 x 3 x 64 x 64"""
    import My_model_1 as M1
    from losses import CharbonnierLoss
    from dehaze_hip import tv_loss as TV
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    seed_all(1234)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=4, token_projection='linear', token_mlp='leff', drop_path_rate=0.).to(dev)
    opt = FlatAdamW(model)
    model.train()
    gt, hazy = synthetic_batch(1, 64, seed=5)
    term = TV.TVTerm(form)
    old = TV.KERNELS
    seed_all(77)                                                       # the sampled keys of the ProbSparse attention
    try:
        TV.KERNELS = mode != "aten"
        args = (model, CharbonnierLoss(), None, opt, None, hazy.to(dev), gt.to(dev))
        for _ in range(steps):
            if mode == "plain":
                out = train_step(*args, w_char=1.0, w_cr=0)
            else:
                out = train_step(*args, w_char=1.0, w_cr=0, tv_term=term, w_tv=0.1)
    finally:
        TV.KERNELS = old
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    return out, term.last_value, grads, params


@pytest.mark.parametrize("form", ["beta", "sq"])
@pytest.mark.parametrize("step", [ffa_steps, uformer_steps], ids=["ffa_train_step", "train_step"])
def test_steps_with_the_term(dev, spy, step, form):
    from dehaze_hip import ops
    (loss, first, third), term, grads, _ = step(dev, form, "kernels")
    assert spy.count("dhz_tv_loss_fwd") == 1 and spy.count("dhz_tv_loss_bwd") == 1
    assert third is None and term is not None and term.item() > 0
    print(f"{step.__name__}/{form}: loss {loss.item():.6f} = {first.item():.6f} + 0.1 * {term.item():.6f}")
    assert abs(loss.item() - (first.item() + 0.1 * term.item())) < 1e-6
    assert all(torch.isfinite(g).all() for g in grads.values())
    del spy[:]
    (loss_a, _, _), term_a, grads_a, _ = step(dev, form, "aten")
    assert "dhz_tv_loss_fwd" not in spy and "dhz_tv_loss_bwd" not in spy
    assert abs(loss.item() - loss_a.item()) < 1e-5 and abs(term.item() - term_a.item()) < 1e-5
    assert grads.keys() == grads_a.keys() and len(grads) > 10
    for n in grads:                                                    # the suite's route comparison: atol 2e-4, rtol 1e-3
        assert torch.allclose(grads[n], grads_a[n], atol=2e-4, rtol=1e-3), (n, (grads[n] - grads_a[n]).abs().max())
    # the term moves the gradients: the comparison above is not one of two steps that ignore it
    _, term_p, grads_p, _ = step(dev, form, "plain")
    assert term_p is None
    assert any(not torch.allclose(grads[n], grads_p[n], atol=2e-4, rtol=1e-3) for n in grads)
    # with the deterministic mode, two 3-step runs are bit-equal
    try:
        ops.set_deterministic(True)
        out_1, term_1, _, params_1 = step(dev, form, "kernels", steps=3)
        out_2, term_2, _, params_2 = step(dev, form, "kernels", steps=3)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(out_1[0], out_2[0]) and torch.equal(term_1, term_2) and torch.isfinite(out_1[0])
    assert all(torch.equal(params_1[n], params_2[n]) for n in params_1)


# ------------------------------------------------------------------------------------------------ 5. command lines
NUM = r"([-+]?(?:nan|inf|[0-9.]+(?:e[-+]?[0-9]+)?))"


def test_my_train_command_line_with_the_term():
    """the run whose first step turns every weight into NaN under the literal reference formula: the term sees a clamped prediction"""
    cmd = [sys.executable, os.path.join(PKG, "My_train.py"), "--arch", "Uformer", "--train_ps", "64", "--embed_dim", "32", "--batch_size", "2",
           "--synthetic", "8", "--val_synthetic", "2", "--nepoch", "1", "--w_loss_vgg7", "0", "--w_loss_tv", "0.1", "--tv_form", "beta",
           "--log_every", "1", "--env", "_tv_loss_test"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"loss:%s = Charbonnier:%s; contrast:[0-9.eE+-]+; tv:%s" % (NUM, NUM, NUM), r.stdout)
    assert len(rows) == 4, r.stdout[-2000:]                            # four steps of two pairs
    for loss, rec, term in rows:
        loss, rec, term = float(loss), float(rec), float(term)
        assert math.isfinite(loss) and math.isfinite(term) and term > 0 and abs(loss - (rec + 0.1 * term)) < 1e-4, rows
    assert all(math.isfinite(float(v)) for v in re.findall(r"PSNR: %s" % NUM, r.stdout))


def test_ffa_main_command_line_with_the_term(tmp_path):
    cmd = [sys.executable, "FFA_main.py", "--synthetic", "4", "--val_synthetic", "2", "--steps", "3", "--eval_step", "3", "--blocks", "1",
           "--crop", "--crop_size", "32", "--tvloss", "0.1", "--log_every", "1", "--model_dir", str(tmp_path) + os.sep]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = re.findall(r"train loss : %s\| tv loss : %s" % (NUM, NUM), r.stdout)
    assert len(rows) == 3, r.stdout[-2000:]
    assert all(math.isfinite(float(a)) and math.isfinite(float(b)) and float(b) > 0 and float(a) > 0.1 * float(b) for a, b in rows), rows
