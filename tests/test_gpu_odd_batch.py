"""-m gpu: 64 x 64 patches at batch 1 and batch 3 - the 4 x 4 bottleneck then holds 16 and 48 tokens, a 16-token tail for every
token-Linear weight gradient - against the CPU oracle, through train_step and through the command line.  Recipes and tolerances are
those of tests/test_gpu_win4_model.py (_grads_vs_oracle; its three-step test, which has the numbers of tests/test_gpu_model.py)."""
import math
import os
import re
import subprocess
import sys
import warnings

import pytest
import torch

from oracle import uformer_oracle as O
from test_gpu_win4_model import PKG, _grads_vs_oracle, _pair, seed_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def _model(embed_dim, dev):
    import My_model_1 as M1
    seed_all(1234)
    model = M1.Uformer(img_size=64, embed_dim=embed_dim, win_size=8, token_projection='linear', token_mlp='leff', drop_path_rate=0.).to(dev)
    assert model.conv.blocks[0].win_size == 4 and model.conv.blocks[0].input_resolution == (4, 4)
    P = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    return model, P


# ----------------------------------------------------------------------------- 6. gradients of the whole model
@pytest.mark.parametrize("embed_dim,B", [(32, 1), (32, 3), (16, 3)])          # embed_dim 16: the narrow (16-wide) kernel's tail
def test_model_grads_64px_odd_batch_vs_oracle(dev, embed_dim, B):
    model, P = _model(embed_dim, dev)
    gt, hazy = _pair(B, 64, 11 + B)
    _grads_vs_oracle(model, P, hazy, gt, dev, img_size=64, win=8, drop_path_rate=0.)


# ----------------------------------------------------------------------------- 7. three optimisation steps
def test_train_steps_64px_batch3_vs_oracle(dev):
    """three train_step calls (Charbonnier, FlatAdamW) vs the oracle + torch.optim.AdamW: loss 5e-5, parameters 5e-4
    (tests/test_gpu_model.py::test_training_steps_vs_oracle)"""
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    model, P = _model(32, dev)
    ref_params = [P[n] for n, _ in model.named_parameters()]
    opt_ref = torch.optim.AdamW(ref_params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    opt = FlatAdamW(model, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    gt, hazy = _pair(3, 64, 7)
    gtd, hazyd = gt.to(dev), hazy.to(dev)
    crit = CharbonnierLoss()
    model.train()
    for step in range(3):
        torch.manual_seed(500 + step)
        loss, _, _ = train_step(model, crit, None, opt, None, hazyd, gtd, w_cr=0.0)
        torch.manual_seed(500 + step)
        opt_ref.zero_grad()
        loss_ref = O.charbonnier(torch.clamp(O.uformer_forward(P, hazy, img_size=64, win=8, drop_path_rate=0., training=True), 0, 1), gt)
        loss_ref.backward()
        opt_ref.step()
        print(f"step {step}: loss {loss.item():.7f} oracle {loss_ref.item():.7f}")
        assert abs(loss.item() - loss_ref.item()) < 5e-5, (step, loss.item(), loss_ref.item())
    sd = model.state_dict()
    worst = max((sd[k].cpu() - P[k].detach()).abs().max().item() for k in P if P[k].dtype.is_floating_point)
    print(f"worst parameter difference {worst:.3e}")
    assert worst < 5e-4, worst


@pytest.mark.parametrize("B", [1, 3])
def test_full_train_step_64px_odd_batch_runs(dev, B):
    """the whole step - Charbonnier + contrastive loss + AdamW, DropPath on - refuses nothing at an odd batch"""
    import My_CR
    import My_model_1 as M1
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    seed_all(1234)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev)
    model.train()
    opt = FlatAdamW(model)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cr = My_CR.ContrastLoss().to(dev)
    gt, hazy = _pair(B, 64, 3)
    before = model.conv.blocks[0].mlp.linear1[0].weight.detach().clone()
    loss, lrec, lcr = train_step(model, CharbonnierLoss(), cr, opt, None, hazy.to(dev), gt.to(dev))
    assert math.isfinite(loss.item()) and math.isfinite(lrec.item()) and math.isfinite(lcr.item())
    after = model.conv.blocks[0].mlp.linear1[0].weight.detach()
    assert torch.isfinite(after).all() and not torch.equal(before, after)          # the bottleneck's weights moved


# ----------------------------------------------------------------------------- 8. command line
def test_my_train_64px_partial_last_batch_command_line():
    """7 patches at batch size 4: batches of 4 and 3 (drop_last=False)"""
    cmd = [sys.executable, os.path.join(PKG, "My_train.py"), "--train_ps", "64", "--embed_dim", "32", "--batch_size", "4",
           "--synthetic", "7", "--nepoch", "1", "--w_loss_vgg7", "0"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"loss:([0-9.eE+-]+|nan|inf)", r.stdout)]
    assert losses and all(math.isfinite(x) for x in losses), r.stdout[-2000:]
