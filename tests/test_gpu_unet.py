"""-m gpu: the UNet baseline (dehaze_hip/unet.py) on the kernels - the model against the reference fixture, training steps, deterministic
mode, the library fallback and the command line (second half of the file) - and, first, the LeakyReLU(0.01) store of the
3x3 convolution, forward (with the block's conv11 branch added in the same store) and backward-data (derivative factor 1 / 0.01 from
the sign of the saved activation), against float64 on the CPU at the tolerances of tests/test_gpu_winograd.py (forward atol 2e-5,
backward-data atol 5e-5, rtol 1e-4), and the two layout copies between tokens and the blocked layout, bit for bit against torch."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def blocked(t):
    B, C, H, W = t.shape
    return t.view(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def plain(tb):
    B, CG, H, W, _ = tb.shape
    return tb.permute(0, 1, 4, 2, 3).reshape(B, CG * 8, H, W)


# seeds whose float64 pre-activations stay 2e-4 away from zero (found on the CPU; the guard below holds them to 1e-5).  Beside the two
# C == K cases: C = 2K and K = 2C (the decoder and encoder blocks of the UNet: a channel count swapped in the indexing of bias, mask
# or addend shows only there), five 8 x 8 images (a ragged last block of four, forward and backward), and maps with H != W.
LEAKY_SEEDS = {(2, 32, 32, 16, 16): 241, (1, 64, 64, 8, 8): 457, (1, 64, 32, 16, 16): 38, (1, 32, 64, 16, 16): 37, (5, 64, 32, 8, 8): 21,
               (1, 32, 32, 16, 32): 10, (1, 32, 32, 32, 16): 33}


@pytest.mark.parametrize("B,C,K,H", [(2, 32, 32, 16), (1, 64, 64, 8), (1, 64, 32, 16), (1, 32, 64, 16), (5, 64, 32, 8)])
def test_leaky_store_forward_and_backward(B, C, K, H):
    leaky_store_case(B, C, K, H, H)


@pytest.mark.parametrize("H,W", [(16, 32), (32, 16)])
def test_leaky_store_forward_and_backward_nonsquare(H, W):
    leaky_store_case(1, 32, 32, H, W)


def close(what, got, want, atol, rtol):
    """torch.allclose with the worst error printed first"""
    print(f"{what}: worst error {(got - want).abs().max().item():.3e} (atol {atol:.0e}, rtol {rtol:.0e})")
    assert torch.allclose(got, want, atol=atol, rtol=rtol), (what, (got - want).abs().max())


def leaky_store_case(B, C, K, H, W):
    from dehaze_hip import _lib
    tag = f"winograd_conv3x3_act B={B} C={C} K={K} {H}x{W}"
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(LEAKY_SEEDS[(B, C, K, H, W)])
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    b = 0.1 * torch.randn(K, generator=g)
    add = torch.randn(B, K, H, W, generator=g)
    pre = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert pre.abs().min().item() > 1e-5, "a pre-activation of the float64 reference within 1e-5 of zero: reseed"
    act = F.leaky_relu(pre, 0.01)
    wd = w.cuda()
    up = torch.empty(16 * K * C, device="cuda")
    _lib.call("dhz_winograd_prepack", wd.data_ptr(), up.data_ptr(), K, C, 0, s)
    xb, addb, bd = blocked(x).cuda(), blocked(add).cuda(), b.cuda()
    yb = torch.full((B, K // 8, H, W, 8), float("nan"), device="cuda")
    # forward: y = leaky(conv + bias)
    _lib.call("dhz_winograd_conv3x3_act", xb.data_ptr(), up.data_ptr(), bd.data_ptr(), 0, None, None, yb.data_ptr(), B, H, W, C, K, s)
    y = plain(yb).cpu()
    close(tag + " forward", y, act.float(), 2e-5, 1e-4)
    act_dev = yb.clone()                                    # the saved activation of the backward below
    # ... + addend in the same store (the block's conv11 branch)
    _lib.call("dhz_winograd_conv3x3_act", xb.data_ptr(), up.data_ptr(), bd.data_ptr(), 0, None, addb.data_ptr(), yb.data_ptr(), B, H, W, C, K, s)
    y = plain(yb).cpu()
    want = (act + add.double()).float()
    close(tag + " forward + addend", y, want, 2e-5, 1e-4)
    # backward-data of a convolution ABOVE this activation: dpre = (conv_transpose(dz, w2) + addend) * leaky'(pre), the factor taken
    # from the sign of the saved activation (K channels here are that convolution's input channels)
    w2 = torch.randn(C, K, 3, 3, generator=g) * (2.0 / (9 * K)) ** 0.5
    dz = torch.randn(B, C, H, W, generator=g)
    w2d = w2.cuda()
    upt = torch.empty(16 * K * C, device="cuda")
    _lib.call("dhz_winograd_prepack", w2d.data_ptr(), upt.data_ptr(), K, C, 1, s)
    dzb = blocked(dz).cuda()
    gb = torch.full((B, K // 8, H, W, 8), float("nan"), device="cuda")
    slope = torch.where(pre > 0, 1.0, 0.01)
    refd = F.conv_transpose2d(dz.double(), w2.double(), padding=1)
    for addend in (None, addb):
        _lib.call("dhz_winograd_conv3x3_act", dzb.data_ptr(), upt.data_ptr(), None, 1, act_dev.data_ptr(),
                  None if addend is None else addend.data_ptr(), gb.data_ptr(), B, H, W, C, K, s)
        want = ((refd + (0 if addend is None else add.double())) * slope).float()
        got = plain(gb).cpu()
        close(tag + " backward, mask" + ("" if addend is None else " + addend"), got, want, 5e-5, 1e-4)
    # the mixed-up argument sets are refused
    lib = _lib.load()
    assert lib.dhz_winograd_conv3x3_act(xb.data_ptr(), up.data_ptr(), bd.data_ptr(), 1, act_dev.data_ptr(), None, gb.data_ptr(), B, H, W, C, K, s) == -22
    assert lib.dhz_winograd_conv3x3_act(xb.data_ptr(), up.data_ptr(), None, 0, act_dev.data_ptr(), None, gb.data_ptr(), B, H, W, C, K, s) == -22


def test_leaky_and_relu_stores_agree_on_positive_maps():
    """where no pre-activation is negative, the LeakyReLU store and the ReLU store of dhz_winograd_conv3x3 agree bit for bit"""
    from dehaze_hip import _lib
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(11)
    B, C, K, H = 1, 32, 32, 16
    x = torch.rand(B, C, H, H, generator=g)
    w = torch.rand(K, C, 3, 3, generator=g) * 0.05               # all positive: every pre-activation is positive
    wd, xb = w.cuda(), blocked(x).cuda()
    up = torch.empty(16 * K * C, device="cuda")
    _lib.call("dhz_winograd_prepack", wd.data_ptr(), up.data_ptr(), K, C, 0, s)
    ya = torch.empty(B, K // 8, H, H, 8, device="cuda")
    yr = torch.empty_like(ya)
    _lib.call("dhz_winograd_conv3x3_act", xb.data_ptr(), up.data_ptr(), None, 0, None, None, ya.data_ptr(), B, H, H, C, K, s)
    _lib.call("dhz_winograd_conv3x3", xb.data_ptr(), up.data_ptr(), None, 1, None, None, yr.data_ptr(), B, H, H, C, K, s)
    assert (yr > 0).all() and torch.equal(ya, yr)


# ---- the layout copies between tokens [B][HW][C] (row stride ld) and the blocked layout [B][C/8][HW][8], with the ConvBlock's elementwise
# factors folded in (dhz_tokens_to_blocked8 / dhz_blocked8_to_tokens).  Pure data movement plus at most one fp32 operation per element:
# compared bit for bit with torch on the CPU.  (1, 9, 8): one channel group, 18 threads; (3, 64, 40): C no multiple of 32, a ragged last
# workgroup; the model only ever passes ld == ld_add == C and thread counts in whole workgroups.
LAYOUT_SHAPES = [(1, 9, 8), (3, 64, 40), (2, 256, 64)]
LAYOUT_CASES = [(s, 0, 0) for s in LAYOUT_SHAPES] + [(s, 12, 4) for s in LAYOUT_SHAPES[1:]]       # (shape, ld - C, ld_add - C)
CANARY = 64


def to_blocked_ref(tok, B, HW, C):
    return tok.reshape(B, HW, C // 8, 8).permute(0, 2, 1, 3).contiguous()


def strided_tokens(tok, ld):
    """[B*HW, C] values as a view into a NaN-filled [B*HW, ld] buffer on the device; returns (buffer, view)"""
    buf = torch.full((tok.shape[0], ld), float("nan"), device="cuda")
    buf[:, :tok.shape[1]] = tok.cuda()
    return buf, buf[:, :tok.shape[1]]


def call_to_blocked(tokbuf, ld, mask, B, HW, C):
    from dehaze_hip import _lib
    blk = torch.full((B * (C // 8) * HW * 8 + CANARY,), float("nan"), device="cuda")
    _lib.call("dhz_tokens_to_blocked8", tokbuf.data_ptr(), ld, None if mask is None else mask.data_ptr(), blk.data_ptr(), B, HW, C,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(blk[-CANARY:]).all(), "written behind the blocked map"
    return blk[:-CANARY].view(B, C // 8, HW, 8)


def call_to_tokens(blk, addbuf, ld_add, ld, B, HW, C):
    from dehaze_hip import _lib
    out = torch.full((B * HW, ld), float("nan"), device="cuda")
    _lib.call("dhz_blocked8_to_tokens", blk.data_ptr(), None if addbuf is None else addbuf.data_ptr(), ld_add, out.data_ptr(), ld, B, HW, C,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(out[:, C:]).all(), "the padding columns of the token rows were written"
    return out[:, :C]


@pytest.mark.parametrize("shape,pad,pad_add", LAYOUT_CASES)
def test_layout_copies_are_exact(shape, pad, pad_add):
    B, HW, C = shape
    ld, ld_add = C + pad, C + pad_add
    g = torch.Generator().manual_seed(B * 1000 + HW + C + pad)
    tok = torch.randn(B * HW, C, generator=g)
    add = torch.randn(B * HW, C, generator=g)
    mask = torch.randn(B, C // 8, HW, 8, generator=g)
    flat = mask.view(-1)
    planted = torch.tensor([0.0, -0.0, -1e-40, 1e-40])            # zero, minus zero, a negative and a positive denormal
    assert planted[2] < 0 < planted[3]
    for i in range(4):                                             # one of each in the first and in the last float4
        flat[i] = planted[i]
        flat[flat.numel() - 4 + i] = planted[3 - i]
    tokbuf, _ = strided_tokens(tok, ld)
    # tokens -> blocked: a plain copy ...
    want = to_blocked_ref(tok, B, HW, C)
    blk = call_to_blocked(tokbuf, ld, None, B, HW, C)
    assert not torch.isnan(blk).any() and torch.equal(blk.cpu(), want)
    # ... and with the LeakyReLU derivative of the saved activation: one fp32 multiply by the same constant
    blk_m = call_to_blocked(tokbuf, ld, mask.cuda(), B, HW, C)
    want_m = want * torch.where(mask > 0, 1.0, 0.01)
    assert torch.equal(blk_m.cpu().view(torch.int32), want_m.view(torch.int32))
    assert torch.isnan(tokbuf[:, C:]).all()
    # blocked -> tokens: the round trip is the identity; with the addend one fp32 addition
    back = call_to_tokens(blk, None, 0, ld, B, HW, C)
    assert torch.equal(back.cpu(), tok)
    addbuf, _ = strided_tokens(add, ld_add)
    back_a = call_to_tokens(blk, addbuf, ld_add, ld, B, HW, C)
    assert torch.equal(back_a.cpu(), tok + add)
    assert torch.isnan(addbuf[:, C:]).all()


def test_layout_copies_refuse_bad_arguments():
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    B, HW, C = 2, 16, 16
    tok = torch.randn(B * HW, C + 8, device="cuda")
    blk = torch.full((B * HW * (C + 8),), float("nan"), device="cuda")
    out = torch.full((B * HW, C + 8), float("nan"), device="cuda")
    t, k, o = tok.data_ptr(), blk.data_ptr(), out.data_ptr()
    assert lib.dhz_tokens_to_blocked8(t, 12, None, k, B, HW, 12, s) == -22           # C % 8 != 0
    assert lib.dhz_tokens_to_blocked8(t, C - 4, None, k, B, HW, C, s) == -22         # ld < C
    assert lib.dhz_tokens_to_blocked8(t, C + 2, None, k, B, HW, C, s) == -22         # ld % 4 != 0
    assert lib.dhz_tokens_to_blocked8(t + 4, C + 4, None, k, B, HW, C, s) == -22     # pointers 4 bytes off a 16-byte boundary
    assert lib.dhz_tokens_to_blocked8(t, C, k + 4, k, B, HW, C, s) == -22
    assert lib.dhz_tokens_to_blocked8(t, C, None, k + 4, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, None, 0, o, 12, B, HW, 12, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, None, 0, o, C - 4, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, None, 0, o, C + 2, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, t, C - 4, o, C, B, HW, C, s) == -22         # the addend's own row stride
    assert lib.dhz_blocked8_to_tokens(t, t, C + 2, o, C, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t + 4, None, 0, o, C, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, t + 4, C, o, C, B, HW, C, s) == -22
    assert lib.dhz_blocked8_to_tokens(t, None, 0, o + 4, C, B, HW, C, s) == -22
    torch.cuda.synchronize()
    assert torch.isnan(blk).all() and torch.isnan(out).all()


# ---- the module on the kernels (dehaze_hip/unet.py) at dim 32, 1 x 3 x 128 x 128: the smallest input all of whose layers are tiled
import os  # noqa: E402
import random  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
GOLD = os.path.join(ROOT, "tests", "golden", "unet_m1_dim32.npz")
MODEL_SEED, POS_SEED, NPOS = 41, 43, 32


def seeded_unet(dim=32, seed=MODEL_SEED):
    from dehaze_hip.unet import UNet
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return UNet(dim=dim)


def test_unet_forward_and_gradients_against_the_reference_fixture():
    g = np.load(GOLD)
    net = seeded_unet().cuda()
    x, gout = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["gout"]).cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y = net(x)
        (y * gout).sum().backward()
    assert not [w for w in rec if "library" in str(w.message)], [str(w.message) for w in rec]
    yr = torch.from_numpy(g["y"])
    # tests/test_gpu_model.py:69, the Uformer full-model forward tolerance
    assert torch.allclose(y.detach().cpu(), yr, atol=2e-4, rtol=1e-3), (y.detach().cpu() - yr).abs().max()
    named = list(net.named_parameters())
    gn = np.array([float(p.grad.double().norm()) for _, p in named])
    rel = np.abs(gn - g["grad_norm"]) / (g["grad_norm"] + 1e-8)
    print("UNet gradient norms: worst relative error", rel.max())
    assert rel.max() < 5e-3, rel.max()                                 # tests/test_gpu_model.py:85-86
    pg = torch.Generator().manual_seed(POS_SEED)
    worst = 0.0
    for i, (n, p) in enumerate(named):
        pos = torch.randint(p.numel(), (NPOS,), generator=pg)
        got = p.grad.reshape(-1).cpu()[pos].double().numpy()
        ref = g["grad_samples"][i]
        worst = max(worst, np.abs(got - ref).max() / (np.abs(ref).max() + 1e-8))
    print("UNet sampled gradient entries: worst error relative to the parameter's largest sample", worst)
    assert worst < 5e-3, worst                                         # the same 5e-3, per entry against the parameter's scale


def _three_steps(deterministic=False):
    from dehaze_hip import ops
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(2, 3, 128, 128, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    try:
        if deterministic:
            ops.set_deterministic(True)
        net = seeded_unet(seed=1234).cuda()
        opt = FlatAdamW(net, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
        crit = CharbonnierLoss()
        net.train()
        losses = []
        for _ in range(3):
            loss, _, _ = train_step(net, crit, None, opt, None, hazy.cuda(), gt.cuda(), w_cr=0.0)
            losses.append(loss.item())
        return losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, (hazy, gt)
    finally:
        if deterministic:
            ops.set_deterministic(False)


def test_unet_three_train_steps_against_float64_adamw():
    losses, sd, (hazy, gt) = _three_steps()
    ref = seeded_unet(seed=1234).double()
    opt = torch.optim.AdamW(ref.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    for step in range(3):
        opt.zero_grad()
        d = ref(hazy.double()).clamp(0, 1) - gt.double()
        loss = torch.sqrt(d * d + 1e-3 ** 2).mean()                    # CharbonnierLoss, eps 1e-3 (losses.py)
        loss.backward()
        opt.step()
        print("UNet step", step, losses[step], loss.item())
        assert abs(losses[step] - loss.item()) < 5e-5, (step, losses[step], loss.item())       # tests/test_gpu_model.py:215
    worst = max((sd[k].double() - v.detach()).abs().max().item() for k, v in ref.state_dict().items())
    assert worst < 5e-4, worst                                         # tests/test_gpu_model.py:218


def test_unet_deterministic_steps_are_bit_equal():
    la, sa, _ = _three_steps(deterministic=True)
    lb, sb, _ = _three_steps(deterministic=True)
    assert la == lb
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_unet_dim16_falls_back_with_warnings_and_equals_torch():
    from dehaze_hip import ops
    net = seeded_unet(dim=16, seed=5).cuda()
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    ops._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = net(x)
            y2 = net(x)
    msgs = [str(w.message) for w in rec if "library" in str(w.message)]
    assert any("UNet Conv3x3" in m for m in msgs) and any("UNet pool" in m for m in msgs), msgs
    assert len(msgs) == len(set(msgs)), "a layer kind and shape warns once"
    with torch.no_grad():
        yt = net._forward_torch(x)
    assert torch.allclose(y, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y2, yt, atol=2e-4, rtol=1e-3)
    # the fallback's autograd mixes kernel Functions (input projection, conv11, upv) with library layers: gradients equal the torch path's
    gout = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(4)).cuda()
    grads = []
    for fwd in (net, net._forward_torch):
        net.zero_grad(set_to_none=True)
        (fwd(x) * gout).sum().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    for (n, _), ga, gb in zip(net.named_parameters(), *grads):
        scale = gb.abs().max().item()
        assert (ga - gb).abs().max().item() < 5e-3 * scale + 1e-6, (n, (ga - gb).abs().max().item(), scale)


def test_my_train_command_line_unet():
    r = subprocess.run([sys.executable, "My_train.py", "--arch", "UNet", "--train_ps", "128", "--batch_size", "2", "--synthetic", "4",
                        "--nepoch", "1", "--w_loss_vgg7", "0"], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "nan" not in r.stdout.lower() and "inf" not in r.stdout.lower().replace("info", ""), r.stdout[-2000:]
