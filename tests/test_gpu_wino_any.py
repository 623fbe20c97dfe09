"""-m gpu: the F(2x2,3x3) Winograd convolution on maps of any size (dhz_winograd_conv3x3_any, dhz_winograd_conv3x3_any_slices) - ragged
16 x 16 blocks at the right and bottom edges of a map, sixteen 4 x 4 images per block - against float64 conv2d / conv_transpose2d at the
tolerances of tests/test_gpu_winograd.py (forward 2e-5 / 1e-4, backward-data 5e-5 / 1e-4), and the feature engine, the contrastive loss and
the training step at the patch sizes that these entries open (64, 64 x 192, 240, 384 pixels).

Every launch writes into the middle of a larger buffer and reads out_mask / out_addend from the middle of larger buffers; the margins (two
16 x 16 x 8-float blocks on either side) hold a sentinel that is checked word for word afterwards, the output starts as NaN, and the
input's last image ends where its allocation ends: a masked-store bug shows up as a failed comparison.

B, C, K name the kernel's arguments: C input channels, K output channels.  The backward-data modes run the kernel with the
transposed_rot filters of a weight [C, K, 3, 3], i.e. conv_transpose2d of the C-channel input - the same C and K as the forward modes."""
import contextlib
import functools
import math
import os
import re
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD_TOL = (2e-5, 1e-4)
BWD_TOL = (5e-5, 1e-4)
MODES = ("bias_relu", "plain", "mask_addend", "addend")
GUARD = 2 * 16 * 16 * 8          # floats on either side of a guarded tensor
SENTINEL = -7777.25

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _blocked(x):
    from dehaze_hip import _lib
    B, C, H, W = x.shape
    out = torch.empty(B, C // 8, H, W, 8, device=x.device)
    _lib.call("dhz_layout_blocked8", x.contiguous().data_ptr(), out.data_ptr(), B, C, H * W, 1, None, 0, _s())
    return out


def _plain(xb, C):
    from dehaze_hip import _lib
    B, CG, H, W, _ = xb.shape
    out = torch.empty(B, C, H, W, device=xb.device)
    _lib.call("dhz_layout_blocked8", xb.contiguous().data_ptr(), out.data_ptr(), B, C, H * W, 0, None, 0, _s())
    return out


def close(what, got, want, tol):
    print(f"{what}: worst error {(got - want).abs().max().item():.3e} (atol {tol[0]:.0e}, rtol {tol[1]:.0e})")
    assert torch.allclose(got, want, atol=tol[0], rtol=tol[1]), (what, (got - want).abs().max())


def _guarded(src=None, shape=None):
    """(buffer, view): `view` lies GUARD floats inside `buffer`, whose margins hold SENTINEL; the view is a copy of src, or NaN"""
    shape = tuple(src.shape) if src is not None else shape
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=torch.device("cuda:0"))
    view = buf[GUARD:GUARD + n].view(shape)
    view.copy_(src) if src is not None else view.fill_(float("nan"))
    return buf, view


def _guards_intact(what, buf):
    lo, hi = buf[:GUARD], buf[-GUARD:]
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"{what}: a guard word changed"


def _at_end(src):
    """a copy of src whose last element is the last element of its allocation"""
    n = src.numel()
    buf = torch.full((GUARD + n,), SENTINEL, device=src.device)
    view = buf[GUARD:].view(src.shape)
    view.copy_(src)
    return buf, view


@functools.lru_cache(maxsize=None)
def _case(B, C, K, H, W):
    """inputs, packed filters and the float64 references of one shape, computed once and shared by every test of it (never modified)"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7 * C + K + H + 1000 * W + B)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)       # forward: [K out][C in]
    wt = (torch.randn(C, K, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)      # backward-data of a K -> C layer: contraction over C
    b = (0.1 * torch.randn(K, generator=g)).to(dev)
    act = torch.relu(torch.randn(B, K, H, W, generator=g)).to(dev)                    # saved post-ReLU map at the output positions
    add = torch.randn(B, K, H, W, generator=g).to(dev)
    up, upt = torch.empty(16 * K * C, device=dev), torch.empty(16 * K * C, device=dev)
    _lib.call("dhz_winograd_prepack", w.data_ptr(), up.data_ptr(), K, C, 0, _s())
    _lib.call("dhz_winograd_prepack", wt.data_ptr(), upt.data_ptr(), K, C, 1, _s())
    conv = F.conv2d(x.double(), w.double(), padding=1)
    convt = F.conv_transpose2d(x.double(), wt.double(), padding=1)
    ref = {"bias_relu": F.relu(conv + b.double().view(1, K, 1, 1)).float(), "plain": conv.float(),
           "mask_addend": ((convt + add.double()) * (act > 0)).float(), "addend": (convt + add.double()).float()}
    xbuf, xb = _at_end(_blocked(x))
    actbuf, actb = _guarded(_blocked(act))
    addbuf, addb = _guarded(_blocked(add))
    return dict(xbuf=xbuf, xb=xb, up=up, upt=upt, b=b, actbuf=actbuf, actb=actb, addbuf=addbuf, addb=addb, ref=ref)


def _args(c, mode):
    """(filters, bias, relu, mask, addend) of a mode"""
    if mode == "bias_relu":
        return c["up"], c["b"].data_ptr(), 1, None, None
    if mode == "plain":
        return c["up"], None, 0, None, None
    if mode == "mask_addend":
        return c["upt"], None, 0, c["actb"].data_ptr(), c["addb"].data_ptr()
    return c["upt"], None, 0, None, c["addb"].data_ptr()


def _run(entry, c, mode, B, C, K, H, W, S=None):
    """one launch of `entry` (S: its slice count, for the sliced entries) into a guarded NaN output; returns the blocked output"""
    from dehaze_hip import _lib
    up, bias, relu, mask, addend = _args(c, mode)
    ybuf, yb = _guarded(shape=(B, K // 8, H, W, 8))
    if S is None:
        _lib.call(entry, c["xb"].data_ptr(), up.data_ptr(), bias, relu, mask, addend, yb.data_ptr(), B, H, W, C, K, _s())
    else:
        wsbuf, ws = _guarded(shape=(S, B, K // 8, H, W, 8))
        _lib.call(entry, c["xb"].data_ptr(), up.data_ptr(), bias, relu, mask, addend, yb.data_ptr(), ws.data_ptr() if S > 1 else None, S,
                  B, H, W, C, K, _s())
        _guards_intact(f"{entry} workspace", wsbuf)
    what = f"{entry} B={B} C={C} K={K} {H}x{W} {mode}"
    _guards_intact(what + " y", ybuf)
    _guards_intact(what + " out_mask", c["actbuf"])
    _guards_intact(what + " out_addend", c["addbuf"])
    assert bool((c["xbuf"][:GUARD] == SENTINEL).all()), what + ": the words in front of the input changed"
    return yb.clone()


def _tol(mode):
    return FWD_TOL if mode in ("bias_relu", "plain") else BWD_TOL


# ragged blocks: maps of the feature stack at 192 / 240 / 384-pixel patches (24, 12, 30, 15), a non-square map with three images, maps smaller
# than one 2 x 2 tile, odd sizes (an output tile half outside the map), and 17 x 33: one row and one column reach into a new block
RAGGED = [(2, 32, 64, 24, 24), (1, 64, 32, 12, 12), (3, 32, 32, 40, 24), (1, 32, 32, 15, 15), (2, 32, 32, 30, 30), (1, 32, 64, 2, 2),
          (1, 32, 32, 1, 1), (1, 32, 32, 17, 33)]
# sixteen 4 x 4 images per block: one whole block; a partly filled one; one image; two blocks, the second with one image; three blocks (an
# odd count: the second half of the last workgroup stores nothing); more channels than one group and one output-channel block
PACKED4 = [(16, 32, 32, 4, 4), (5, 32, 32, 4, 4), (1, 32, 32, 4, 4), (17, 32, 32, 4, 4), (33, 32, 32, 4, 4), (3, 128, 64, 4, 4)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W", RAGGED + PACKED4)
def test_any_vs_float64(B, C, K, H, W, mode):
    c = _case(B, C, K, H, W)
    yb = _run("dhz_winograd_conv3x3_any", c, mode, B, C, K, H, W)
    close(f"winograd_conv3x3_any B={B} C={C} K={K} {H}x{W} {mode}", _plain(yb, K), c["ref"][mode], _tol(mode))


# shapes the entries without `_any` take: the same launch, the same bits (whole blocks; four 8 x 8 images per block with a partly filled
# last block; a non-square map)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W", [(2, 64, 64, 32, 32), (5, 32, 64, 8, 8), (2, 32, 64, 16, 32)])
def test_any_is_the_old_launch_on_old_shapes(B, C, K, H, W, mode):
    c = _case(B, C, K, H, W)
    old = _run("dhz_winograd_conv3x3", c, mode, B, C, K, H, W)
    close(f"winograd_conv3x3 B={B} C={C} K={K} {H}x{W} {mode}", _plain(old, K), c["ref"][mode], _tol(mode))
    assert torch.equal(_run("dhz_winograd_conv3x3_any", c, mode, B, C, K, H, W), old)
    assert torch.equal(_run("dhz_winograd_conv3x3_any_slices", c, mode, B, C, K, H, W, S=2),
                       _run("dhz_winograd_conv3x3_slices", c, mode, B, C, K, H, W, S=2))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W", [(5, 32, 32, 4, 4), (3, 32, 32, 40, 24), (1, 32, 32, 15, 15)])
def test_any_slices_one_slice_is_the_plain_launch(B, C, K, H, W, mode):
    c = _case(B, C, K, H, W)
    assert torch.equal(_run("dhz_winograd_conv3x3_any_slices", c, mode, B, C, K, H, W, S=1),
                       _run("dhz_winograd_conv3x3_any", c, mode, B, C, K, H, W))


# conv5_1 of 64-pixel patches (six 4 x 4 images: a partly filled block) and of 384-pixel patches (24 x 24), 512 -> 512, in 2 and 4 slices;
# 40 channel groups in 3 slices: the uneven ranges 13, 13, 14
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W,S", [(6, 512, 512, 4, 4, 2), (6, 512, 512, 4, 4, 4), (2, 512, 512, 24, 24, 2), (2, 512, 512, 24, 24, 4),
                                         (2, 320, 32, 12, 12, 3)])
def test_any_slices_vs_float64(B, C, K, H, W, S, mode):
    c = _case(B, C, K, H, W)
    yb = _run("dhz_winograd_conv3x3_any_slices", c, mode, B, C, K, H, W, S=S)
    close(f"winograd_conv3x3_any_slices S={S} B={B} C={C} K={K} {H}x{W} {mode}", _plain(yb, K), c["ref"][mode], _tol(mode))
    # the same call again: the same bits (no atomics, a fixed order of the parts)
    assert torch.equal(_run("dhz_winograd_conv3x3_any_slices", c, mode, B, C, K, H, W, S=S), yb)


# --------------------------------------------------------------------------------------------------------- the feature engine
@contextlib.contextmanager
def _no_library(monkeypatch):
    """inside: ops.warn_library_fallback and torch.nn.functional.conv2d must not be called; yields the list of (entry, H, W) of the
    Winograd launches made"""
    from dehaze_hip import _lib, ops
    launches = []
    real_call = _lib.call

    def call(name, *args):
        if name.startswith("dhz_winograd") and "conv3x3" in name:
            ints = [a for a in args[-7:-1]] if name.endswith("_slices") else [a for a in args[-6:-1]]
            launches.append((name, ints[-4], ints[-3]))           # ..., B, H, W, C, K, stream
        return real_call(name, *args)

    def refuse(what):
        def f(*a, **k):
            raise AssertionError(f"{what} was called")
        return f

    with monkeypatch.context() as m:
        m.setattr(_lib, "call", call)
        m.setattr(ops, "warn_library_fallback", refuse("ops.warn_library_fallback"))
        m.setattr(F, "conv2d", refuse("torch.nn.functional.conv2d"))
        yield launches


def _vgg(dev):
    import My_CR
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return My_CR.Vgg19().to(dev)


@pytest.mark.parametrize("B,H,W", [(6, 4, 4), (2, 24, 24), (40, 24, 24), (3, 12, 12)])
def test_engine_dispatch_follows_the_library_rule(monkeypatch, B, H, W):
    """VggEngine.conv / conv_dgrad of conv5_1 (512 -> 512) on maps only the any-size entries take: the sliced entry with the count of
    dhz_winograd_slices_any where that says more than 1 (few blocks: 6 images of 4 x 4 are one block), the plain one otherwise (40 maps
    of 24 x 24 are 160 blocks), and the bits of that raw call"""
    from dehaze_hip import _lib, vgg as V
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cus = lib.dhz_grid_cus() + lib.dhz_get_reserved_cus()
    S = lib.dhz_winograd_slices_any(B, H, W, 512, 512)
    assert S == V.wino_slices_any_rule(B, H, W, 512, 512, cus)
    nblk = lib.dhz_winograd_any_blocks(B, H, W)
    assert nblk == V.any_blocks(B, H, W) and (S > 1) == (4 * ((nblk + 1) // 2) * 16 <= cus or 2 * ((nblk + 1) // 2) * 16 <= cus)
    net = _vgg(dev)
    eng = net.engine_for(torch.zeros(1, 3, 64, 64, device=dev))
    g = torch.Generator().manual_seed(B + H)
    xb = torch.randn(B, 64, H, W, 8, generator=g).to(dev)
    with _no_library(monkeypatch) as launches:
        yb = eng.conv(12, xb)
        dxb = eng.conv_dgrad(12, yb, below_act=xb, addend=None)
    want = "dhz_winograd_conv3x3_any_slices" if (S > 1 and V.SLICES_ON) else "dhz_winograd_conv3x3_any"
    assert launches == [(want, H, W), (want, H, W)], launches
    uf, ub = eng.packed(12, dev)
    bias = eng.convs[12].bias
    for up, b, relu, mask, got in ((uf, bias.data_ptr(), 1, None, yb), (ub, None, 0, xb.data_ptr(), dxb)):
        ref = torch.full_like(got, float("nan"))
        ws = torch.empty((max(S, 1),) + tuple(got.shape), device=dev)
        _lib.call("dhz_winograd_conv3x3_any_slices", (xb if relu else yb).data_ptr(), up.data_ptr(), b, relu, mask, None, ref.data_ptr(),
                  ws.data_ptr(), S if V.SLICES_ON else 1, B, H, W, 512, 512, _s())
        assert torch.equal(got, ref)


@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 64, 192)])
def test_engine_small_patches_vs_oracle(monkeypatch, B, H, W):
    """64 x 64 (8 x 8 and 4 x 4 maps: both packed forms) and 64 x 192 (8 x 24 and 4 x 12: ragged): features and the input gradient of the
    smooth functional sum_i <R_i, tap_i(a)> against float64 autograd of the CPU oracle; the bounds of test_vgg_engine_backward_smooth_loss
    and of the feature check of test_contrast_loss_engine_vs_oracle (tests/test_gpu_winograd.py)"""
    from oracle import uformer_oracle as O
    dev = torch.device("cuda:0")
    net = _vgg(dev)
    g = torch.Generator().manual_seed(5 + W)
    a = torch.rand(B, 3, H, W, generator=g)
    Wt = O.seeded_vgg_weights(dtype=torch.float64)
    a64 = a.double().requires_grad_()
    feats_o = O.vgg19_features(a64, Wt)
    R = [torch.randn(f.shape, generator=g) for f in feats_o]
    sum((f * r.double()).sum() for f, r in zip(feats_o, R)).backward()

    ad = a.to(dev).requires_grad_()
    Rd = [r.to(dev) for r in R]
    with _no_library(monkeypatch) as launches:
        assert net.engine_for(ad) is not None
        feats = net(ad)
        sum((f * r).sum() for f, r in zip(feats, Rd)).backward()
        torch.cuda.synchronize()
    sizes = {(h, w) for name, h, w in launches if "_any" in name}
    assert (H // 16, W // 16) in sizes, launches                                     # conv5_1 ran the any-size entry
    for f, fo in zip(feats, feats_o):
        assert f.shape == fo.shape
        err = (f.detach().cpu() - fo.detach().float()).abs().max().item()
        print(f"tap {tuple(f.shape)}: worst error {err:.3e} of max {fo.abs().max().item():.3e}")
        assert err < 2e-3 * fo.abs().max().item()
    ref = a64.grad.float()
    err = (ad.grad.cpu() - ref).abs().max().item()
    print(f"input gradient: worst error {err:.3e} of max {ref.abs().max().item():.3e}")
    assert err < 2e-4 * ref.abs().max().item(), (err, ref.abs().max().item())


@pytest.mark.parametrize("n", [240, 384])
def test_engine_large_patches_vs_float64_module(monkeypatch, n):
    """240 x 240 (FFA-Net's crop: maps 240 / 120 / 60 / 30 / 15) and 384 x 384 (conv5_1 on 24 x 24): the whole stack on the Winograd kernels,
    against the same module evaluated by the library in float64 - test_vgg_engine_library_tail_for_untiled_maps, with its bounds"""
    dev = torch.device("cuda:0")
    net = _vgg(dev)
    g = torch.Generator().manual_seed(9)
    a = torch.rand(1, 3, n, n, generator=g).to(dev)
    ae = a.clone().requires_grad_()
    with _no_library(monkeypatch) as launches:
        assert net.engine_for(ae) is not None
        fe = net(ae)
        R = [torch.randn(f.shape, generator=g).to(dev) for f in fe]
        sum((f * r).sum() for f, r in zip(fe, R)).backward()
        torch.cuda.synchronize()
    assert any("_any" in name and (h, w) == (n // 16, n // 16) for name, h, w in launches), launches
    net.double()                                              # float64: the engine does not apply, library convolutions
    a64 = a.double().requires_grad_()
    assert net.engine_for(a64) is None
    f64 = net(a64)
    sum((f * r.double()).sum() for f, r in zip(f64, R)).backward()
    for x, y in zip(fe, f64):
        assert x.shape == y.shape and (x.double() - y).abs().max().item() < 1e-4 * y.abs().max().item()
    err = (ae.grad.double() - a64.grad).abs()
    print(f"{n} px: gradient error mean {err.mean().item():.3e} of {a64.grad.abs().mean().item():.3e}, "
          f"max {err.max().item():.3e} of {a64.grad.abs().max().item():.3e}")
    assert err.mean().item() < 1e-3 * a64.grad.abs().mean().item(), (err.mean().item(), a64.grad.abs().mean().item())
    assert err.max().item() < 5e-2 * a64.grad.abs().max().item(), (err.max().item(), a64.grad.abs().max().item())


@pytest.mark.parametrize("ablation", [False, True])
def test_contrast_loss_64px_vs_oracle(monkeypatch, ablation):
    """ContrastLoss at 64 x 64 against the CPU oracle in float64, with the bounds of test_contrast_loss_engine_vs_oracle
    (tests/test_gpu_winograd.py): loss and distances 2e-4 relative; gradient max 3e-2, mean 8e-3"""
    import My_CR
    from oracle import uformer_oracle as O
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cl = My_CR.ContrastLoss(ablation=ablation).to(dev)
    g = torch.Generator().manual_seed(77)
    a, p, n = (torch.rand(2, 3, 64, 64, generator=g) for _ in range(3))
    Wt = O.seeded_vgg_weights(dtype=torch.float64)
    a64 = a.double().requires_grad_()
    loss_o, ap_o, an_o = O.contrast_loss(a64, p.double(), n.double(), Wt, ablation=ablation)
    loss_o.backward()

    ad = a.to(dev).requires_grad_()
    with _no_library(monkeypatch):
        assert cl.vgg.engine_for(ad) is not None
        loss, ap, an = cl(ad, p.to(dev), n.to(dev))
        loss.backward()
        torch.cuda.synchronize()
    ref = a64.grad.float()
    err = (ad.grad.cpu() - ref).abs()
    print(f"loss {loss.item():.7f} oracle {loss_o.item():.7f}; gradient error max {err.max().item():.3e} of {ref.abs().max().item():.3e}, "
          f"mean {err.mean().item():.3e} of {ref.abs().mean().item():.3e}")
    assert abs(loss.item() - loss_o.item()) < 2e-4 * abs(loss_o.item()), (loss.item(), loss_o.item())
    assert abs(float(ap) - float(ap_o)) < 2e-4 * float(ap_o)
    if not ablation:
        assert abs(float(an) - float(an_o)) < 2e-4 * float(an_o)
    assert err.max().item() < 3e-2 * ref.abs().max().item(), (err.max().item(), ref.abs().max().item())
    assert err.mean().item() < 8e-3 * ref.abs().mean().item(), (err.mean().item(), ref.abs().mean().item())


# --------------------------------------------------------------------------------------------------------- the training step
def _steps_64px(steps, B):
    import My_CR
    import My_model_1 as M1
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    from losses import CharbonnierLoss
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(4321)
        cr = My_CR.ContrastLoss().to(dev)
    opt = FlatAdamW(model)
    gt, hazy = synthetic_batch(B, 64, seed=5)
    gt, hazy = gt.to(dev), hazy.to(dev)
    model.train()
    losses = []
    for step in range(steps):
        torch.manual_seed(1000 + step)
        loss, lrec, lcr = train_step(model, CharbonnierLoss(), cr, opt, None, hazy, gt)
        losses += [loss.detach().clone(), lcr.detach().clone()]
    torch.cuda.synchronize()
    return torch.stack(losses), opt._flat["g"].clone()


def test_deterministic_steps_64px_batch3(monkeypatch):
    """two training steps with the contrastive loss at 64 x 64, batch 3 (partly filled blocks of 4 x 4 and 8 x 8 images), twice from the same
    seeds in the deterministic mode: the same losses and the same flat gradient, bit for bit, and no library convolution in the step -
    every Winograd layer of the three passes ran, the 4 x 4 ones on the any-size entries (the model's 256 -> 512 down-sampling runs its
    own kernels at this batch too, tests/test_gpu_downsample_batch_pad.py)."""
    from test_gpu_deterministic import deterministic
    with deterministic():
        with _no_library(monkeypatch) as launches:
            l0, g0 = _steps_64px(2, 3)
        l1, g1 = _steps_64px(2, 3)
    # a step: 12 Winograd layers forward for the reference pair and for the restored images, 12 backward-data products
    assert len(launches) == 2 * 36 and {(h, w) for _, h, w in launches} == {(64, 64), (32, 32), (16, 16), (8, 8), (4, 4)}, launches
    assert sum("_any" in name and (h, w) == (4, 4) for name, h, w in launches) == 2 * 3, launches
    assert not any("_any" in name for name, h, w in launches if (h, w) != (4, 4)), launches        # the other maps: the launches of before
    assert torch.isfinite(l0).all() and torch.isfinite(g0).all() and float(l0[1]) > 0
    assert torch.equal(l0, l1), (l0 - l1).abs().max().item()
    assert torch.equal(g0, g1), (g0 - g1).abs().max().item()


def test_my_train_64px_default_loss_weights_command_line():
    """the reference's command line at 64-pixel patches with the contrastive loss on (the default --w_loss_vgg7): no layer of the step
    goes to the library"""
    cmd = [sys.executable, os.path.join(PKG, "My_train.py"), "--train_ps", "64", "--embed_dim", "32", "--batch_size", "4",
           "--synthetic", "8", "--nepoch", "1"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240, env=dict(os.environ, DEHAZE_ALLOW_RANDOM_VGG="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "not tiled by the HIP kernels" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-2000:]
    losses = [float(x) for x in re.findall(r"loss:([0-9.eE+-]+|nan|inf)", r.stdout)]
    assert losses and all(math.isfinite(x) for x in losses), r.stdout[-2000:]
