"""-m gpu: the Winograd F(2x2,3x3) MFMA convolution (dhz_winograd_conv3x3) vs torch conv2d: forward (+bias, +ReLU)
and the backward-data pass (rotated/transposed filters + ReLU mask)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _blocked(x):
    from dehaze_hip import _lib
    B, C, H, W = x.shape
    out = torch.empty(B, C // 8, H, W, 8, device=x.device)
    _lib.call("dhz_layout_blocked8", x.contiguous().data_ptr(), out.data_ptr(), B, C, H * W, 1, None, 0, torch.cuda.current_stream().cuda_stream)
    return out


def _plain(xb, C):
    from dehaze_hip import _lib
    B, CG, H, W, _ = xb.shape
    out = torch.empty(B, C, H, W, device=xb.device)
    _lib.call("dhz_layout_blocked8", xb.data_ptr(), out.data_ptr(), B, C, H * W, 0, None, 0, torch.cuda.current_stream().cuda_stream)
    return out


# H = 8: the conv5_1 geometry - four 8 x 8 images share one 16 x 16 block of the kernel (B = 8: whole blocks; 5 and 3: a ragged
# last block, odd block counts; 1: a single image)
@pytest.mark.parametrize("B,C,K,H", [(2, 64, 64, 32), (1, 64, 128, 16), (2, 128, 128, 16), (1, 256, 512, 16), (3, 8, 32, 48),
                                     (8, 64, 64, 8), (5, 32, 64, 8), (3, 128, 32, 8), (1, 32, 32, 8)])
def test_winograd_forward_and_dgrad(B, C, K, H):
    winograd_case(B, C, K, H, H)


# H != W (the header's contract is H % 16 == 0 and W % 16 == 0): the block walk bx_n = W / 16, by_n = H / 16 and the row pitch W of the
# planes, with C != K
@pytest.mark.parametrize("H,W", [(16, 32), (32, 16)])
def test_winograd_forward_and_dgrad_nonsquare(H, W):
    winograd_case(2, 32, 64, H, W)


def close(what, got, want, atol, rtol):
    """torch.allclose with the worst error printed first"""
    print(f"{what}: worst error {(got - want).abs().max().item():.3e} (atol {atol:.0e}, rtol {rtol:.0e})")
    assert torch.allclose(got, want, atol=atol, rtol=rtol), (what, (got - want).abs().max())


def winograd_case(B, C, K, H, W):
    from dehaze_hip import _lib
    tag = f"winograd_conv3x3 B={B} C={C} K={K} {H}x{W}"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(C + K + H + 1000 * (W - H))
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)
    b = (0.1 * torch.randn(K, generator=g)).to(dev)
    up = torch.empty(16 * K * C, device=dev)
    _lib.call("dhz_winograd_prepack", w.data_ptr(), up.data_ptr(), K, C, 0, s)
    xb = _blocked(x)
    yb = torch.empty(B, K // 8, H, W, 8, device=dev)
    _lib.call("dhz_winograd_conv3x3", xb.data_ptr(), up.data_ptr(), b.data_ptr(), 1, None, None, yb.data_ptr(), B, H, W, C, K, s)
    y = _plain(yb, K)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).float()
    close(tag + " forward", y, ref, 2e-5, 1e-4)
    assert torch.equal(_plain(xb, C), x)
    # backward-data with the fused store: dx = (x > 0) ? conv_transpose(dy, w) + addend : 0  (x plays the saved post-ReLU
    # map below the layer, addend a tap gradient) == winograd with the transposed_rot filters
    dy = torch.randn(B, K, H, W, generator=g).to(dev)
    add = torch.randn(B, C, H, W, generator=g).to(dev)
    if C % 32 == 0:
        upt = torch.empty(16 * K * C, device=dev)
        _lib.call("dhz_winograd_prepack", w.data_ptr(), upt.data_ptr(), C, K, 1, s)      # Kout = C (of fwd), Cin = K
        dxb = torch.empty(B, C // 8, H, W, 8, device=dev)
        refdx = F.conv_transpose2d(dy.double(), w.double(), padding=1).float()
        dyb, addb = _blocked(dy), _blocked(add)
        _lib.call("dhz_winograd_conv3x3", dyb.data_ptr(), upt.data_ptr(), None, 0, xb.data_ptr(), addb.data_ptr(),
                  dxb.data_ptr(), B, H, W, K, C, s)
        want = (refdx + add) * (x > 0)
        close(tag + " backward-data, mask + addend", _plain(dxb, C), want, 5e-5, 1e-4)
        _lib.call("dhz_winograd_conv3x3", dyb.data_ptr(), upt.data_ptr(), None, 0, None, addb.data_ptr(),
                  dxb.data_ptr(), B, H, W, K, C, s)
        close(tag + " backward-data + addend", _plain(dxb, C), refdx + add, 5e-5, 1e-4)


@pytest.mark.parametrize("B,C,H", [(2, 64, 32), (1, 16, 8)])
def test_maxpool_blocked(B, C, H):
    from dehaze_hip import vgg as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H)
    a = torch.relu(torch.randn(B, C, H, H, generator=g)).to(dev).requires_grad_()     # post-ReLU map: many exact-zero windows
    yb = V.pool_fwd(_blocked(a.detach()))
    ref = F.max_pool2d(a, 2, 2)
    assert torch.equal(_plain(yb, C), ref.detach())
    gy = torch.randn(B, C, H // 2, H // 2, generator=g).to(dev)
    ref.backward(gy)
    gx = _plain(V.pool_bwd_relu(_blocked(gy), _blocked(a.detach())), C)
    assert torch.equal(gx, a.grad * (a.detach() > 0))


# F(4x4,3x3) (csrc/winograd43_conv.hip, round 5): the layers of the VGG19 stack it takes (maps of 32 x 32 and more; 64 .. 256 input
# channels), a 16 x 16 map, a ragged block count - at the SAME tolerances as the F(2x2,3x3) kernel above
@pytest.mark.parametrize("B,C,K,H", [(2, 64, 64, 32), (1, 64, 128, 64), (2, 128, 128, 32), (1, 128, 256, 32), (1, 256, 256, 32),
                                     (1, 256, 512, 16), (3, 64, 32, 16), (1, 16, 32, 48), (5, 32, 64, 16),
                                     (2, 512, 512, 16), (1, 384, 64, 16)])      # > 256 input channels: two accumulation chains (two launches)
def test_winograd43_forward_and_dgrad(B, C, K, H):
    winograd43_case(B, C, K, H, H)


@pytest.mark.parametrize("H,W", [(16, 32), (32, 16)])
def test_winograd43_forward_and_dgrad_nonsquare(H, W):
    winograd43_case(2, 32, 64, H, W)


def winograd43_case(B, C, K, H, W):
    from dehaze_hip import _lib
    tag = f"winograd43_conv3x3 B={B} C={C} K={K} {H}x{W}"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(C + K + H + 1000 * (W - H))
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)
    b = (0.1 * torch.randn(K, generator=g)).to(dev)
    up = torch.empty(36 * K * C, device=dev)
    _lib.call("dhz_winograd43_prepack", w.data_ptr(), up.data_ptr(), K, C, 0, s)
    xb = _blocked(x)
    yb = torch.empty(B, K // 8, H, W, 8, device=dev)
    _lib.call("dhz_winograd43_conv3x3", xb.data_ptr(), up.data_ptr(), b.data_ptr(), 1, None, None, yb.data_ptr(), B, H, W, C, K, s)
    y = _plain(yb, K)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).float()
    close(tag + " forward", y, ref, 2e-5, 1e-4)
    # without bias / ReLU
    _lib.call("dhz_winograd43_conv3x3", xb.data_ptr(), up.data_ptr(), None, 0, None, None, yb.data_ptr(), B, H, W, C, K, s)
    ref0 = F.conv2d(x.double(), w.double(), padding=1).float()
    close(tag + " forward, no bias / ReLU", _plain(yb, K), ref0, 2e-5, 1e-4)
    if C % 32 == 0:
        dy = torch.randn(B, K, H, W, generator=g).to(dev)
        add = torch.randn(B, C, H, W, generator=g).to(dev)
        upt = torch.empty(36 * K * C, device=dev)
        _lib.call("dhz_winograd43_prepack", w.data_ptr(), upt.data_ptr(), C, K, 1, s)      # Kout = C (of fwd), Cin = K
        dxb = torch.empty(B, C // 8, H, W, 8, device=dev)
        refdx = F.conv_transpose2d(dy.double(), w.double(), padding=1).float()
        dyb, addb = _blocked(dy), _blocked(add)
        _lib.call("dhz_winograd43_conv3x3", dyb.data_ptr(), upt.data_ptr(), None, 0, xb.data_ptr(), addb.data_ptr(),
                  dxb.data_ptr(), B, H, W, K, C, s)
        want = (refdx + add) * (x > 0)
        close(tag + " backward-data, mask + addend", _plain(dxb, C), want, 5e-5, 1e-4)
        _lib.call("dhz_winograd43_conv3x3", dyb.data_ptr(), upt.data_ptr(), None, 0, None, addb.data_ptr(),
                  dxb.data_ptr(), B, H, W, K, C, s)
        close(tag + " backward-data + addend", _plain(dxb, C), refdx + add, 5e-5, 1e-4)
    # convolution + bias + ReLU + 2 x 2 max pooling in one launch (the un-pooled map is never written; C > 256: chains through the scratch map)
    yp = torch.empty(B, K // 8, H // 2, W // 2, 8, device=dev)
    scratch = torch.empty(B, K // 8, H, W, 8, device=dev) if C > 256 else None
    _lib.call("dhz_winograd43_conv3x3_pool", xb.data_ptr(), up.data_ptr(), b.data_ptr(), yp.data_ptr(),
              scratch.data_ptr() if scratch is not None else None, B, H, W, C, K, s)
    close(tag + " forward + pooling", _plain(yp, K), F.max_pool2d(ref, 2, 2), 2e-5, 1e-4)
    lib = _lib.load()
    assert lib.dhz_winograd43_conv3x3(xb.data_ptr(), up.data_ptr(), None, 0, None, None, yb.data_ptr(), B, 8, 8, C, K, s) == -22
    if C > 256:
        assert lib.dhz_winograd43_conv3x3_pool(xb.data_ptr(), up.data_ptr(), b.data_ptr(), yp.data_ptr(), None, B, H, W, C, K, s) == -22


@pytest.mark.parametrize("ablation", [False, True])
def test_contrast_loss_engine_vs_oracle(ablation):
    """ContrastLoss on the Winograd feature engine (128x128 patches) vs the CPU oracle in float64: value, the two L1
    sums, and the gradient w.r.t. the restored image; and Vgg19.forward's NCHW features vs the oracle's."""
    import warnings
    import My_CR
    from oracle import uformer_oracle as O
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cl = My_CR.ContrastLoss(ablation=ablation).to(dev)
    g = torch.Generator().manual_seed(77)
    a, p, n = (torch.rand(2, 3, 128, 128, generator=g) for _ in range(3))
    W = O.seeded_vgg_weights(dtype=torch.float64)
    a64 = a.double().requires_grad_()
    loss_o, ap_o, an_o = O.contrast_loss(a64, p.double(), n.double(), W, ablation=ablation)
    loss_o.backward()

    ad = a.to(dev).requires_grad_()
    assert cl.vgg.engine_for(ad) is not None
    loss, ap, an = cl(ad, p.to(dev), n.to(dev))
    loss.backward()
    assert abs(loss.item() - loss_o.item()) < 2e-4 * abs(loss_o.item()), (loss.item(), loss_o.item())
    assert abs(float(ap) - float(ap_o)) < 2e-4 * float(ap_o)
    if not ablation:
        assert abs(float(an) - float(an_o)) < 2e-4 * float(an_o)
    # d|fa - fp| = sign(fa - fp): an fp32-vs-fp64 rounding difference flips a few signs / ReLU masks among the ~10^6
    # feature elements, so the max error is loose (the smooth-loss test below pins the backward chain tightly)
    ref = a64.grad.float()
    err = (ad.grad.cpu() - ref).abs()
    assert err.max().item() < 3e-2 * ref.abs().max().item(), (err.max().item(), ref.abs().max().item())
    # (mean: 4.4e-3 measured - every layer incl. conv5_1 now has the F(2x2,3x3) rounding error, 4.4e-7 absolute on O(1) features)
    assert err.mean().item() < 8e-3 * ref.abs().mean().item(), (err.mean().item(), ref.abs().mean().item())

    feats = cl.vgg(a.to(dev))
    feats_o = O.vgg19_features(a.double(), W)
    for f, fo in zip(feats, feats_o):
        assert f.shape == fo.shape
        assert (f.cpu() - fo.float()).abs().max().item() < 2e-3 * fo.abs().max().item()


def test_vgg_engine_backward_smooth_loss():
    """The engine's hand-sequenced backward (Winograd backward-data + ReLU masks + pool scatter + library ends) against
    float64 autograd of the oracle on a smooth functional: sum_i <R_i, tap_i(a)>."""
    import warnings
    import My_CR
    from dehaze_hip import vgg as V
    from oracle import uformer_oracle as O
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = My_CR.Vgg19().to(dev)
    g = torch.Generator().manual_seed(5)
    a = torch.rand(1, 3, 128, 128, generator=g)
    W = O.seeded_vgg_weights(dtype=torch.float64)
    a64 = a.double().requires_grad_()
    feats_o = O.vgg19_features(a64, W)
    R = [torch.randn(f.shape, generator=g) for f in feats_o]
    sum((f * r.double()).sum() for f, r in zip(feats_o, R)).backward()

    ad = a.to(dev).requires_grad_()
    feats = net(ad)                                   # engine taps -> NCHW through the differentiable layout op
    assert net.engine_for(ad) is not None
    sum((f * r.to(dev)).sum() for f, r in zip(feats, R)).backward()
    ref = a64.grad.float()
    err = (ad.grad.cpu() - ref).abs().max().item()
    assert err < 2e-4 * ref.abs().max().item(), (err, ref.abs().max().item())


def test_vgg_engine_library_tail_for_untiled_maps():
    """384 x 384 patches: conv5_1 sees 24 x 24 maps, which the Winograd kernel does not tile (neither multiples of 16 nor 8 x 8) -
    that one layer runs on the library inside the engine.  Features and the input gradient of a smooth functional against the
    same module evaluated by the library in float64.  (A single ReLU mask that flips between two roundings moves the max error
    of the gradient to ~3 % of its max - measured for the fp32 library path itself - so the tight criterion is the mean.)"""
    import warnings
    import My_CR
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = My_CR.Vgg19().to(dev)
    g = torch.Generator().manual_seed(9)
    a = torch.rand(1, 3, 384, 384, generator=g).to(dev)
    ae = a.clone().requires_grad_()
    assert net.engine_for(ae) is not None
    fe = net(ae)
    R = [torch.randn(f.shape, generator=g).to(dev) for f in fe]
    sum((f * r).sum() for f, r in zip(fe, R)).backward()
    net.double()                                              # float64: the engine does not apply, library convolutions
    try:
        a64 = a.double().requires_grad_()
        assert net.engine_for(a64) is None
        f64 = net(a64)
        sum((f * r.double()).sum() for f, r in zip(f64, R)).backward()
    finally:
        net.float()
    for x, y in zip(fe, f64):
        assert x.shape == y.shape and (x.double() - y).abs().max().item() < 1e-4 * y.abs().max().item()
    err = (ae.grad.double() - a64.grad).abs()
    assert err.mean().item() < 1e-3 * a64.grad.abs().mean().item(), (err.mean().item(), a64.grad.abs().mean().item())
    assert err.max().item() < 5e-2 * a64.grad.abs().max().item(), (err.max().item(), a64.grad.abs().max().item())


@pytest.mark.parametrize("B,C,H,W", [(2, 16, 8, 8), (1, 8, 7, 7), (3, 64, 12, 20)])
def test_layout_conversion_with_bias_relu(B, C, H, W):
    """NCHW <-> NCHW8c (vector kernel for H*W % 4 == 0, scalar otherwise), with the optional bias + ReLU on the way in."""
    from dehaze_hip import vgg as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    xb = V.to_blocked(x)
    assert torch.equal(xb, x.view(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2))
    assert torch.equal(V.to_plain(xb), x)
    yb = V.to_blocked(x, b, relu=True)
    assert torch.equal(V.to_plain(yb), torch.relu(x + b.view(1, C, 1, 1)))


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 13, 21)])
def test_first_vgg_layer_kernel(B, H, W):
    """Conv2d(3 -> 64, 3x3) + bias + ReLU from NCHW straight into the blocked layout (ragged tiles included) vs conv2d."""
    from dehaze_hip import _lib, vgg as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H)
    x = torch.rand(B, 3, H, W, generator=g).to(dev)
    w = (torch.randn(64, 3, 3, 3, generator=g) * 0.3).to(dev)
    b = torch.randn(64, generator=g).to(dev)
    yb = torch.empty(B, 8, H, W, 8, device=dev)
    _lib.call("dhz_conv3x3_in3_blocked", x.data_ptr(), w.data_ptr(), b.data_ptr(), yb.data_ptr(), B, H, W, 64, 1,
              torch.cuda.current_stream().cuda_stream)
    ref = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1)).float()
    assert torch.allclose(V.to_plain(yb), ref, atol=2e-5, rtol=1e-4), (V.to_plain(yb) - ref).abs().max()


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 13, 21), (5, 128, 128)])
def test_first_vgg_layer_backward_data_from_blocked_gradient(B, H, W):
    """dhz_thin_conv3x3_dgrad_blocked (first VGG layer's backward-data, 64 -> 3, straight from the channel-blocked gradient;
    matrix-pipe kernel with persistent workgroups - the last shape has more tiles than workgroups) vs conv_transpose2d."""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H + B)
    G = torch.randn(B, 64, H, W, generator=g).to(dev)
    w = (torch.randn(64, 3, 3, 3, generator=g) * 0.3).to(dev)
    gb = _blocked(G)
    dx = torch.empty(B, 3, H, W, device=dev)
    _lib.call("dhz_thin_conv3x3_dgrad_blocked", gb.data_ptr(), w.data_ptr(), dx.data_ptr(), B, H, W, 64,
              torch.cuda.current_stream().cuda_stream)
    ref = F.conv_transpose2d(G.double(), w.double(), padding=1).float()
    assert torch.allclose(dx, ref, atol=1e-4, rtol=1e-4), (dx - ref).abs().max()


def test_vgg_engine_f43_dispatch_at_step_size():
    """The F(4x4,3x3) form inside the feature engine at the training step's sizes (32 restored images with gradient, 64 reference images
    without): it is taken exactly where dehaze_hip.vgg.use_f43 says - in the differentiated forward pass only under vgg.F43_DIFF, on the
    no-gradient pass and the backward-data products when the grid fills the CUs in whole rounds - and the contrastive loss, its two
    distances and d(loss)/d(restored) agree with the all-F(2x2) engine (DHZ_WINO_F43=0) to rounding."""
    import warnings
    import My_CR
    from dehaze_hip import _lib, vgg as V
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cl = My_CR.ContrastLoss().to(dev)
    g = torch.Generator().manual_seed(3)
    a0, p, n = (torch.rand(32, 3, 128, 128, generator=g).to(dev) for _ in range(3))
    calls, pooled = [], []
    real = _lib.call

    def spy(name, *args):
        if name in ("dhz_winograd43_conv3x3", "dhz_winograd_conv3x3"):
            calls.append((name, args[7], args[8], args[10], args[11], args[3] == 0))   # B, H, C, K, backward-data product? (no ReLU)
        if name == "dhz_winograd43_conv3x3_pool":                                      # convolution + ReLU + pooling in one launch
            calls.append(("dhz_winograd43_conv3x3", args[5], args[6], args[8], args[9], False))
            pooled.append((args[5], args[6]))
        return real(name, *args)

    res = {}
    old = V.F43_ON
    try:
        for on in (False, True):
            V.F43_ON = on
            calls.clear()
            pooled.clear()
            _lib.call = V._lib.call = spy
            a = a0.clone().requires_grad_()
            loss, ap, an = cl(a, p, n)
            loss.backward()
            _lib.call = V._lib.call = real
            res[on] = (loss.item(), float(ap), float(an), a.grad.clone(), list(calls))
    finally:
        V.F43_ON = old
        _lib.call = V._lib.call = real
    off, on = res[False], res[True]
    assert not any(c[0] == "dhz_winograd43_conv3x3" for c in off[4])
    f43 = [c for c in on[4] if c[0] == "dhz_winograd43_conv3x3"]
    assert len(f43) >= 15, len(f43)
    if V.F43_DIFF:     # round 6 (profiles/r06_wino_f43_diff.txt): the differentiated forward of the 32 restored images too, on whole-round grids
        assert any(c[1] == 32 and not c[5] for c in f43)
    else:
        assert not any(c[1] == 32 and not c[5] for c in f43)               # never the forward pass of the 32 differentiated images
    assert any(c[1] == 64 and c[2] == 16 for c in f43)                     # 64 reference images on the 16 x 16 maps: 256 workgroups
    assert not any(c[1] == 32 and c[2] == 16 for c in f43)                 # 32 images there: half a round - stays on F(2x2)
    assert sorted(pooled) == [(64, 16), (64, 32), (64, 64), (64, 128)]     # the four pooled layers of the no-gradient pass: pooling in the launch
    assert abs(on[0] - off[0]) < 2e-5 * abs(off[0]) and abs(on[1] - off[1]) < 2e-5 * off[1] and abs(on[2] - off[2]) < 2e-5 * off[2]
    d = (on[3] - off[3]).abs()
    # (DHZ_WINO_F43_DIFF=0: same ReLU masks in both runs, the differentiated forward pass is F(2x2) either way; sign(fa - fp) may flip where
    # the reference features moved by their ~1e-6 rounding difference.  Default: the masks come from the F(4x4) forward - the same bound holds)
    assert d.mean().item() < 2e-3 * off[3].abs().mean().item(), (d.mean().item(), off[3].abs().mean().item())


def test_vgg_engine_pooling_in_the_convolution_store_is_bit_identical():
    """The no-gradient pass with the 2 x 2 max pooling inside the F(4x4) launch (dhz_winograd43_conv3x3_pool) against the same pass with
    the pooling as its own launch: the five tap features are bit-identical (the maximum of the same four values)."""
    import warnings
    import My_CR
    from dehaze_hip import vgg as V
    dev = torch.device("cuda:0")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cl = My_CR.ContrastLoss().to(dev)
    x = torch.rand(64, 3, 128, 128, generator=torch.Generator().manual_seed(11)).to(dev)
    eng = cl.vgg.engine_for(x)
    assert eng is not None
    old = V.POOL_FUSED
    try:
        with torch.no_grad():
            V.POOL_FUSED = True
            a = [t.clone() for t in eng.forward_taps(x)]
            V.POOL_FUSED = False
            b = eng.forward_taps(x)
    finally:
        V.POOL_FUSED = old
    assert len(a) == len(b) == 5
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("with_n", [True, False])
def test_l1_pair_fp32(with_n):
    """dhz_l1_pair_fwd / _bwd on fp32 maps: the twin of test_l1_pair_bf16 (tests/test_gpu_vgg_bf16.py) - same count, planted exact ties
    (sign 0), with and without the negative.  The sums against float64 at that test's 1e-5 relative bound.  The backward against
    g0 / cnt * sign(a - p) + g1 / cnt * sign(a - n) formed in fp32: the kernel multiplies g by a host-computed 1.0f / cnt instead of
    dividing (csrc/elementwise.hip, l1_pair_bwd_kernel: cp = g[0] * inv_n), one more rounding than the quotient, so the comparison is
    allclose at rtol 1e-6 with no absolute term - not torch.equal.  The signs themselves are exact: where a == p the term is 0."""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    cnt = 8 * 12345
    a, p, n = ((torch.randn(cnt, generator=g) * 2).to(dev) for _ in range(3))
    p[:100] = a[:100]                                   # exact zeros of the difference: sign 0
    n[50:150] = a[50:150]                               # ... of either difference, and of both at once (50..99)
    sums = torch.zeros(2, device=dev)
    _lib.call("dhz_l1_pair_fwd", a.data_ptr(), p.data_ptr(), n.data_ptr() if with_n else None, sums.data_ptr(), cnt, s)
    rp = (a.double() - p.double()).abs().sum().item()
    rn = (a.double() - n.double()).abs().sum().item()
    print(f"l1_pair fp32 with_n={with_n}: relative error of the sums {abs(sums[0].item() - rp) / rp:.3e}"
          + (f", {abs(sums[1].item() - rn) / rn:.3e}" if with_n else ""))
    assert abs(sums[0].item() - rp) < 1e-5 * rp
    assert abs(sums[1].item() - rn) < 1e-5 * rn if with_n else sums[1].item() == 0.0
    gsc = torch.tensor([0.7, -1.3], device=dev)
    da = torch.full((cnt + 64,), float("nan"), device=dev)
    _lib.call("dhz_l1_pair_bwd", a.data_ptr(), p.data_ptr(), n.data_ptr() if with_n else None, gsc.data_ptr(), da.data_ptr(), cnt, s)
    assert torch.isnan(da[cnt:]).all() and not torch.isnan(da[:cnt]).any()
    da = da[:cnt].cpu()
    ac, pc, nc, gc = a.cpu(), p.cpu(), n.cpu(), gsc.cpu()
    ref = gc[0] / cnt * torch.sign(ac - pc)
    if with_n:
        ref = ref + gc[1] / cnt * torch.sign(ac - nc)
    print(f"l1_pair fp32 with_n={with_n}: worst relative error of da {((da - ref).abs() / ref.abs().clamp_min(1e-30)).max().item():.3e}")
    assert torch.allclose(da, ref, rtol=1e-6, atol=0.0)
    assert (da[50:100] == 0).all() if with_n else (da[:100] == 0).all()
