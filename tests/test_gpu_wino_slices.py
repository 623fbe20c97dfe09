"""-m gpu: channel slices of the Winograd convolutions (dhz_winograd_conv3x3_slices, dhz_winograd43_conv3x3_slices) - S copies of the plain
grid, each over 1 / S of the input-channel groups, raw sums into a workspace, one epilogue kernel - against float64 conv2d /
conv_transpose2d at the tolerances of tests/test_gpu_winograd.py (forward 2e-5 / 1e-4, backward-data 5e-5 / 1e-4).  The workspace and the
output are filled with NaN before every call: every element the epilogue reads must have been written by a slice.

B, C, K name the kernel's arguments: C input channels, K output channels.  The backward-data modes run the kernel with the
transposed_rot filters of a weight [C, K, 3, 3], i.e. conv_transpose2d of the C-channel input - the same C and K as the forward modes."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FWD_TOL = (2e-5, 1e-4)
BWD_TOL = (5e-5, 1e-4)
MODES = ("bias_relu", "plain", "mask_addend", "addend")
EINVAL = -22


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


def close(what, got, want, tol):
    print(f"{what}: worst error {(got - want).abs().max().item():.3e} (atol {tol[0]:.0e}, rtol {tol[1]:.0e})")
    assert torch.allclose(got, want, atol=tol[0], rtol=tol[1]), (what, (got - want).abs().max())


@functools.lru_cache(maxsize=None)
def _case(f43, B, C, K, H, W):
    """inputs, packed filters and the float64 references of one shape, computed once and shared by every slice count (never modified)"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7 * C + K + H + 1000 * W + B)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(K, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)       # forward: [K out][C in]
    wt = (torch.randn(C, K, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)      # backward-data of a K -> C layer: contraction over C
    b = (0.1 * torch.randn(K, generator=g)).to(dev)
    act = torch.relu(torch.randn(B, K, H, W, generator=g)).to(dev)                    # saved post-ReLU map at the output positions
    add = torch.randn(B, K, H, W, generator=g).to(dev)
    n, pre = (36, "dhz_winograd43_prepack") if f43 else (16, "dhz_winograd_prepack")
    up, upt = torch.empty(n * K * C, device=dev), torch.empty(n * K * C, device=dev)
    _lib.call(pre, w.data_ptr(), up.data_ptr(), K, C, 0, s)
    _lib.call(pre, wt.data_ptr(), upt.data_ptr(), K, C, 1, s)
    conv = F.conv2d(x.double(), w.double(), padding=1)
    convt = F.conv_transpose2d(x.double(), wt.double(), padding=1)
    ref = {"bias_relu": F.relu(conv + b.double().view(1, K, 1, 1)).float(), "plain": conv.float(),
           "mask_addend": ((convt + add.double()) * (act > 0)).float(), "addend": (convt + add.double()).float()}
    return dict(xb=_blocked(x), up=up, upt=upt, b=b, actb=_blocked(act), addb=_blocked(add), ref=ref)


def _args(c, mode):
    """(filters, bias, relu, mask, addend) of a mode"""
    if mode == "bias_relu":
        return c["up"], c["b"].data_ptr(), 1, None, None
    if mode == "plain":
        return c["up"], None, 0, None, None
    if mode == "mask_addend":
        return c["upt"], None, 0, c["actb"].data_ptr(), c["addb"].data_ptr()
    return c["upt"], None, 0, None, c["addb"].data_ptr()


def _run_sliced(entry, c, mode, S, B, C, K, H, W):
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    up, bias, relu, mask, addend = _args(c, mode)
    yb = torch.full((B, K // 8, H, W, 8), float("nan"), device=dev)
    ws = torch.full((S, B, K // 8, H, W, 8), float("nan"), device=dev)
    _lib.call(entry, c["xb"].data_ptr(), up.data_ptr(), bias, relu, mask, addend, yb.data_ptr(), ws.data_ptr(), S, B, H, W, C, K,
              torch.cuda.current_stream().cuda_stream)
    return yb


def _run_plain(entry, c, mode, B, C, K, H, W):
    from dehaze_hip import _lib
    up, bias, relu, mask, addend = _args(c, mode)
    yb = torch.full((B, K // 8, H, W, 8), float("nan"), device=torch.device("cuda:0"))
    _lib.call(entry, c["xb"].data_ptr(), up.data_ptr(), bias, relu, mask, addend, yb.data_ptr(), B, H, W, C, K,
              torch.cuda.current_stream().cuda_stream)
    return yb


# F(2x2).  8 x 8 maps (four images per 16 x 16 block): B = 5 - a ragged last block and an odd block count (the second half of the last
# workgroup stores nothing) - with S = 8 leaving ONE channel group per slice, and a single image.  16-pixel maps: three blocks (odd count),
# S = 3, and S = 4 on six groups, which gives the uneven ranges 1, 2, 1, 2 (floor(s 6 / 4) = 0, 1, 3, 4, 6); a 16 x 32 map.
F22_CASES = [(5, 64, 32, 8, 8, 1), (5, 64, 32, 8, 8, 2), (5, 64, 32, 8, 8, 4), (5, 64, 32, 8, 8, 8), (1, 32, 64, 8, 8, 4),
             (3, 48, 64, 16, 16, 3), (3, 48, 64, 16, 16, 4), (2, 32, 64, 16, 32, 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W,S", F22_CASES)
def test_winograd_slices_vs_float64(B, C, K, H, W, S, mode):
    c = _case(False, B, C, K, H, W)
    yb = _run_sliced("dhz_winograd_conv3x3_slices", c, mode, S, B, C, K, H, W)
    close(f"winograd_conv3x3_slices S={S} B={B} C={C} K={K} {H}x{W} {mode}", _plain(yb, K), c["ref"][mode],
          FWD_TOL if mode in ("bias_relu", "plain") else BWD_TOL)
    # the same call again: the same bits (no atomics, a fixed order of the parts)
    assert torch.equal(_run_sliced("dhz_winograd_conv3x3_slices", c, mode, S, B, C, K, H, W), yb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W", [(5, 64, 32, 8, 8), (3, 48, 64, 16, 16)])
def test_winograd_slices_one_slice_is_the_plain_launch(B, C, K, H, W, mode):
    from dehaze_hip import _lib
    c = _case(False, B, C, K, H, W)
    want = _run_plain("dhz_winograd_conv3x3", c, mode, B, C, K, H, W)
    assert torch.equal(_run_sliced("dhz_winograd_conv3x3_slices", c, mode, 1, B, C, K, H, W), want)
    # one slice takes no workspace
    up, bias, relu, mask, addend = _args(c, mode)
    yb = torch.full_like(want, float("nan"))
    _lib.call("dhz_winograd_conv3x3_slices", c["xb"].data_ptr(), up.data_ptr(), bias, relu, mask, addend, yb.data_ptr(), None, 1, B, H, W, C,
              K, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(yb, want)


def test_winograd_slices_refusals():
    from dehaze_hip import _lib
    lib = _lib.load()
    B, C, K, H, W = 1, 32, 64, 8, 8
    c = _case(False, B, C, K, H, W)
    s = torch.cuda.current_stream().cuda_stream
    yb = torch.zeros(B, K // 8, H, W, 8, device=torch.device("cuda:0"))
    ws = torch.zeros(8, B, K // 8, H, W, 8, device=torch.device("cuda:0"))
    x, up = c["xb"].data_ptr(), c["up"].data_ptr()
    assert lib.dhz_winograd_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), ws.data_ptr(), C // 8 + 1, B, H, W, C, K, s) == EINVAL
    assert lib.dhz_winograd_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), None, 2, B, H, W, C, K, s) == EINVAL
    assert lib.dhz_winograd_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), ws.data_ptr(), 0, B, H, W, C, K, s) == EINVAL
    assert lib.dhz_winograd_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), ws.data_ptr(), C // 8, B, H, W, C, K, s) == 0
    torch.cuda.synchronize()
    assert not yb.isnan().any()


# F(4x4): parallel accumulation-chain links.  512 channels in two slices are the two links of the chained launch, added in the chain's order:
# the same bits.  Three blocks = one ragged workgroup per (slice, output-channel block); 32 x 16: a non-square map, four slices of 64 channels.
F43_CASES = [(2, 512, 32, 16, 16, 2), (3, 64, 64, 16, 16, 2), (3, 64, 64, 16, 16, 4), (1, 256, 32, 32, 16, 4)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,C,K,H,W,S", F43_CASES)
def test_winograd43_slices_vs_float64(B, C, K, H, W, S, mode):
    c = _case(True, B, C, K, H, W)
    yb = _run_sliced("dhz_winograd43_conv3x3_slices", c, mode, S, B, C, K, H, W)
    close(f"winograd43_conv3x3_slices S={S} B={B} C={C} K={K} {H}x{W} {mode}", _plain(yb, K), c["ref"][mode],
          FWD_TOL if mode in ("bias_relu", "plain") else BWD_TOL)
    assert torch.equal(_run_sliced("dhz_winograd43_conv3x3_slices", c, mode, S, B, C, K, H, W), yb)
    if C == 512 and S == 2:
        assert torch.equal(yb, _run_plain("dhz_winograd43_conv3x3", c, mode, B, C, K, H, W))


def test_winograd43_slices_refusals():
    from dehaze_hip import _lib
    lib = _lib.load()
    B, C, K, H, W = 3, 64, 64, 16, 16
    c = _case(True, B, C, K, H, W)
    s = torch.cuda.current_stream().cuda_stream
    yb = torch.zeros(B, K // 8, H, W, 8, device=torch.device("cuda:0"))
    ws = torch.zeros(4, B, K // 8, H, W, 8, device=torch.device("cuda:0"))
    x, up = c["xb"].data_ptr(), c["up"].data_ptr()
    assert lib.dhz_winograd43_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), None, 2, B, H, W, C, K, s) == EINVAL
    assert lib.dhz_winograd43_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), ws.data_ptr(), 1, B, H, W, C, K, s) == EINVAL
    assert lib.dhz_winograd43_conv3x3_slices(x, up, None, 0, None, None, yb.data_ptr(), ws.data_ptr(), 3, B, H, W, C, K, s) == EINVAL   # 8 groups % 3


def _map_side(i, patch=128):
    """side of the map conv i of the VGG19 stack works on"""
    from dehaze_hip import vgg as V
    return patch >> sum(1 for p in V.POOL_AFTER if p < i)


def _expected_launches(V, cus):
    """(entry, slices, B, H, C, K) of every sliced launch of one loss forward + backward at the step's sizes, from the rules alone"""
    want = []

    def one(B, H, C, K, allow43):
        if allow43 and V.use_f43(B, H, H, C, K):
            return
        s43 = V.f43_slices_rule(B, H, H, C, K, cus) if (allow43 and V.F43_ON) else 0
        if s43:
            want.append(("dhz_winograd43_conv3x3_slices", s43, B, H, C, K))
            return
        s22 = V.wino_slices_rule(B, H, H, C, K, cus)
        if s22 > 1:
            want.append(("dhz_winograd_conv3x3_slices", s22, B, H, C, K))

    for i in range(1, 13):
        C, K = V.CONVS[i]
        H = _map_side(i)
        one(32, H, C, K, V.F43_DIFF)       # differentiated forward of the 32 restored images
        one(64, H, C, K, True)             # no-gradient pass of the 64 reference images
        one(32, H, K, C, True)             # backward-data product
    return sorted(want)


def test_vgg_engine_slice_dispatch_at_step_size():
    """The sliced entries inside the feature engine at the training step's sizes (32 restored images with gradient, 64 reference images
    without): with the switch on they are called for exactly the launches the two rules name at this device's CU count, with
    dehaze_hip.vgg.SLICES_ON off (DHZ_WINO_SLICES=0) never; the contrastive loss, its two distances and d(loss)/d(restored) of the two settings
    agree within the bounds of test_vgg_engine_f43_dispatch_at_step_size (2e-5 relative, 2e-3 of the mean)."""
    import warnings
    import My_CR
    from dehaze_hip import _lib, vgg as V
    dev = torch.device("cuda:0")
    lib = _lib.load()
    cus = lib.dhz_grid_cus() + lib.dhz_get_reserved_cus()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cl = My_CR.ContrastLoss().to(dev)
    g = torch.Generator().manual_seed(3)
    a0, p, n = (torch.rand(32, 3, 128, 128, generator=g).to(dev) for _ in range(3))
    calls = []
    real = _lib.call

    def spy(name, *args):
        if name in ("dhz_winograd43_conv3x3_slices", "dhz_winograd_conv3x3_slices"):
            calls.append((name, args[8], args[9], args[10], args[12], args[13]))       # slices, B, H, C, K
        return real(name, *args)

    res = {}
    old = V.SLICES_ON
    try:
        for on in (False, True):
            V.SLICES_ON = on
            calls.clear()
            _lib.call = V._lib.call = spy
            a = a0.clone().requires_grad_()
            loss, ap, an = cl(a, p, n)
            loss.backward()
            _lib.call = V._lib.call = real
            res[on] = (loss.item(), float(ap), float(an), a.grad.clone(), sorted(calls))
        V.SLICES_ON = True
        want = _expected_launches(V, cus)
    finally:
        V.SLICES_ON = old
        _lib.call = V._lib.call = real
    # the library's own query is the rule stated in dehaze_hip.vgg.wino_slices_rule, at this device's CU count
    for i in range(1, 13):
        (C, K), H = V.CONVS[i], _map_side(i)
        for B, c, k in ((32, C, K), (64, C, K), (32, K, C)):
            assert lib.dhz_winograd_slices(B, H, H, c, k) == V.wino_slices_rule(B, H, H, c, k, cus), (B, H, c, k)
    off, on = res[False], res[True]
    assert off[4] == []
    print("sliced launches:", on[4])
    assert on[4] == want, (on[4], want)
    if cus == 256:
        assert len(want) >= 4            # the step's under-filled launches exist on the full part
    print(f"loss {on[0]:.8f} / {off[0]:.8f}, ap {on[1]:.8f} / {off[1]:.8f}, an {on[2]:.8f} / {off[2]:.8f}")
    assert abs(on[0] - off[0]) < 2e-5 * abs(off[0]) and abs(on[1] - off[1]) < 2e-5 * off[1] and abs(on[2] - off[2]) < 2e-5 * off[2]
    d = (on[3] - off[3]).abs()
    print(f"d(loss)/d(restored): mean difference {d.mean().item():.3e}, mean magnitude {off[3].abs().mean().item():.3e}")
    assert d.mean().item() < 2e-3 * off[3].abs().mean().item(), (d.mean().item(), off[3].abs().mean().item())
