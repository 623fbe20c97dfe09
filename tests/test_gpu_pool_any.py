"""The 2 x 2 max pooling of the channel-blocked layout on maps of ANY size (dhz_maxpool2x2_blocked_fwd_any, dhz_maxpool2x2_blocked_bwd_any,
dhz_maxpool2x2_blocked_bwd_add_any: floor mode, the dropped odd row / column written by the backward) and the L1 mean on any element count
(dhz_l1_pair_fwd_any, dhz_l1_pair_bwd_any), through the raw C-ABI against float64.

Bounds are the existing ones: the pooling forward exact and the backward rtol 1e-6, atol 0 (tests/test_gpu_perloss.py::
test_pool_backward_with_tap_gradient_against_float64 - one addition of two fp32 values); the L1 sums 1e-5 relative and the L1 backward
rtol 1e-6, atol 0 (tests/test_gpu_winograd.py::test_l1_pair_fp32).  On even maps the `_any` poolings must give the bits of the even-only
entries, which are reached here through their wrappers vgg.pool_fwd / vgg.pool_bwd_relu / vgg.pool_bwd_relu_add."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                                                    # NaN floats behind every output that must stay NaN
POOL_SHAPES = [(1, 3, 3), (2, 5, 4), (2, 4, 7), (3, 13, 21), (16, 33, 31)]       # one window; odd H; odd W; both odd; several grid passes


def _lib():
    from dehaze_hip import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


def pool_case(N, H, W):
    """pre-activation [N][H][W][8] with a window that is all zero after the ReLU, gy, addend; float64 references by autograd of
    max_pool2d(relu(.), 2, 2) (floor mode), without and with the tap's own gradient"""
    gen = torch.Generator().manual_seed(1000 * N + 31 * H + W)
    pre = torch.randn(N, H, W, 8, generator=gen)
    pre[:, 0:2, 0:2] = -1.0                                               # a window that is zero after the ReLU
    if H % 2:
        pre[:, H - 1, 0] = -0.5                                           # a non-positive and a positive unit on the dropped row ...
        pre[:, H - 1, W - 1] = 0.75
    if W % 2:
        pre[:, 0, W - 1] = -0.5                                           # ... and column
        pre[:, 1, W - 1] = 0.75
    act = pre.clamp(min=0)
    gy = torch.randn(N, H // 2, W // 2, 8, generator=gen)
    add = torch.randn(N, H, W, 8, generator=gen)
    refs = []
    for with_add in (False, True):
        p64 = pre.double().permute(0, 3, 1, 2).requires_grad_()           # planes [N, 8, H, W]
        a64 = torch.relu(p64)
        pooled = torch.nn.functional.max_pool2d(a64, 2, 2)
        loss = (pooled * gy.double().permute(0, 3, 1, 2)).sum()
        if with_add:
            loss = loss + (a64 * add.double().permute(0, 3, 1, 2)).sum()
        loss.backward()
        refs.append(p64.grad.permute(0, 2, 3, 1).contiguous())
    return act, gy, add, pooled.detach().permute(0, 2, 3, 1).contiguous(), refs[0], refs[1]


def guarded(numel):
    return torch.full((numel + GUARD,), float("nan"), device="cuda")


def take(buf, shape):
    n = 1
    for d in shape:
        n *= d
    torch.cuda.synchronize()
    got, tail = buf[:n].cpu().view(shape), buf[n:].cpu()
    assert not torch.isnan(got).any(), "an element was not written"
    assert torch.isnan(tail).all(), "written past the end"
    return got


# ------------------------------------------------------------------------------------------------ 1. the poolings against float64
@pytest.mark.parametrize("N,H,W", POOL_SHAPES)
def test_pool_any_entries_against_float64(N, H, W):
    L = _lib()
    act, gy, add, pooled64, ref, ref_add = pool_case(N, H, W)
    Ho, Wo = H // 2, W // 2
    actd, gyd, addd = act.cuda(), gy.cuda(), add.cuda()                   # (referenced until the launches have run)

    yb = guarded(N * Ho * Wo * 8)
    L.call("dhz_maxpool2x2_blocked_fwd_any", actd.data_ptr(), yb.data_ptr(), N, H, W, _st())
    y = take(yb, (N, Ho, Wo, 8))
    assert torch.equal(y.double(), pooled64)                              # a maximum of fp32 values: exact

    gb = guarded(act.numel())
    L.call("dhz_maxpool2x2_blocked_bwd_any", gyd.data_ptr(), actd.data_ptr(), gb.data_ptr(), N, H, W, _st())
    got = take(gb, (N, H, W, 8))
    assert torch.allclose(got.double(), ref, rtol=1e-6, atol=0), (got.double() - ref).abs().max()
    assert (got[act <= 0] == 0).all()
    assert (got[:, 2 * Ho:] == 0).all() and (got[:, :, 2 * Wo:] == 0).all()          # the dropped row / column: exactly 0

    ga = guarded(act.numel())
    L.call("dhz_maxpool2x2_blocked_bwd_add_any", gyd.data_ptr(), actd.data_ptr(), addd.data_ptr(), ga.data_ptr(), N, H, W, _st())
    got = take(ga, (N, H, W, 8))
    assert torch.allclose(got.double(), ref_add, rtol=1e-6, atol=0), (got.double() - ref_add).abs().max()
    assert (got[act <= 0] == 0).all()
    masked = torch.where(act > 0, add, torch.zeros_like(add))                         # the dropped row / column: exactly the masked addend
    assert torch.equal(got[:, 2 * Ho:], masked[:, 2 * Ho:]) and torch.equal(got[:, :, 2 * Wo:], masked[:, :, 2 * Wo:])
    if H % 2:
        assert (got[:, H - 1, 0] == 0).all() and torch.equal(got[:, H - 1, W - 1], add[:, H - 1, W - 1])
    if W % 2:
        assert (got[:, 0, W - 1] == 0).all() and torch.equal(got[:, 1, W - 1], add[:, 1, W - 1])


def test_pool_any_entries_equal_the_even_entries_bit_for_bit():
    from dehaze_hip import vgg as V
    L = _lib()
    N, H, W = 3, 12, 20
    act, gy, add, _, _, _ = pool_case(N, H, W)
    actd, gyd, addd = act.cuda().view(N, 1, H, W, 8), gy.cuda().view(N, 1, H // 2, W // 2, 8), add.cuda().view(N, 1, H, W, 8)
    assert V._pool_sfx(H, W) == ""                                        # the wrappers run the even-only entries here
    y0, g0, a0 = V.pool_fwd(actd), V.pool_bwd_relu(gyd, actd), V.pool_bwd_relu_add(gyd, actd, addd)
    y1, g1, a1 = torch.empty_like(y0), torch.empty_like(g0), torch.empty_like(a0)
    L.call("dhz_maxpool2x2_blocked_fwd_any", actd.data_ptr(), y1.data_ptr(), N, H, W, _st())
    L.call("dhz_maxpool2x2_blocked_bwd_any", gyd.data_ptr(), actd.data_ptr(), g1.data_ptr(), N, H, W, _st())
    L.call("dhz_maxpool2x2_blocked_bwd_add_any", gyd.data_ptr(), actd.data_ptr(), addd.data_ptr(), a1.data_ptr(), N, H, W, _st())
    torch.cuda.synchronize()
    for even, anysize in ((y0, y1), (g0, g1), (a0, a1)):
        assert torch.equal(even.view(torch.int32), anysize.view(torch.int32))


def test_pool_wrappers_run_odd_maps():
    """vgg.pool_fwd / pool_bwd_relu / pool_bwd_relu_add on an odd map: the `_any` entries, the shapes of floor mode"""
    from dehaze_hip import vgg as V
    N, H, W = 2, 5, 7
    act, gy, add, pooled64, ref, ref_add = pool_case(N, H, W)
    actd, gyd, addd = act.cuda().view(N, 1, H, W, 8), gy.cuda().view(N, 1, 2, 3, 8), add.cuda().view(N, 1, H, W, 8)
    y = V.pool_fwd(actd)
    assert y.shape == (N, 1, 2, 3, 8) and torch.equal(y.cpu().view(N, 2, 3, 8).double(), pooled64)
    assert torch.allclose(V.pool_bwd_relu(gyd, actd).cpu().view(N, H, W, 8).double(), ref, rtol=1e-6, atol=0)
    assert torch.allclose(V.pool_bwd_relu_add(gyd, actd, addd).cpu().view(N, H, W, 8).double(), ref_add, rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 2. the L1 mean on any count
L1_COUNTS = [1, 3, 6, 8 * 5 + 2, 3 * 768 * 256 * 4 + 1024 + 3]            # ..., 8 k + 2, three grid passes of the 768-workgroup grid and a tail


def l1_case(n, seed):
    gen = torch.Generator().manual_seed(seed)
    a, p, q = (torch.randn(n, generator=gen) * 2 for _ in range(3))
    if n >= 6:                                                            # exact ties: sign 0, in the head and in the tail
        p[:2] = a[:2]
        p[n - 1] = a[n - 1]
    return a, p, q


@pytest.mark.parametrize("n", L1_COUNTS)
@pytest.mark.parametrize("with_n", [False, True])
def test_l1_pair_any_against_float64(n, with_n):
    L = _lib()
    a, p, q = l1_case(n, seed=n)
    ad, pd, qd = a.cuda(), p.cuda(), q.cuda()
    sums = torch.zeros(2, device="cuda")
    L.call("dhz_l1_pair_fwd_any", ad.data_ptr(), pd.data_ptr(), qd.data_ptr() if with_n else None, sums.data_ptr(), n, _st())
    rp = (a.double() - p.double()).abs().sum().item()
    rn = (a.double() - q.double()).abs().sum().item()
    print(f"l1_pair_any n={n} with_n={with_n}: sums {sums.tolist()} ref {rp} {rn}")
    assert abs(sums[0].item() - rp) <= 1e-5 * rp
    assert abs(sums[1].item() - rn) <= 1e-5 * rn if with_n else sums[1].item() == 0.0
    gsc = torch.tensor([0.7, -1.3], device="cuda")
    buf = guarded(n)
    L.call("dhz_l1_pair_bwd_any", ad.data_ptr(), pd.data_ptr(), qd.data_ptr() if with_n else None, gsc.data_ptr(), buf.data_ptr(), n, _st())
    da = take(buf, (n,))
    g64 = gsc.cpu().double()
    ref = g64[0] / n * torch.sign(a.double() - p.double())
    if with_n:
        # the two terms as the kernel forms them, in fp32 (their sum cancels where the signs differ: test_l1_pair_fp32's reference)
        gc = gsc.cpu()
        ref = (gc[0] / n * torch.sign(a - p) + gc[1] / n * torch.sign(a - q)).double()
    assert torch.allclose(da.double(), ref, rtol=1e-6, atol=0), (da.double() - ref).abs().max()
    if not with_n and n >= 6:
        assert (da[:2] == 0).all() and da[n - 1] == 0 and (da[2:n - 1] != 0).all()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_l1_pair_any_on_pointers_off_the_16_byte_grid(offset):
    """a head before the float4 body (all pointers `offset` floats behind a 16-byte boundary), and pointers that never align together (no
    body: every element singly)"""
    L = _lib()
    n = 4099
    a, p, _ = l1_case(n + 8, seed=offset)
    ad, pd = a.cuda(), p.cuda()
    gsc = torch.tensor([0.7, 0.0], device="cuda")
    for po in (offset, (offset + 1) % 4):
        av, pv = a[offset:offset + n], p[po:po + n]
        sums = torch.zeros(2, device="cuda")
        L.call("dhz_l1_pair_fwd_any", ad.data_ptr() + 4 * offset, pd.data_ptr() + 4 * po, None, sums.data_ptr(), n, _st())
        want = (av.double() - pv.double()).abs().sum().item()
        assert abs(sums[0].item() - want) <= 1e-5 * want
        buf = guarded(n + 4)
        L.call("dhz_l1_pair_bwd_any", ad.data_ptr() + 4 * offset, pd.data_ptr() + 4 * po, None, gsc.data_ptr(), buf.data_ptr() + 4 * offset, n, _st())
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.isnan(host[:offset]).all() and torch.isnan(host[offset + n:]).all(), "written outside [offset, offset + n)"
        ref = gsc.cpu().double()[0] / n * torch.sign(av.double() - pv.double())
        assert torch.allclose(host[offset:offset + n].double(), ref, rtol=1e-6, atol=0)


def test_l1_pair_any_equals_the_even_entry_bit_for_bit():
    """count % 4 == 0 on 16-byte aligned pointers: the same launch geometry and per-workgroup arithmetic.  The backward and the deterministic
    forward are compared bit for bit at a count of several grid passes; the default forward adds its workgroup sums with fp32 atomics in
    arrival order, so it is compared bit for bit at a count of ONE workgroup (one atomic), where that order does not exist."""
    from dehaze_hip import ops
    L = _lib()
    gsc = torch.tensor([0.7, -1.3], device="cuda")

    def both(n, qd, ad, pd):
        out = []
        for sfx in ("", "_any"):
            s = torch.zeros(2, device="cuda")
            L.call("dhz_l1_pair_fwd" + sfx, ad.data_ptr(), pd.data_ptr(), qd, s.data_ptr(), n, _st())
            d = torch.empty(n, device="cuda")
            L.call("dhz_l1_pair_bwd" + sfx, ad.data_ptr(), pd.data_ptr(), qd, gsc.data_ptr(), d.data_ptr(), n, _st())
            out.append((s.cpu(), d.cpu()))
        return out

    a, p, q = l1_case(1024, seed=5)
    ad, pd, qd = a.cuda(), p.cuda(), q.cuda()
    for qp in (None, qd.data_ptr()):
        (s0, d0), (s1, d1) = both(1024, qp, ad, pd)
        assert torch.equal(s0, s1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    n = 3 * 768 * 256 * 4 + 1024
    a, p, q = l1_case(n, seed=6)
    ad, pd, qd = a.cuda(), p.cuda(), q.cuda()
    (_, d0), (_, d1) = both(n, qd.data_ptr(), ad, pd)
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    try:
        ops.set_deterministic(True)
        ops._stream()
        (s0, _), (s1, _) = both(n, qd.data_ptr(), ad, pd)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(s0, s1), (s0, s1)


def test_l1_pair_any_deterministic_mode():
    from dehaze_hip import ops
    L = _lib()
    n = L1_COUNTS[-1]
    a, p, _ = l1_case(n, seed=2)
    ad, pd = a.cuda(), p.cuda()

    def run():
        s = torch.zeros(2, device="cuda")
        L.call("dhz_l1_pair_fwd_any", ad.data_ptr(), pd.data_ptr(), None, s.data_ptr(), n, _st())
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
    want = (a.double() - p.double()).abs().sum().item()
    assert abs(d1[0].item() - want) <= 1e-5 * want and abs(plain[0].item() - want) <= 1e-5 * want
