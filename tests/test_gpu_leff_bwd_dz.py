"""-m gpu: the LeFF depthwise backward that forms dz = dy . W2 itself (dhz_leff_dwconv_bwd_dy, csrc/leff_dwconv_dz.hip) against float64,
against the kernel chain it replaces (backward-data GEMM + dhz_leff_dwconv_bwd_scaled_dt), in its multi-trip regime, in deterministic
mode, and through fused.leff_branch with the planes of a FlatAdamW.

Bounds (none of them measured on the kernel):
  du    the depthwise backward's own bound (tests/test_gpu_kernels.py::test_leff_dwconv: 2e-5 + 1e-4 |ref|) plus the six-term bound of the
        project, 2^-21 sum |dy||W2| (tests/test_gpu_split.py), carried linearly through the per-image scale, |gelu'(t)|, sum_k |w_k| over
        the nine neighbours and |gelu'(u)|;
  dw/db the reordering bound of tests/test_gpu_persistent.py, RED * mag + floor (1e-5 against float64, 1e-6 between grids), mag = the same
        sums over the magnitudes of their terms (|dy||W2| for dz);
  chain the chain's dz comes from the fp32 pipe (C = 32) or a six-term kernel: 2^-19 sum |dy||W2| (the fp32-pipe row of
        tests/test_gpu_persistent.py) covers both; the two results may differ by the sum of both bounds."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from _grid import LEVELS, assert_trips, reserved_grid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RED = 2.0 ** -18
BOUND6 = 2.0 ** -21
BOUND_F32 = 2.0 ** -19


def _s():
    return torch.cuda.current_stream().cuda_stream


def _scale(B):
    sc = torch.ones(B)
    sc[-1] = 1.0 / 0.7
    if B > 1:
        sc[0 if B == 2 else 1] = 0.0
    return sc


def _inputs(C, B, H, W):
    g = torch.Generator().manual_seed(1000 * C + 100 * B + H + W)
    Ch, T = 4 * C, B * H * W
    d = dict(C=C, Ch=Ch, B=B, H=H, W=W, T=T)
    d["dy"] = torch.randn(T, C, generator=g).to(DEV)
    d["w2"] = (torch.randn(C, Ch, generator=g) / math.sqrt(C)).to(DEV)
    d["u"] = torch.randn(T, Ch, generator=g).to(DEV)
    d["tp"] = (1.4 * torch.rand(T, Ch, generator=g) - 0.2).to(DEV)
    d["wd"] = (0.3 * torch.randn(Ch, 9, generator=g)).to(DEV)
    d["sc"] = _scale(B).to(DEV)
    return d


def _planes(w2):
    """the three bf16 truncation planes of W2^T [Ch, C]"""
    from dehaze_hip import _lib
    wt = w2.t().contiguous()
    pl = torch.empty((3, wt.numel()), device=DEV, dtype=torch.bfloat16)
    _lib.call("dhz_split3_planes", wt.data_ptr(), wt.numel(), pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _s())
    return pl


def _run_new(d, pl):
    from dehaze_hip import _lib
    du = torch.full_like(d["u"], float("nan"))
    dw = torch.zeros(d["Ch"] * 9, device=DEV)
    db = torch.zeros(d["Ch"], device=DEV)
    _lib.call("dhz_leff_dwconv_bwd_dy", d["dy"].data_ptr(), d["C"], pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), d["u"].data_ptr(),
              d["tp"].data_ptr(), d["wd"].data_ptr(), du.data_ptr(), dw.data_ptr(), db.data_ptr(), d["sc"].data_ptr(), d["B"], d["H"], d["W"],
              d["C"], d["Ch"], _s())
    torch.cuda.synchronize()
    return du, dw, db


def _run_chain(d):
    from dehaze_hip import _lib, ops
    dz = ops.gemm_dgrad(d["dy"], d["w2"])
    du = torch.full_like(d["u"], float("nan"))
    dw = torch.zeros(d["Ch"] * 9, device=DEV)
    db = torch.zeros(d["Ch"], device=DEV)
    _lib.call("dhz_leff_dwconv_bwd_scaled_dt", dz.data_ptr(), d["u"].data_ptr(), d["tp"].data_ptr(), d["wd"].data_ptr(), du.data_ptr(),
              dw.data_ptr(), db.data_ptr(), d["sc"].data_ptr(), d["B"], d["H"], d["W"], d["Ch"], 0, _s())
    torch.cuda.synchronize()
    return du, dw, db


def _img(x, d):
    return x.view(d["B"], d["H"], d["W"], d["Ch"]).permute(0, 3, 1, 2)


def _reference(d):
    """float64: (du, dw, db), and per output the propagated sum |dy||W2| (unit: one relative error of the product) and the magnitudes
    of the reduced sums"""
    B, H, W, Ch = d["B"], d["H"], d["W"], d["Ch"]
    dy, w2, tp, sc = d["dy"].double(), d["w2"].double(), d["tp"].double(), d["sc"].double()
    rows = sc.repeat_interleave(H * W).view(-1, 1)
    dt = rows * (dy @ w2) * tp
    dtmag = rows * (dy.abs() @ w2.abs()) * tp.abs()
    u = d["u"].double().requires_grad_()
    wd = d["wd"].double().view(Ch, 1, 3, 3).requires_grad_()
    out = F.conv2d(_img(F.gelu(u), d), wd, padding=1, groups=Ch)
    (out * _img(dt, d)).sum().backward()
    ref = (u.grad, wd.grad.reshape(-1), dt.sum(0))
    ud = d["u"].double()
    gp = 0.5 * (1 + torch.erf(ud / math.sqrt(2))) + ud * torch.exp(-0.5 * ud * ud) / math.sqrt(2 * math.pi)
    wabs = d["wd"].double().abs().view(Ch, 1, 3, 3).requires_grad_()
    du_mag = gp.abs() * F.conv_transpose2d(_img(dtmag, d), wabs.detach(), padding=1, groups=Ch).permute(0, 2, 3, 1).reshape(-1, Ch)
    (F.conv2d(_img(F.gelu(ud).abs(), d), wabs, padding=1, groups=Ch) * _img(dtmag, d)).sum().backward()
    return ref, (du_mag, wabs.grad.reshape(-1), dtmag.sum(0))


def _check(tag, got, ref, mag, prod_bound):
    du, dw, db = (t.double() for t in got)
    err = (du - ref[0]).abs()
    bound = 2e-5 + 1e-4 * ref[0].abs() + prod_bound * mag[0]
    print(tag, "du max err / bound", (err / bound).max().item())
    assert (err <= bound).all(), (tag, "du", (err / bound).max().item())
    for name, g, r, m in (("dw", dw, ref[1], mag[1]), ("db", db, ref[2], mag[2])):
        e = (g - r).abs()
        b = RED * m + 1e-5
        print(tag, name, "max err / bound", (e / b).max().item())
        assert (e <= b).all(), (tag, name, (e / b).max().item())
    return bound


@pytest.mark.parametrize("C,B,H,W", [(32, 2, 16, 16), (32, 1, 8, 48), (64, 3, 12, 24), (128, 2, 16, 16)])
def test_raw_abi_vs_fp64_and_chain(C, B, H, W):
    d = _inputs(C, B, H, W)
    assert (H * W) % 32 == 0
    ref, mag = _reference(d)
    new = _run_new(d, _planes(d["w2"]))
    chain = _run_chain(d)
    b_new = _check("new", new, ref, mag, BOUND6)
    b_chain = _check("chain", chain, ref, mag, BOUND_F32)
    zero = (d["sc"] == 0).repeat_interleave(H * W)
    if zero.any():
        assert new[0][zero].abs().max().item() == 0.0            # the dropped image passes no gradient
    diff = (new[0].double() - chain[0].double()).abs()
    assert (diff <= b_new + b_chain).all(), (diff / (b_new + b_chain)).max().item()
    for k in (1, 2):
        diff = (new[k].double() - chain[k].double()).abs()
        assert (diff <= 2 * (RED * mag[k] + 1e-5)).all(), k


@pytest.mark.parametrize("C", [32, 64])
def test_multi_trip(C):
    """20 tiles of one channel group on grids sized for 8 and 9 CUs: 6 (C = 32) / 3 (C = 64) workgroups per channel group"""
    B, H, W = 1, 40, 64
    d = _inputs(C, B, H, W)
    pl = _planes(d["w2"])
    ref, mag = _reference(d)
    ntiles, ncg = B * ((H + 7) // 8) * ((W + 15) // 16), d["Ch"] // 32
    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            if lvl is not None:
                assert_trips("depthwise backward with dz", ntiles, min(ntiles, max(1, 3 * ncu // ncg)))
            res[lvl] = _run_new(d, pl)
    for lvl in LEVELS:
        _check(lvl, res[lvl], ref, mag, BOUND6)
        if lvl is not None:
            assert torch.equal(res[lvl][0], res[None][0]), (lvl, "du depends on the grid")
            for k, name in ((1, "dw"), (2, "db")):
                e = (res[lvl][k].double() - res[None][k].double()).abs()
                assert (e <= RED * mag[k] + 1e-6).all(), (lvl, name)


@contextlib.contextmanager
def _deterministic():
    from dehaze_hip import _lib, ops
    try:
        ops.set_deterministic(True, None)
        assert _lib.load().dhz_get_deterministic() == 1
        ops._stream()                 # hands the workspace to the library
        yield
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("C,B,H,W", [(32, 2, 24, 40), (64, 3, 12, 24), (128, 2, 16, 16)])
def test_deterministic_mode_repeats_bit_for_bit(C, B, H, W):
    d = _inputs(C, B, H, W)
    pl = _planes(d["w2"])
    ref, mag = _reference(d)
    with _deterministic():
        a = _run_new(d, pl)
        b = _run_new(d, pl)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _check("deterministic", a, ref, mag, BOUND6)


def _leff_reference(x, norm, mlp, scale, H, W):
    B, L, C = x.shape
    xn = F.layer_norm(x, (C,), norm.weight, norm.bias, 1e-5)
    u = F.gelu(F.linear(xn, mlp.linear1[0].weight, mlp.linear1[0].bias))
    m = u.view(B, H, W, -1).permute(0, 3, 1, 2)
    t = F.gelu(F.conv2d(m, mlp.dwconv[0].weight, mlp.dwconv[0].bias, padding=1, groups=m.shape[1]))
    z = t.permute(0, 2, 3, 1).reshape(B, L, -1)
    y = F.linear(z, mlp.linear2[0].weight, mlp.linear2[0].bias)
    return x + scale.view(B, 1, 1) * y


@pytest.mark.parametrize("C,H,W,B", [(32, 16, 16, 2), (64, 16, 32, 3), (128, 16, 16, 2)])
def test_through_leff_branch(C, H, W, B):
    import copy
    import My_model_1 as M1
    from dehaze_hip import _lib, fused, ops
    from dehaze_hip.train import FlatAdamW
    torch.manual_seed(C + H + W)
    net = torch.nn.ModuleDict({"norm": torch.nn.LayerNorm(C), "mlp": M1.LeFF(C, 4 * C)})
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(B, H * W, C)
    gout = torch.randn(B, H * W, C)
    scale = _scale(B)
    n64 = copy.deepcopy(net).double()
    x64 = x.double().requires_grad_()
    (_leff_reference(x64, n64["norm"], n64["mlp"], scale.double(), H, W) * gout.double()).sum().backward()
    ref = {"dx": x64.grad}
    ref.update({n_: p.grad for n_, p in n64.named_parameters()})

    def run(on):
        saved = (fused.LEFF_BWD_DZ, fused.LEFF_BWD_DZ_C, ops.SPLIT_SHADOW, ops.SHADOW_OWNER, _lib.call)
        names = []

        def spy(name, *args):
            names.append(name)
            return saved[4](name, *args)

        nd = copy.deepcopy(net).to(DEV)
        opt = FlatAdamW(nd)
        try:
            fused.LEFF_BWD_DZ, fused.LEFF_BWD_DZ_C = on, (32, 64, 128)
            opt.zero_grad()
            opt.enable_split_shadow()
            assert ops.split_planes_t(nd["mlp"].linear2[0].weight) is not None
            xd = x.to(DEV).requires_grad_()
            y = fused.leff_branch(xd, nd["norm"], nd["mlp"], scale.to(DEV), H, W)
            _lib.call = spy
            (y * gout.to(DEV)).sum().backward()
            _lib.call = saved[4]
            torch.cuda.synchronize()
            out = {"dx": xd.grad.cpu().double()}
            out.update({n_: p.grad.cpu().double() for n_, p in nd.named_parameters()})
            return out, names
        finally:
            fused.LEFF_BWD_DZ, fused.LEFF_BWD_DZ_C, ops.SPLIT_SHADOW, ops.SHADOW_OWNER, _lib.call = saved

    (got, on_names), (chain, off_names) = run(True), run(False)
    assert on_names.count("dhz_leff_dwconv_bwd_dy") == 1 and "dhz_leff_dwconv_bwd_scaled_dt" not in on_names
    assert "dhz_leff_dwconv_bwd_dy" not in off_names and off_names.count("dhz_leff_dwconv_bwd_scaled_dt") == 1
    # the only other difference: ONE token-Linear product that is no weight gradient - backward-data of linear2
    rest_on = sorted(n for n in on_names if n != "dhz_leff_dwconv_bwd_dy")
    rest_off = sorted(n for n in off_names if n != "dhz_leff_dwconv_bwd_scaled_dt")
    extra = list(rest_off)
    for n in rest_on:
        extra.remove(n)
    assert len(extra) == 1 and extra[0].startswith("dhz_linear_") and "wgrad" not in extra[0], extra
    for k, r in ref.items():
        tol = 3e-5 + 3e-5 * r.abs().max().item()
        if k != "dx":
            tol *= (B * H * W) ** 0.5                   # sums over all tokens
        for tag, o in (("dz in the kernel", got), ("chain", chain)):
            e = (o[k] - r).abs().max().item()
            print(tag, k, e, tol)
            assert e < tol, (tag, k, e, tol)
