"""-m gpu: the Downsample convolution (4 x 4, stride 2, pad 1, token layout) on the six-term plane kernels - dhz_conv4s2_prepack6,
dhz_conv4s2_fwd6, dhz_conv4s2_dgrad6 (csrc/split6_gemm.hip, the gathered forms of split6_gemm_kernel) - through the raw C entries
against a float64 torch.nn.functional.conv2d and its autograd on the CPU.

Bound on every element: the project's six-term bound |err| <= 2^-21 mag + 1e-7 (S6_BOUND, S6_FLOOR of tests/_tile_cases.py), mag = the
same convolution over absolute values in float64: |x| with |w| plus |b| (forward), |dy| with |w| (backward-data).  The first five
shapes are those of tests/test_gpu_conv.py::test_conv4s2_c_abi, so the fp32 entries serve as a second reference; (2, 64, 64, 32, 64)
also runs on grids sized for 8 and for 9 CUs: more tiles than workgroups and, at 9, a workgroup of the backward-data launch whose
parity class changes between two of its tiles.  y and dx are NaN before every call and no NaN survives; the planes of the prepack
equal dhz_split3_planes of the permuted weight bit for bit; the tile query names every gathered instance over the cases; bad
arguments return -22.  Each case prints its worst err / bound share (profiles/conv4s2_split6.txt)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import _tile_cases as TC
from _grid import reserved_grid

pytestmark = pytest.mark.gpu

#        (B, H, W, Cin, Cout)
CASES = ((2, 16, 16, 32, 64),       # smallest legal channels; one stage per tap; all four borders
         (1, 32, 16, 64, 128),      # non-square map; two stages per tap
         (3, 8, 8, 128, 256),       # 48 output rows: a ragged row tile
         (1, 8, 16, 256, 512),      # K = 4096 with 32 rows, far fewer rows than one tile
         (1, 26, 18, 32, 64),       # odd 13 x 9 output map, no power of two
         (2, 64, 64, 32, 64))       # 16 forward tiles, 64 backward-data tiles: more tiles than workgroups at 8 / 9 CUs
BIG = CASES[5]
FWD_INSTANCES, DGRAD_INSTANCES = {44, 42}, {44, 42, 41}


def _levels(case):
    return (None, 8, 9) if case == BIG else (None,)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """float32 operands and the float64 references of one case (CPU), computed once and shared"""
    B, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(B + H + W + Cin)
    x = torch.randn(B, H * W, Cin, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) * 0.05
    b = torch.randn(Cout, generator=g) * 0.1
    xr = x.double().view(B, H, W, Cin).permute(0, 3, 1, 2).requires_grad_()
    yr = F.conv2d(xr, w.double(), b.double(), stride=2, padding=1)
    gy = torch.randn(yr.shape, generator=g).double()
    (yr * gy).sum().backward()
    tok = lambda t: t.detach().permute(0, 2, 3, 1).reshape(B, -1, t.shape[1]).contiguous()
    ymag = F.conv2d(xr.detach().abs(), w.double().abs(), b.double().abs(), stride=2, padding=1)
    dxmag = F.conv_transpose2d(gy.abs(), w.double().abs(), stride=2, padding=1)
    return dict(x=x, w=w, b=b, dy=tok(gy).float(), y=tok(yr), ymag=tok(ymag), dx=tok(xr.grad), dxmag=tok(dxmag))


def _share(got, ref, mag):
    """worst |err| / bound over the elements"""
    return ((got.cpu().double() - ref).abs() / (TC.S6_BOUND * mag + TC.S6_FLOOR)).max().item()


def _prepack(lib, wd, Cin, Cout, s):
    n = 16 * Cin * Cout
    pf = torch.full((3, n), -1, device=wd.device, dtype=torch.int16)
    pb = torch.full((3, n), -1, device=wd.device, dtype=torch.int16)
    assert lib.dhz_conv4s2_prepack6(wd.data_ptr(), pf.data_ptr(), pb.data_ptr(), Cin, Cout, s) == 0
    return pf, pb


def _split3(lib, t, s):
    out = torch.empty((3, t.numel()), device=t.device, dtype=torch.int16)
    assert lib.dhz_split3_planes(t.data_ptr(), t.numel(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), s) == 0
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv4s2_split6_c_abi(case):
    from dehaze_hip import _lib
    lib = _lib.load()
    TC.s6_no_override()
    B, H, W, Cin, Cout = case
    R = _reference(case)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    xd, wd, bd, dyd = (R[k].to(dev) for k in ("x", "w", "b", "dy"))
    pf, pb = _prepack(lib, wd, Cin, Cout, s)
    # the planes: bit for bit those of dhz_split3_planes over the permuted weight
    assert torch.equal(pf, _split3(lib, wd.permute(0, 2, 3, 1).contiguous(), s))
    assert torch.equal(pb, _split3(lib, wd.permute(1, 2, 3, 0).contiguous(), s))
    # the fp32 entries: a second reference
    wp = wd.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).contiguous()
    wq = wd.permute(2, 3, 0, 1).contiguous()
    y32 = torch.empty(B, (H // 2) * (W // 2), Cout, device=dev)
    dx32 = torch.empty(B, H * W, Cin, device=dev)
    _lib.call("dhz_conv4s2_fwd", xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y32.data_ptr(), B, H, W, Cin, Cout, s)
    _lib.call("dhz_conv4s2_dgrad", dyd.data_ptr(), wq.data_ptr(), dx32.data_ptr(), B, H, W, Cin, Cout, s)
    tol_y = (3e-6 * (16 * Cin) ** 0.5 + 1e-5) * max(1.0, R["y"].abs().max().item())        # the bounds of test_conv4s2_c_abi
    tol_dx = (3e-6 * (4 * Cout) ** 0.5 + 1e-5) * max(1.0, R["dx"].abs().max().item())
    for ncu in _levels(case):
        with reserved_grid(ncu) as n:
            tf, td = lib.dhz_conv4s2_tile6(1, B, H, W, Cin, Cout), lib.dhz_conv4s2_tile6(2, B, H, W, Cin, Cout)
            assert tf in FWD_INSTANCES and td in DGRAD_INSTANCES
            y = torch.full_like(y32, float("nan"))
            dx = torch.full_like(dx32, float("nan"))
            assert lib.dhz_conv4s2_fwd6(xd.data_ptr(), pf.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W, Cin, Cout, s) == 0
            assert lib.dhz_conv4s2_dgrad6(dyd.data_ptr(), pb.data_ptr(), dx.data_ptr(), B, H, W, Cin, Cout, s) == 0
            torch.cuda.synchronize()
        assert not torch.isnan(y).any() and not torch.isnan(dx).any(), "an element was not written"
        sy, sdx = _share(y, R["y"], R["ymag"]), _share(dx, R["dx"], R["dxmag"])
        print(f"conv4s2_split6 {case} cus={n}: fwd tile {tf} err/bound {sy:.3f}   dgrad tile {td} err/bound {sdx:.3f}")
        assert sy <= 1.0, f"forward: worst err / bound {sy}"
        assert sdx <= 1.0, f"backward-data: worst err / bound {sdx}"
        assert ((y - y32).abs().cpu().double() <= TC.S6_BOUND * R["ymag"] + TC.S6_FLOOR + tol_y).all()
        assert ((dx - dx32).abs().cpu().double() <= TC.S6_BOUND * R["dxmag"] + TC.S6_FLOOR + tol_dx).all()
    if case == CASES[0]:                                           # without bias
        y = torch.full_like(y32, float("nan"))
        assert lib.dhz_conv4s2_fwd6(xd.data_ptr(), pf.data_ptr(), None, y.data_ptr(), B, H, W, Cin, Cout, s) == 0
        assert _share(y, R["y"] - R["b"].double(), R["ymag"] - R["b"].double().abs()) <= 1.0


def test_conv4s2_split6_every_instance_is_reached():
    from dehaze_hip import _lib
    lib = _lib.load()
    TC.s6_no_override()
    seen = {1: set(), 2: set()}
    for case in CASES:
        for ncu in _levels(case):
            with reserved_grid(ncu):
                for mode in (1, 2):
                    seen[mode].add(lib.dhz_conv4s2_tile6(mode, *case))
    assert seen[1] == FWD_INSTANCES and seen[2] == DGRAD_INSTANCES, seen


def test_conv4s2_split6_bad_arguments():
    from dehaze_hip import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    B, H, W, Cin, Cout = 1, 8, 8, 32, 64
    x = torch.zeros(B, H * W, Cin, device=dev)
    w = torch.zeros(Cout, Cin, 4, 4, device=dev)
    y = torch.zeros(B, H * W // 4, Cout, device=dev)
    pf, pb = _prepack(lib, w, Cin, Cout, s)
    p = lambda t: t.data_ptr()
    assert lib.dhz_conv4s2_fwd6(p(x), p(pf), None, p(y), B, H + 1, W, Cin, Cout, s) == -22          # odd map
    assert lib.dhz_conv4s2_fwd6(p(x), p(pf), None, p(y), B, H, W, Cin, 32, s) == -22               # forward: features in 64s
    assert lib.dhz_conv4s2_fwd6(p(x), p(pf), None, p(y), B, H, W, 16, Cout, s) == -22
    assert lib.dhz_conv4s2_fwd6(p(x), None, None, p(y), B, H, W, Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_fwd6(p(x), p(pf), None, p(y), 0, H, W, Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_dgrad6(p(y), p(pb), p(x), B, H, W + 1, Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_dgrad6(p(y), p(pb), p(x), B, H, W, Cin, 48, s) == -22
    assert lib.dhz_conv4s2_dgrad6(p(y), p(pb), None, B, H, W, Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_prepack6(p(w), p(pf), p(pb), 16, Cout, s) == -22
    assert lib.dhz_conv4s2_prepack6(p(w), None, None, Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_prepack6(None, p(pf), p(pb), Cin, Cout, s) == -22
    assert lib.dhz_conv4s2_tile6(1, B, H, W, Cin, 32) == 0 and lib.dhz_conv4s2_tile6(2, B, H, W, Cin, 32) == 41
    assert lib.dhz_conv4s2_tile6(3, B, H, W, Cin, Cout) == 0 and lib.dhz_conv4s2_tile6(1, B, H + 1, W, Cin, Cout) == 0
    torch.cuda.synchronize()


def test_downsample_module_switch_on_against_off(monkeypatch):
    """Downsample(32 -> 64) at B = 2, 16 x 16 with both products on the six-term entries against the same module on the fp32 entries:
    forward and dx within the sum of the two bounds (six-term bound + the fp32 entries' tolerance of test_conv4s2_c_abi), dW / db inside
    the tolerance of test_downsample_module_matches_library_conv."""
    import My_model_1 as M1
    from dehaze_hip import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    B, H, W, Cin, Cout = 2, 16, 16, 32, 64
    ds = M1.Downsample(Cin, Cout).to(dev)
    x = torch.randn(B, H * W, Cin, device=dev)
    gout = torch.randn(B, H * W // 4, Cout, device=dev)
    monkeypatch.setattr(ops, "SPLIT_BF16", 6)
    monkeypatch.setattr(ops, "CONV4S2_SPLIT6_FWD", {(Cin, Cout)})
    monkeypatch.setattr(ops, "CONV4S2_SPLIT6_DGRAD", {(Cin, Cout)})
    assert not ops.DETERMINISTIC

    def run(on):
        monkeypatch.setattr(ops, "CONV4S2_SPLIT6", on)
        assert ops._conv4s2_split6(Cin, Cout) == (on, on)
        ds.zero_grad(set_to_none=True)
        xa = x.clone().requires_grad_()
        ya = ds(xa)
        ya.backward(gout)
        return ya.detach(), xa.grad.clone(), ds.conv[0].weight.grad.clone(), ds.conv[0].bias.grad.clone()

    y1, dx1, dw1, db1 = run(True)
    y0, dx0, dw0, db0 = run(False)
    w64, b64 = ds.conv[0].weight.detach().double().cpu(), ds.conv[0].bias.detach().double().cpu()
    xm = x.double().cpu().view(B, H, W, Cin).permute(0, 3, 1, 2)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(B, -1, t.shape[1])
    ymag = tok(F.conv2d(xm.abs(), w64.abs(), b64.abs(), stride=2, padding=1))
    gm = gout.double().cpu().view(B, H // 2, W // 2, Cout).permute(0, 3, 1, 2)
    dxmag = tok(F.conv_transpose2d(gm.abs(), w64.abs(), stride=2, padding=1))
    tol_y = (3e-6 * (16 * Cin) ** 0.5 + 1e-5) * max(1.0, y0.abs().max().item())
    tol_dx = (3e-6 * (4 * Cout) ** 0.5 + 1e-5) * max(1.0, dx0.abs().max().item())
    assert ((y1 - y0).abs().cpu().double() <= TC.S6_BOUND * ymag + TC.S6_FLOOR + tol_y).all()
    assert ((dx1 - dx0).abs().cpu().double() <= TC.S6_BOUND * dxmag + TC.S6_FLOOR + tol_dx).all()
    assert torch.allclose(dw1, dw0, atol=2e-3, rtol=1e-3), (dw1 - dw0).abs().max()
    assert torch.allclose(db1, db0, atol=2e-3, rtol=1e-3)
