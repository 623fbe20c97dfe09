"""-m gpu: the Mlp activation of token_mlp = 'ffn' (dhz_gelu_fwd_dt / dhz_gelu_bwd_dt, csrc/elementwise.hip) through the raw C-ABI,
fp32 and bf16 storage, against float64 0.5 u (1 + erf(u / sqrt 2)) and its derivative on the CPU.

Inputs: 3 * randn with a planted grid of u from -9 to 9 (the tails, where the kernel's 1 - poly * e cancels), +-0.0 and +-1e-30.
Lengths: one float4; a ragged last workgroup; and more than the capped grid (2048 workgroups x 256 threads x 4 elements) covers in one
stride, so the grid-stride loop runs on.  The backward's per-image factor (the DropPath scale that ops._GeluTokens never passes) is
checked with scale = [0, 1 / 0.9, 1].

Bounds.  fp32: those under which test_leff_dwconv (tests/test_gpu_kernels.py:206-207) checks the same gelu_both4 - forward atol 1e-5 /
rtol 1e-5, backward atol 2e-5 / rtol 1e-4.
bf16: the kernels convert to fp32 on load, run the fp32 arithmetic and round once on the store, so (a) against the fp32 kernel on the
same bf16-representable inputs, rounded to bf16, the rule tests/test_gpu_bf16.py:107 states for its streaming kernels holds:
    bool((d <= 2.0 ** -7 * torch.maximum(a.float().abs(), b.float().abs())).all())
i.e. at most one bf16 step; and (b) against the float64 value rounded to bf16, the same one step plus the fp32 bound above - the stored
value cannot be closer to float64 than the fp32 value it is rounded from (the absolute part matters only in the negative tail, where
|gelu| < 1e-5 and the polynomial's 1.5e-7 error of erf is no longer small against the value; everywhere else it is below 2^-9 of it)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, BF16 = 0, 1                                   # DHZ_F32, DHZ_BF16
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}
GRID_CAP = 2048 * 256 * 4                          # elements one stride of the capped grid covers (grid_for: 256 * 8 workgroups)
LENGTHS = [4, 4 * 1031, GRID_CAP + 4 * 300]
SCALED_LENGTHS = [12, 12 * 1031, 12 * 174863]      # three images of n / 3 elements, n / 3 a multiple of 4
PAD = 64                                           # NaN elements behind every output
FWD_TOL, BWD_TOL = (1e-5, 1e-5), (2e-5, 1e-4)


def inputs(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    u = 3 * torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    u[:4] = special
    plant = torch.cat([special, torch.linspace(-9, 9, 361)])
    if n >= 2 * plant.numel():                                    # the grid at both ends: the first and the last stride of the long inputs
        u[:plant.numel()] = plant
        u[n - plant.numel():] = plant.flip(0)
    dy = torch.randn(n, generator=g)
    u, dy = u.to(TORCH_DT[dtype]), dy.to(TORCH_DT[dtype])         # bf16: the references start from the rounded values
    return u, dy


def gelu64(u):
    u = u.double()
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    return u * cdf, cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def gelu_fwd(u, dtype):
    from dehaze_hip import _lib
    n = u.numel()
    y = torch.full((n + PAD,), NAN, device="cuda", dtype=TORCH_DT[dtype])
    _lib.call("dhz_gelu_fwd_dt", u.data_ptr(), y.data_ptr(), n, dtype, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not torch.isnan(y[:n]).any() and torch.isnan(y[n:]).all()
    return y[:n].cpu()


def gelu_bwd(dy, u, dtype, scale=None, elems_per_scale=0):
    from dehaze_hip import _lib
    n = u.numel()
    du = torch.full((n + PAD,), NAN, device="cuda", dtype=TORCH_DT[dtype])
    _lib.call("dhz_gelu_bwd_dt", dy.data_ptr(), u.data_ptr(), du.data_ptr(), n, None if scale is None else scale.data_ptr(),
              elems_per_scale, dtype, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not torch.isnan(du[:n]).any() and torch.isnan(du[n:]).all()
    return du[:n].cpu()


def check(what, got, ref, tol, dtype):
    """fp32: |got - ref| <= atol + rtol |ref|.  bf16: one bf16 step around the rounded float64 value on top of that (module docstring)."""
    atol, rtol = tol
    err = (got.double() - ref).abs()
    bound = atol + rtol * ref.abs()
    if dtype == BF16:
        ref_bf = ref.float().to(torch.bfloat16).double()
        err = (got.double() - ref_bf).abs()
        bound = bound + 2.0 ** -7 * torch.maximum(got.double().abs(), ref_bf.abs())
    units = (err / bound).max().item()
    print(f"{what}: worst error {err.max().item():.3e}, {units:.3f} of the bound")
    assert units <= 1.0, (what, err.max().item(), units)


def one_bf16_step(what, a, b):
    d = (a.float() - b.float()).abs()
    print(f"{what}: {(a != b).float().mean().item():.2e} of the elements differ from the fp32 kernel's rounded result")
    assert bool((d <= 2.0 ** -7 * torch.maximum(a.float().abs(), b.float().abs())).all()), what


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", LENGTHS)
def test_gelu_forward_and_backward_match_float64(n, dtype):
    if n == LENGTHS[-1]:
        assert n > GRID_CAP and n % 4 == 0                      # the capped grid takes a second stride, ragged
    u, dy = inputs(n, dtype, 100 + n % 977)
    g64, gp64 = gelu64(u)
    ud, dyd = u.cuda(), dy.cuda()
    name = f"gelu {'bf16' if dtype else 'fp32'} n={n}"
    y = gelu_fwd(ud, dtype)
    du = gelu_bwd(dyd, ud, dtype)
    check(name + " forward", y, g64, FWD_TOL, dtype)
    check(name + " backward", du, dy.double() * gp64, BWD_TOL, dtype)
    if dtype == BF16:                                           # (a): the fp32 kernel on the same values, rounded once
        y32 = gelu_fwd(ud.float(), F32)
        du32 = gelu_bwd(dyd.float(), ud.float(), F32)
        one_bf16_step(name + " forward", y, y32.to(torch.bfloat16))
        one_bf16_step(name + " backward", du, du32.to(torch.bfloat16))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", SCALED_LENGTHS)
def test_gelu_backward_per_image_scale(n, dtype):
    """du = dy gelu'(u) scale[e / elems_per_scale] with three images: a dropped one (exactly zero), a kept one (1 / 0.9) and 1"""
    if n == SCALED_LENGTHS[-1]:
        assert n > GRID_CAP
    per = n // 3
    assert per * 3 == n and per % 4 == 0
    u, dy = inputs(n, dtype, 200 + n % 977)
    _, gp64 = gelu64(u)
    scale = torch.tensor([0.0, 1 / 0.9, 1.0])
    ud, dyd = u.cuda(), dy.cuda()
    du = gelu_bwd(dyd, ud, dtype, scale.cuda(), per)
    ref = dy.double() * gp64 * scale.double().repeat_interleave(per)          # the fp32 factor, as the kernel reads it
    check(f"gelu {'bf16' if dtype else 'fp32'} n={n} scaled backward", du, ref, BWD_TOL, dtype)
    assert (du[:per] == 0).all()
    ones = gelu_bwd(dyd, ud, dtype, torch.ones(3, device="cuda"), per)
    assert torch.equal(ones.view(torch.int16 if dtype else torch.int32), gelu_bwd(dyd, ud, dtype).view(torch.int16 if dtype else torch.int32))


def test_gelu_refusals():
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    n = 12 * 1031
    u = torch.randn(n, device="cuda")
    out = torch.full((n,), NAN, device="cuda")
    sc = torch.ones(3, device="cuda")
    for dtype in (F32, BF16):
        assert lib.dhz_gelu_fwd_dt(u.data_ptr(), out.data_ptr(), 6, dtype, s) == -22
        assert lib.dhz_gelu_bwd_dt(u.data_ptr(), u.data_ptr(), out.data_ptr(), 6, None, 0, dtype, s) == -22
        assert lib.dhz_gelu_bwd_dt(u.data_ptr(), u.data_ptr(), out.data_ptr(), n, sc.data_ptr(), 4000, dtype, s) == -22      # does not divide n
        assert lib.dhz_gelu_bwd_dt(u.data_ptr(), u.data_ptr(), out.data_ptr(), n, sc.data_ptr(), n // 2, dtype, s) == -22    # divides, not in 4s
    assert lib.dhz_gelu_fwd_dt(u.data_ptr(), out.data_ptr(), n, 7, s) == -22                                                 # no such storage type
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
