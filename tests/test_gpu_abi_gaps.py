"""-m gpu: exported entries that only whole-model tests reached and that are cheap to check on their own (the coverage guard of
tests/test_host.py lists what names every other entry):

  dhz_bias_gather_multi, dhz_fused_attn_prepack_multi, dhz_fused_attn_prepack6_multi - the once-per-forward staging of every block's
      bias tile and fragment-ordered weights in ONE launch: pure data movement (and, for the six-term planes, the same truncation
      arithmetic), so bit-equal to the gather in torch / to n calls of the single-entry form, which the kernel tests check;
  dhz_contrast_combine_fwd / _bwd - the scalar side of ContrastLoss over the taps, against float64 autograd;
  dhz_thin_conv3x3_fwd / dhz_thin_conv3x3_dgrad - the fp32 names of the output projection (the product calls the _dt forms), against
      float64 conv2d at the bounds of test_thin_conv3x3_vs_torch (tests/test_gpu_kernels.py: atol 2e-5, rtol 1e-4);
  dhz_split3_planes_t - the six-term planes of the transposed weights, against dhz_split3_planes of the transposed matrix."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import uformer_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _s():
    return torch.cuda.current_stream().cuda_stream


def ptrs(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def ints(values):
    arr = (ctypes.c_int * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def test_bias_gather_multi_is_the_gather():
    """blocks with 1, 4, 2 and 16 heads in one launch (the grid is sized for the widest: the narrower entries end early)"""
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(11)
    heads = [1, 4, 2, 16]
    tables = [torch.randn(225, H, generator=g) for H in heads]
    td = [t.cuda() for t in tables]
    out = [torch.full((H * 64 * 64 + 64,), NAN, device="cuda") for H in heads]
    ka, pa = ptrs(td)
    kb, pb = ptrs(out)
    kh, ph = ints(heads)
    _lib.call("dhz_bias_gather_multi", pa, pb, ph, len(heads), _s())
    torch.cuda.synchronize()
    ridx = O.relative_position_index(8).reshape(-1)
    for t, o, H in zip(tables, out, heads):
        assert torch.isnan(o[H * 64 * 64:]).all()
        assert torch.equal(o[:H * 64 * 64].view(H, 64, 64).cpu(), t[ridx].reshape(64, 64, H).permute(2, 0, 1))
    lib = _lib.load()
    assert lib.dhz_bias_gather_multi(pa, pb, ph, 0, _s()) == -22 and lib.dhz_bias_gather_multi(pa, pb, ph, 33, _s()) == -22
    del ka, kb, kh


def test_prepack_multi_equals_single_calls():
    """three blocks of C = 64, 32, 128 in one launch of each staging entry == three calls of dhz_fused_attn_prepack /
    dhz_fused_attn_prepack6, bit for bit, and nothing written behind any output"""
    from dehaze_hip import _lib, fused
    g = torch.Generator().manual_seed(12)
    Cs = [64, 32, 128]
    W = [[(torch.randn(C, C, generator=g) / C ** 0.5).cuda() for _ in range(4)] for C in Cs]
    pad = 64
    qkv_m = [torch.full((3 * C * C + pad,), NAN, device="cuda") for C in Cs]
    wo_m = [torch.full((C * C + pad,), NAN, device="cuda") for C in Cs]
    p6_m = [torch.full((fused._n6(C) + pad,), NAN, device="cuda").to(torch.bfloat16) for C in Cs]
    keep = [ptrs([w[k] for w in W]) for k in range(4)]
    kq, pq = ptrs(qkv_m)
    ko, po = ptrs(wo_m)
    k6, p6 = ptrs(p6_m)
    kc, pc = ints(Cs)
    _lib.call("dhz_fused_attn_prepack_multi", keep[0][1], keep[1][1], keep[2][1], keep[3][1], pq, po, pc, len(Cs), _s())
    _lib.call("dhz_fused_attn_prepack6_multi", keep[0][1], keep[1][1], keep[2][1], keep[3][1], p6, pc, len(Cs), _s())
    torch.cuda.synchronize()
    for i, C in enumerate(Cs):
        qkv = torch.full((3 * C * C,), NAN, device="cuda")
        wo = torch.full((C * C,), NAN, device="cuda")
        pk6 = torch.full((fused._n6(C),), NAN, device="cuda").to(torch.bfloat16)
        w = W[i]
        _lib.call("dhz_fused_attn_prepack", w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), qkv.data_ptr(), wo.data_ptr(), C, _s())
        _lib.call("dhz_fused_attn_prepack6", w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), pk6.data_ptr(), C, _s())
        torch.cuda.synchronize()
        assert not torch.isnan(qkv).any() and not torch.isnan(wo).any()
        assert torch.equal(qkv_m[i][:-pad], qkv) and torch.isnan(qkv_m[i][-pad:]).all(), C
        assert torch.equal(wo_m[i][:-pad], wo) and torch.isnan(wo_m[i][-pad:]).all(), C
        assert torch.equal(p6_m[i][:-pad].view(torch.int16), pk6.view(torch.int16)) and torch.isnan(p6_m[i][-pad:]).all(), C
        # the fp32 pack is a permutation of the four weights
        assert torch.equal(torch.cat([qkv, wo]).sort().values, torch.cat([t.reshape(-1) for t in w]).sort().values)
    del keep, kq, ko, k6, kc


@pytest.mark.parametrize("ablation", [False, True])
def test_contrast_combine_matches_float64(ablation):
    """loss = sum_i w_i ap_i / (an_i + 1e-7) (ablation: sum_i w_i ap_i), all_ap, all_an from the 2k L1 sums, and the 2k backward
    coefficients for incoming gradients of all three outputs.  Every quantity is a chain of fewer than ten fp32 operations on positive
    terms (the signs of the incoming gradients are chosen so that nothing cancels) plus a sum of k = 5 of them: 32 ulp = 32 * 2^-24
    relative is the bound."""
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(13)
    k = 5
    cnt = torch.tensor([64.0 * 128 * 128, 128.0 * 64 * 64, 256.0 * 32 * 32, 512.0 * 16 * 16, 512.0 * 8 * 8])
    sums = (0.2 + torch.rand(k, 2, generator=g)) * cnt.view(k, 1)
    w = torch.tensor([1 / 32, 1 / 16, 1 / 8, 1 / 4, 1.0])
    inv = (1.0 / cnt).float()
    gin = torch.tensor([0.8, 0.3, -0.2])                      # d / d loss, all_ap, all_an
    s64 = sums.double().requires_grad_()
    d64 = s64 * inv.double().view(k, 1)
    d64.retain_grad()
    ap, an = d64[:, 0], d64[:, 1]
    loss = (w.double() * (ap if ablation else ap / (an + float(torch.tensor(1e-7)))))
    outs = torch.stack([loss.sum(), ap.sum(), an.sum()])
    (outs * gin.double()).sum().backward()
    sd, invd, wd = sums.cuda(), inv.cuda(), w.cuda()
    d = torch.full((k + 1, 2), NAN, device="cuda")
    out = torch.full((4,), NAN, device="cuda")
    _lib.call("dhz_contrast_combine_fwd", sd.data_ptr(), invd.data_ptr(), wd.data_ptr(), k, int(ablation), d.data_ptr(), out.data_ptr(), _s())
    gd = gin.cuda()
    gg = torch.full((k + 1, 2), NAN, device="cuda")
    _lib.call("dhz_contrast_combine_bwd", d.data_ptr(), wd.data_ptr(), k, int(ablation), gd.data_ptr(), gd.data_ptr() + 4, gd.data_ptr() + 8,
              gg.data_ptr(), _s())
    torch.cuda.synchronize()
    assert torch.isnan(d[k]).all() and torch.isnan(out[3]) and torch.isnan(gg[k]).all()
    rtol = 32 * 2.0 ** -24
    for what, got, ref in (("means", d[:k], d64.detach()), ("loss, all_ap, all_an", out[:3], outs.detach()), ("coefficients", gg[:k], d64.grad)):
        rel = ((got.cpu().double() - ref).abs() / ref.abs()).max().item()
        print(f"contrast_combine ablation={ablation} {what}: worst relative error {rel:.3e} (bound {rtol:.2e})")
        assert rel <= rtol, (what, rel)
    # no incoming gradient for an output: its pointer is NULL
    _lib.call("dhz_contrast_combine_bwd", d.data_ptr(), wd.data_ptr(), k, int(ablation), None, gd.data_ptr() + 4, None, gg.data_ptr(), _s())
    torch.cuda.synchronize()
    assert torch.equal(gg[:k].cpu(), torch.tensor([[0.3, 0.0]]).expand(k, 2))


@pytest.mark.parametrize("B,H,W,C", [(2, 24, 40, 64), (1, 16, 16, 128)])
def test_thin_conv3x3_fp32_names(B, H, W, C):
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, H * W, C, generator=g)
    w = torch.randn(3, C, 3, 3, generator=g) * 0.05
    b = torch.randn(3, generator=g)
    gy = torch.randn(B, 3, H, W, generator=g)
    x64 = x.double().requires_grad_()
    ref = F.conv2d(x64.view(B, H, W, C).permute(0, 3, 1, 2), w.double(), b.double(), padding=1)
    ref.backward(gy.double())
    xd, wd, bd, gyd = x.cuda(), w.cuda(), b.cuda(), gy.cuda()
    y = torch.full((B * 3 * H * W + 64,), NAN, device="cuda")
    dx = torch.full((B * H * W * C + 64,), NAN, device="cuda")
    _lib.call("dhz_thin_conv3x3_fwd", xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W, C, _s())
    _lib.call("dhz_thin_conv3x3_dgrad", gyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, W, C, _s())
    torch.cuda.synchronize()
    assert torch.isnan(y[-64:]).all() and torch.isnan(dx[-64:]).all()
    y, dx = y[:-64].view(B, 3, H, W).cpu(), dx[:-64].view(B, H * W, C).cpu()
    want_dx = x64.grad.float()
    print(f"thin_conv3x3 fp32 names {(B, H, W, C)}: forward error {(y - ref.float()).abs().max().item():.3e}, "
          f"backward-data error {(dx - want_dx).abs().max().item():.3e} (atol 2e-5, rtol 1e-4)")
    assert torch.allclose(y, ref.detach().float(), atol=2e-5, rtol=1e-4)
    assert torch.allclose(dx, want_dx, atol=2e-5, rtol=1e-4)


def test_split3_planes_of_transposes():
    """dhz_split3_planes_t (the optimizer's planes of every W^T for the backward-data GEMMs): four matrices inside one buffer, gaps
    between them; the planes at each matrix's offset are the planes dhz_split3_planes gives for the transposed matrix, bit for bit
    (the same truncation pieces, so hi + mid + lo == W^T exactly), and the gaps keep their canaries.  85 tiles of 32 x 32: on grids
    sized for 8 compute units (64 workgroups) the tile loop takes a second, ragged trip."""
    from _grid import reserved_grid
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(14)
    shapes = [(64, 32), (32, 96), (256, 256), (128, 128)]
    gap = 40
    offs, off = [], 8
    for R, C in shapes:
        offs.append(off)
        off += R * C + gap
    total = off
    src = torch.randn(total, generator=g)
    src[offs[0]] = 0.0
    src[offs[0] + 1] = -0.0
    desc, t0 = [], 0
    for (R, C), o in zip(shapes, offs):
        desc.append([o, R, C, t0])
        t0 += (R // 32) * (C // 32)
    ntiles = t0
    assert ntiles == 85
    srcd = src.cuda()
    descd = torch.tensor(desc, dtype=torch.int32).cuda()
    want = []
    for (R, C), o in zip(shapes, offs):
        wt = srcd[o:o + R * C].view(R, C).t().contiguous()
        pl = torch.empty((3, R * C), dtype=torch.bfloat16, device="cuda")
        _lib.call("dhz_split3_planes", wt.data_ptr(), R * C, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _s())
        assert torch.equal(pl.double().sum(0), wt.reshape(-1).double())
        want.append(pl)
    for ncu in (None, 8):
        planes = torch.full((3, total), NAN, device="cuda").to(torch.bfloat16)
        with reserved_grid(ncu) as cus:
            assert ncu is None or ntiles > 8 * cus and ntiles % (8 * cus) != 0
            _lib.call("dhz_split3_planes_t", srcd.data_ptr(), planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
                      descd.data_ptr(), len(shapes), ntiles, _s())
            torch.cuda.synchronize()
        live = torch.zeros(total, dtype=torch.bool, device="cuda")
        for (R, C), o, pl in zip(shapes, offs, want):
            assert torch.equal(planes[:, o:o + R * C].view(torch.int16), pl.view(torch.int16)), (ncu, R, C)
            live[o:o + R * C] = True
        assert torch.isnan(planes[:, ~live]).all(), "written outside the matrices"
