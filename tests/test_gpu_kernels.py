"""-m gpu parity tests: every HIP kernel, called through the C-ABI (ctypes -> libdehaze_hip.so), against
the CPU oracle on the same seeded inputs and against the golden vectors captured from the reference.

Tolerances (fp32, stated per test): the HIP kernels accumulate in a different order than ATen's CPU
kernels (MFMA k-ordered fmaf chains, wave reductions), so agreement is to a few ulp of the largest
term: atol 2e-5 / rtol 1e-4 on activations, 1e-4 / 1e-3 on parameter gradients that sum over tokens.
"""
import numpy as np
import pytest
import torch

from oracle import uformer_oracle as O

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from dehaze_hip import ops as _ops
    return _ops


def rank_to_sets(rank):
    r = rank.cpu().numpy()
    return [[sorted(np.nonzero(r[b, h] < 25)[0].tolist()) for h in range(r.shape[1])] for b in range(r.shape[0])]


# ----------------------------------------------------------------------------- K3 vs golden (reference outputs)
@pytest.mark.parametrize("case", ["h1_nomask_bias", "h2_mask_bias", "h16_nomask_nobias", "h2_mask_nobias",
                                  "h2_mask_bias_d64", "h2_mask_bias_d16"])
def test_ps_attention_golden(golden, dev, ops, case):
    g = golden("probattn_" + case)
    q, k, v = T(g["q"]), T(g["k"]), T(g["v"])                       # [B_,64,H,d]
    B_, N, H, d = q.shape
    C = H * d
    qkv = torch.cat([q.reshape(B_ * N, C), k.reshape(B_ * N, C), v.reshape(B_ * N, C)], 1).to(dev).requires_grad_()
    use_bias = bool(g["use_bias"])
    mask = T(g["mask"]).to(dev) if g["mask"].size else None
    idx = T(g["idx"].astype(np.uint8)).to(dev)
    # the kernel takes the [225,H] table; goldens carry an arbitrary [H,64,64] bias => call the C-ABI
    # directly with that bias (also exercises the raw entry points)
    from dehaze_hip import _lib
    bias = T(g["bias"]).to(dev).contiguous() if use_bias else None
    out = torch.empty(B_ * N, C, device=dev)
    rank = torch.empty(B_, H, N, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    base = qkv.data_ptr()
    nW = mask.shape[0] if mask is not None else 1
    _lib.call("dhz_ps_attn_fwd", base, base + 4 * C, base + 8 * C, 3 * C, p(idx), p(bias), p(mask), p(out), C, p(rank),
              B_, H, nW, d, s)
    ref_top = np.sort(g["top"].astype(np.int64), -1)               # [B_,H,25]
    got = rank_to_sets(rank)
    for b in range(B_):
        for h in range(H):
            assert got[b][h] == ref_top[b, h].tolist(), (b, h)
    ref_ctx = T(g["ctx"]).reshape(B_ * N, C).to(dev)
    assert torch.allclose(out, ref_ctx, atol=2e-5, rtol=1e-4), (out - ref_ctx).abs().max()
    # backward
    gout = T(g["gout"]).reshape(B_ * N, C).to(dev).contiguous()
    dqkv = torch.empty_like(qkv)
    parts = _lib.load().dhz_ps_attn_bwd_parts_d(B_, H, d)
    dpart = torch.empty(parts, 64, 64, device=dev) if use_bias else None
    gb = dqkv.data_ptr()
    _lib.call("dhz_ps_attn_bwd", base, base + 4 * C, base + 8 * C, 3 * C, p(bias), p(mask), p(rank), p(gout), C,
              gb, gb + 4 * C, gb + 8 * C, 3 * C, p(dpart), B_, H, nW, d, s)
    torch.cuda.synchronize()
    for i, name in enumerate(("dq", "dk", "dv")):
        ref = T(g[name]).reshape(B_ * N, C).to(dev)
        got_g = dqkv[:, i * C:(i + 1) * C]
        assert torch.allclose(got_g, ref, atol=5e-5, rtol=1e-3), (name, (got_g - ref).abs().max())
    if use_bias:
        dbias = dpart.view(parts // H, H, 64, 64).sum(0)
        assert torch.allclose(dbias, T(g["dbias"]).to(dev), atol=1e-4, rtol=1e-3)


# ----------------------------------------------------------------------------- K3 vs oracle, larger random case
@pytest.mark.parametrize("B_,H,d,use_mask", [(64, 1, 32, True), (32, 4, 32, False), (8, 16, 32, True), (16, 2, 64, True),
                                             (16, 1, 16, True), (8, 16, 16, False)])
def test_ps_attention_oracle(dev, ops, B_, H, d, use_mask):
    g = torch.Generator().manual_seed(B_ * 131 + H)
    C = H * d
    qkv_c = torch.randn(B_ * 64, 3 * C, generator=g)
    table_c = 0.3 * torch.randn(225, H, generator=g)
    gout_c = torch.randn(B_ * 64, C, generator=g)
    idx = torch.randint(64, (64, 25), generator=g)
    mask_c = O.shift_attn_mask(16, 16, 8, 4) if use_mask else None           # nW = 4
    # oracle
    qkv_o = qkv_c.clone().requires_grad_()
    table_o = table_c.clone().requires_grad_()
    q, k, v = (qkv_o[:, i * C:(i + 1) * C].view(B_, 64, H, d).transpose(1, 2) for i in range(3))
    ridx = O.relative_position_index(8).reshape(-1)
    bias_o = table_o[ridx].reshape(64, 64, H).permute(2, 0, 1)
    ctx_o, top_o, Mq, _, _ = O.prob_attention(q, k, v, idx, bias_o, mask_c, return_aux=True)
    out_o = ctx_o.transpose(1, 2).reshape(B_ * 64, C)
    (out_o * gout_c).sum().backward()
    # HIP
    qkv_d = qkv_c.to(dev).requires_grad_()
    table_d = table_c.to(dev).requires_grad_()
    mask_d = mask_c.to(dev) if use_mask else None
    out_d = ops.ps_window_attention(qkv_d, table_d, idx.to(torch.uint8).to(dev), mask_d, H, d)
    (out_d * gout_c.to(dev)).sum().backward()
    _, rank = ops.ps_window_attention_rank(qkv_d.detach(), table_d.detach(), idx.to(torch.uint8).to(dev), mask_d, H, d)
    # selections must agree except where the 25th/26th sparsity measures are numerically tied
    sets = rank_to_sets(rank)
    bad = 0
    for b in range(B_):
        for h in range(H):
            if sets[b][h] != sorted(top_o[b, h].tolist()):
                m = Mq[b, h].sort(descending=True)[0]
                assert (m[24] - m[25]).abs() < 1e-5 * m.abs().max(), "selection differs without a near-tie"
                bad += 1
    assert bad <= max(1, B_ * H // 200)
    if bad == 0:
        assert torch.allclose(out_d.cpu(), out_o, atol=2e-5, rtol=1e-4)
        assert torch.allclose(qkv_d.grad.cpu(), qkv_o.grad, atol=1e-4, rtol=1e-3)
        assert torch.allclose(table_d.grad.cpu(), table_o.grad, atol=2e-4 * B_ ** 0.5, rtol=2e-3)
    # whatever `bad` is: outputs and gradients against float64 under the KERNEL's selection (tests/_autograd_ref.py), same tolerances
    import _autograd_ref as R
    top_d = (rank.cpu() < 25).to(torch.int8).sort(dim=-1, descending=True, stable=True)[1][..., :25]
    qkv_r = qkv_c.double().requires_grad_()
    table_r = table_c.double().requires_grad_()
    q, k, v = (qkv_r[:, i * C:(i + 1) * C].view(B_, 64, H, d).transpose(1, 2) for i in range(3))
    bias_r = table_r[ridx].reshape(64, 64, H).permute(2, 0, 1)
    ctx_r = R.Reference(tops=[top_d])._prob_attention(q, k, v, idx, bias_r, mask_c.double() if use_mask else None)
    out_r = ctx_r.transpose(1, 2).reshape(B_ * 64, C)
    (out_r * gout_c.double()).sum().backward()
    assert torch.allclose(out_d.detach().cpu().double(), out_r.detach(), atol=2e-5, rtol=1e-4)
    assert torch.allclose(qkv_d.grad.cpu().double(), qkv_r.grad, atol=1e-4, rtol=1e-3)
    assert torch.allclose(table_d.grad.cpu().double(), table_r.grad, atol=2e-4 * B_ ** 0.5, rtol=2e-3)


def test_bias_gather_and_shift_mask(dev, ops):
    from dehaze_hip import _lib
    table = torch.randn(225, 4)
    bias = torch.empty(4, 64, 64, device=dev)
    _lib.call("dhz_bias_gather", table.to(dev).data_ptr(), bias.data_ptr(), 4, torch.cuda.current_stream().cuda_stream)
    ref = table[O.relative_position_index(8).reshape(-1)].reshape(64, 64, 4).permute(2, 0, 1)
    assert torch.equal(bias.cpu(), ref)                                         # pure gather: bit exact
    for res in (16, 32, 128):
        assert torch.equal(ops.shift_mask(res, res, 4, dev).cpu(), O.shift_attn_mask(res, res, 8, 4))


# ----------------------------------------------------------------------------- K1 / K4
@pytest.mark.parametrize("C,res,shift", [(32, 16, 0), (32, 16, 4), (64, 32, 4), (128, 16, 4), (256, 16, 0), (512, 8, 0)])
def test_ln_partition(dev, ops, C, res, shift):
    g = torch.Generator().manual_seed(C + res + shift)
    B = 2
    x = torch.randn(B, res * res, C, generator=g) * 2 + 0.5
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    go = torch.randn(B * res * res, C, generator=g)
    xo, go_, bo = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = torch.nn.functional.layer_norm(xo, (C,), go_, bo, 1e-5).view(B, res, res, C)
    if shift:
        y = torch.roll(y, (-shift, -shift), (1, 2))
    yo = O.window_partition(y, 8).reshape(-1, C)
    (yo * go).sum().backward()
    xd, gd, bd = x.to(dev).requires_grad_(), gamma.to(dev).requires_grad_(), beta.to(dev).requires_grad_()
    yd = ops.ln_partition(xd, gd, bd, res, res, shift)
    (yd * go.to(dev)).sum().backward()
    assert torch.allclose(yd.cpu(), yo, atol=1e-5, rtol=1e-5)
    assert torch.allclose(xd.grad.cpu(), xo.grad, atol=2e-5, rtol=1e-4)
    assert torch.allclose(gd.grad.cpu(), go_.grad, atol=2e-4, rtol=1e-3)
    assert torch.allclose(bd.grad.cpu(), bo.grad, atol=2e-4, rtol=1e-3)
    # plain LN (norm2)
    y2 = ops.layer_norm_tokens(x.to(dev), gamma.to(dev), beta.to(dev))
    assert torch.allclose(y2.cpu(), torch.nn.functional.layer_norm(x, (C,), gamma, beta, 1e-5).view(-1, C), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("C,res,shift", [(32, 16, 4), (64, 16, 0), (512, 16, 4)])
def test_reverse_residual(dev, ops, C, res, shift):
    g = torch.Generator().manual_seed(C + shift)
    B = 3
    yw = torch.randn(B * res * res, C, generator=g)
    sc = torch.randn(B, res * res, C, generator=g)
    scale = torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.9])
    go = torch.randn(B, res * res, C, generator=g)
    ywo, sco = yw.clone().requires_grad_(), sc.clone().requires_grad_()
    y = O.window_reverse(ywo.view(-1, 64, C), 8, res, res)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    out_o = sco + y.reshape(B, -1, C) * scale.view(B, 1, 1)
    (out_o * go).sum().backward()
    ywd, scd = yw.to(dev).requires_grad_(), sc.to(dev).requires_grad_()
    out_d = ops.reverse_residual(ywd, scd, scale.to(dev), res, res, shift)
    (out_d * go.to(dev)).sum().backward()
    assert torch.allclose(out_d.cpu(), out_o, atol=1e-6, rtol=1e-6)
    assert torch.allclose(ywd.grad.cpu(), ywo.grad, atol=1e-6, rtol=1e-6)
    assert torch.allclose(scd.grad.cpu(), sco.grad)
    out2 = ops.residual_scale(yw.to(dev), sc.to(dev), None)
    assert torch.allclose(out2.cpu(), sc + yw.view(B, -1, C), atol=1e-6)


# ----------------------------------------------------------------------------- K5
@pytest.mark.parametrize("Ch,res", [(128, 16), (128, 8), (256, 32), (2048, 8), (64, 24), (96, 16)])      # 96: the 8-lane forward
def test_leff_dwconv(dev, ops, Ch, res):
    g = torch.Generator().manual_seed(Ch + res)
    B = 2
    u = torch.randn(B, res * res, Ch, generator=g)
    w = 0.3 * torch.randn(Ch, 1, 3, 3, generator=g)
    b = 0.1 * torch.randn(Ch, generator=g)
    go = torch.randn(B, res * res, Ch, generator=g)
    F = torch.nn.functional
    uo, wo, bo = u.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    m = F.gelu(uo).transpose(1, 2).reshape(B, Ch, res, res)
    zo = F.gelu(F.conv2d(m, wo, bo, padding=1, groups=Ch)).flatten(2).transpose(1, 2)
    (zo * go).sum().backward()
    ud, wd, bd = u.to(dev).requires_grad_(), w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    zd = ops.leff_dwconv(ud, wd, bd, res, res)
    (zd * go.to(dev)).sum().backward()
    assert torch.allclose(zd.cpu(), zo, atol=1e-5, rtol=1e-5)
    assert torch.allclose(ud.grad.cpu(), uo.grad, atol=2e-5, rtol=1e-4)
    assert torch.allclose(wd.grad.cpu(), wo.grad, atol=3e-4, rtol=1e-3)
    assert torch.allclose(bd.grad.cpu(), bo.grad, atol=3e-4, rtol=1e-3)


def test_leff_dwconv_bwd_scaled_c_abi(dev):
    """dhz_leff_dwconv_bwd_scaled_dt: a per-image factor on dz (the DropPath scale folded into the kernel) == the plain kernel on a
    pre-scaled dz (bit-identical up to the order of two multiplications: compared with a tolerance of a few ulp)."""
    from dehaze_hip import _lib
    s = torch.cuda.current_stream().cuda_stream
    B, res, Ch = 4, 16, 64
    g = torch.Generator().manual_seed(3)
    u, dz, tp = (torch.randn(B * res * res, Ch, generator=g).to(dev) for _ in range(3))
    w = (0.3 * torch.randn(Ch, 9, generator=g)).to(dev)
    sc = torch.tensor([0.0, 1.25, 1.0, 1.111], device=dev)
    out = []
    for scaled in (True, False):
        du = torch.empty_like(u); dw = torch.zeros(Ch * 9, device=dev); db = torch.zeros(Ch, device=dev)
        dzz = dz if scaled else (dz.view(B, -1, Ch) * sc.view(B, 1, 1)).reshape(-1, Ch).contiguous()
        _lib.call("dhz_leff_dwconv_bwd_scaled_dt", dzz.data_ptr(), u.data_ptr(), tp.data_ptr(), w.data_ptr(), du.data_ptr(),
                  dw.data_ptr(), db.data_ptr(), sc.data_ptr() if scaled else None, B, res, res, Ch, 0, s)
        out.append((du, dw, db))
    for a, b in zip(*out):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
    assert out[0][0].view(B, -1)[0].abs().max().item() == 0.0          # the dropped image passes no gradient


# ----------------------------------------------------------------------------- K10 / K12
def test_charbonnier(golden, dev, ops):
    g = golden("losses")
    x = T(g["char_x"]).to(dev).requires_grad_()
    l = ops.charbonnier(x, T(g["char_y"]).to(dev))
    assert abs(l.item() - float(g["char_loss"])) < 1e-6
    l.backward()
    assert torch.allclose(x.grad.cpu(), T(g["char_dx"]), atol=1e-8, rtol=1e-5)
    # clamped variant with a second consumer of the clamp (TR:230-238)
    gen = torch.Generator().manual_seed(1)
    xx = torch.rand(2, 3, 32, 32, generator=gen) * 1.4 - 0.2
    yy = torch.rand(2, 3, 32, 32, generator=gen)
    extra = torch.randn(2, 3, 32, 32, generator=gen)
    xo = xx.clone().requires_grad_()
    co = torch.clamp(xo, 0, 1)
    (O.charbonnier(co, yy) * 0.7 + (co * extra).sum()).backward()
    xd = xx.to(dev).requires_grad_()
    ld, cd = ops.charbonnier_clamped(xd, yy.to(dev))
    (ld * 0.7 + (cd * extra.to(dev)).sum()).backward()
    assert torch.allclose(cd.cpu(), co)
    assert abs(ld.item() - O.charbonnier(co, yy).item()) < 1e-6
    assert torch.allclose(xd.grad.cpu(), xo.grad, atol=1e-7, rtol=1e-5)


def test_adamw(dev, ops):
    gen = torch.Generator().manual_seed(2)
    n = 10007
    p0 = torch.randn(n, generator=gen)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    pd = p0.to(dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    for step in range(1, 6):
        gr = torch.randn(n, generator=gen)
        pr.grad = gr.clone()
        opt.step()
        ops.adamw_step_(pd, gr.to(dev), m, v, 2e-4, 0.9, 0.999, 1e-8, 0.02, step)
    assert torch.allclose(pd.cpu(), pr.detach(), atol=1e-7, rtol=1e-6)
    assert torch.allclose(m.cpu(), opt.state[pr]["exp_avg"], atol=1e-7, rtol=1e-5)   # torch uses lerp for m


# the last two: more 8 x 16 tiles (640, 1152) than persistent workgroups (2 per CU), so workgroups walk several tiles with the
# next one prefetched; C = 128 = two channel chunks per tile
@pytest.mark.parametrize("B,H,W,C", [(2, 24, 40, 64), (1, 16, 16, 128), (3, 9, 21, 64), (5, 128, 128, 64), (9, 128, 128, 128), (7, 100, 90, 64)])
def test_thin_conv3x3_vs_torch(B, H, W, C):
    """Output projection kernels (C -> 3, 3x3, pad 1; ragged tiles included) vs conv2d in float64: forward, backward-data and
    the in-place weight / bias gradients."""
    from dehaze_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, H * W, C, generator=g)
    w = torch.randn(3, C, 3, 3, generator=g) * 0.05
    b = torch.randn(3, generator=g)
    gy = torch.randn(B, 3, H, W, generator=g)
    x64 = x.double().requires_grad_(); w64 = w.double().requires_grad_(); b64 = b.double().requires_grad_()
    ref = torch.nn.functional.conv2d(x64.view(B, H, W, C).permute(0, 3, 1, 2), w64, b64, padding=1)
    ref.backward(gy.double())
    xd = x.to(dev).requires_grad_()
    wd = torch.nn.Parameter(w.to(dev)); bd = torch.nn.Parameter(b.to(dev))
    y = ops.thin_conv3x3(xd, wd, bd, H, W)
    assert y.shape == (B, 3, H, W)
    assert torch.allclose(y.cpu(), ref.float(), atol=2e-5, rtol=1e-4), (y.cpu() - ref.float()).abs().max()
    y.backward(gy.to(dev))
    assert torch.allclose(xd.grad.cpu(), x64.grad.float().reshape(B, H * W, C), atol=2e-5, rtol=1e-4)
    scale = max(1.0, (B * H * W / 1000.0) ** 0.5)            # sums over B H W terms of O(1): fp32 accumulation error grows with sqrt
    assert torch.allclose(wd.grad.cpu(), w64.grad.float(), atol=2e-4 * scale, rtol=1e-4), (wd.grad.cpu() - w64.grad.float()).abs().max()
    assert torch.allclose(bd.grad.cpu(), b64.grad.float(), atol=2e-4 * scale, rtol=1e-4)
