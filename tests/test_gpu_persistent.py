"""-m gpu: the persistent kernels in their multi-trip regime, against float64 references.

Most hot kernels run a persistent grid ("resident workgroups per CU x dhz_num_cus()") and walk windows, window-heads or tiles with a
grid-stride loop; between trips they carry prefetched operands, register-resident weights, gradient accumulators and LDS.  Every case
here runs at three grid levels (tests/_grid.py: the whole device, grids sized for 8 CUs and for 9 CUs), asserts that each kernel makes
at least three trips with a ragged last one, and checks

  (a) grid invariance: outputs that no cross-workgroup reduction touches (activations, dx, dqkv, ranks, saved tensors) are bit-equal
      to the whole-device result - the per-item arithmetic does not depend on the grid;
  (b) reduced outputs (weight / bias / LayerNorm / bias-table gradients: atomics and per-workgroup partial sums) agree with the
      whole-device result within an fp32 reordering bound, elementwise: |err| <= RED * mag + floor, mag = the same sum over |terms|;
  (c) every output agrees with a float64 reference of the same operation (plain torch in float64 on the same inputs; bf16 cases
      on bf16-representable inputs).

RED = 2^-18 (64 units of fp32 round-off of the summed magnitudes): the partial sums of a reduction over up to ~400k tokens are
combined in an order that depends on the grid; the wgrad tests of the suite hold 2^-21 over 65k tokens on one grid.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from _grid import LEVELS, MAX_WG_PER_CU, assert_trips, physical_cus, reserved_grid
from oracle import uformer_oracle as O

pytestmark = pytest.mark.gpu
RED = 2.0 ** -18
BOUND6 = 2.0 ** -21          # six-term split GEMMs against float64, relative to sum |a||b| (tests/test_gpu_split.py)
EPS = 2.0 ** -8              # bf16 unit round-off
BF = torch.bfloat16
DEV = torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _check_red(name, got, ref, mag, floor):
    err = (got.double() - ref.double()).abs()
    bad = err > RED * mag + floor
    assert not bad.any(), (name, int(bad.sum()), (err / (mag + floor / RED)).max().item())


def _check_selection(name, rank, Mq):
    """rank [B_,H,64] (< 25 = selected) is a top-25 of the float64 sparsity measure Mq [B_,H,64], up to near-ties"""
    sel = rank < 25
    assert (sel.sum(-1) == 25).all(), name
    lo = Mq.masked_fill(~sel, math.inf).min(-1)[0]
    hi = Mq.masked_fill(sel, -math.inf).max(-1)[0]
    tol = 1e-5 * Mq.abs().amax(-1)
    assert (lo >= hi - tol).all(), (name, "selection differs from the float64 top-25 without a near-tie")


def _prob_attention_given(q, k, v, idx, top, bias, mask):
    """O.prob_attention with the selection `top` [B_,H,25] given (the HIP kernel's own), on any device / dtype.  Returns ctx, the
    float64 sparsity measure and the per-window gathered bias rows (for the magnitude of the table gradient)."""
    B_, H, N, d = q.shape
    ks = k[:, :, idx, :]
    S = torch.matmul(q.unsqueeze(-2), ks.transpose(-2, -1)).squeeze(-2)
    Mq = (S.max(-1)[0] - S.sum(-1) / N).detach()
    bi = torch.arange(B_, device=q.device)[:, None, None]
    hi = torch.arange(H, device=q.device)[None, :, None]
    scores = torch.matmul(q[bi, hi, top], k.transpose(-2, -1)) * (1.0 / math.sqrt(d))
    ctx = v.mean(dim=-2, keepdim=True).expand(B_, H, N, d).clone()
    a = torch.softmax(scores, dim=-1)
    bsel = None
    if bias is not None:
        bsel = bias[hi, top]
        bsel.retain_grad()
        a = a + bsel
    if mask is not None:
        wi = (torch.arange(B_, device=q.device) % mask.shape[0])[:, None, None]
        a = a + mask[wi, top]
    a = torch.softmax(a, dim=-1)
    ctx[bi, hi, top] = torch.matmul(a, v)
    return ctx, Mq, bsel


def _table_mag(bsel, top, H):
    """sum of |d(bias rows)| per table entry: the magnitude of the table gradient's terms"""
    ridx = O.relative_position_index(8).to(top.device)
    e = ridx[top] * H + torch.arange(H, device=top.device)[None, :, None, None]
    return torch.zeros(225 * H, dtype=torch.float64, device=top.device).index_add_(0, e.flatten(), bsel.grad.abs().flatten().double()).view(225, H)


def _top(rank):
    """[B_,H,64] ranks -> [B_,H,25] selected query rows"""
    return (rank < 25).to(torch.int8).sort(dim=-1, descending=True, stable=True)[1][..., :25]


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. fused window attention, C = 32 (persistent forward, register-resident weights; fused backward)
def _attn_inputs(B, Hres, Wres, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    C = 32
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    P = dict(gamma=1 + 0.1 * r(C), beta=0.1 * r(C), wq=r(C, C) / C ** 0.5, bq=0.1 * r(C), wk=r(C, C) / C ** 0.5, bk=0.1 * r(C),
             wv=r(C, C) / C ** 0.5, bv=0.1 * r(C), wo=r(C, C) / C ** 0.5, bo=0.1 * r(C), table=0.3 * r(225, 1))
    x = r(B, Hres * Wres, C)
    dout = r(B, Hres * Wres, C)
    dscale = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(B)], device=DEV)      # DropPath: dropped images included
    idx = torch.randint(64, (64, 25), generator=g, device=DEV)
    return x, dout, dscale, idx, P


PNAMES = ("gamma", "beta", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "table")


def _attn_hip(x, dout, dscale, idx, P, Hres, Wres, shift, mode):
    """one forward without gradients and one with (saves: 'rank' = the fused backward's, 'all' = the kernel chain's five), then the
    backward the record asks for; parameter gradients land in .grad"""
    from dehaze_hip import fused, ops
    mask = ops.shift_mask(Hres, Wres, shift, DEV) if shift else None
    idx8 = idx.to(torch.uint8)
    prm = {n: t.clone().requires_grad_() for n, t in P.items()}
    args = lambda: (x, prm["gamma"], prm["beta"], prm["wq"], prm["bq"], prm["wk"], prm["bk"], prm["wv"], prm["bv"], prm["wo"],
                    prm["bo"], prm["table"], idx8, mask, dscale, Hres, Wres, shift, 1)
    with torch.no_grad():
        out_inf, rec = fused._attn_fused_fwd(False, *args())
        assert rec is None
    keep = fused.ATTN_FUSED_BWD_C
    fused.ATTN_FUSED_BWD_C = (32,) if mode == "rank" else ()
    try:
        with torch.no_grad():
            out, rec = fused._attn_fused_fwd(True, *args())
    finally:
        fused.ATTN_FUSED_BWD_C = keep
    assert rec.kind == ("attn_fused_bwd" if mode == "rank" else "attn_chain_bwd")
    saves = {}
    if mode == "all":
        _, _, stats, xn, qkv, cx, rank = rec.saved[:7]
        saves = dict(stats=stats, xn=xn, qkv=qkv, cx=cx)
    else:
        rank = rec.saved[3]
    saves["rank"] = rank
    saves = {k_: v_.clone() for k_, v_ in saves.items()}
    with torch.no_grad():
        ret = fused._attn_bwd(rec, dout)
    for n, gr in zip(PNAMES, ret[1:]):
        if gr is not None:
            prm[n].grad = gr if prm[n].grad is None else prm[n].grad + gr
    torch.cuda.synchronize()
    grads = {n: prm[n].grad.clone() for n in PNAMES}
    return out_inf, out, ret[0], saves, grads


def _attn_ref(x, dout, dscale, idx, P, Hres, Wres, shift, top):
    """float64 attention branch (O.lewin_block's first half, M1:838-872) with the given selection; returns the output, dx, parameter
    gradients, their term magnitudes and the float64 sparsity measure"""
    B, L, C = x.shape
    x = x.double().requires_grad_()
    prm = {n: t.double().requires_grad_() for n, t in P.items()}
    xn = F.layer_norm(x, (C,), prm["gamma"], prm["beta"], 1e-5)
    xn.retain_grad()
    y = xn.view(B, Hres, Wres, C)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    xw = O.window_partition(y, 8)
    B_ = xw.shape[0]
    lin = {}
    for n in "qkv":
        lin[n] = F.linear(xw, prm["w" + n], prm["b" + n])
        lin[n].retain_grad()
    q, k, v = (lin[n].view(B_, 64, 1, C).transpose(1, 2) for n in "qkv")
    bias = prm["table"][O.relative_position_index(8).to(DEV).reshape(-1)].reshape(64, 64, 1).permute(2, 0, 1)
    mask = O.shift_attn_mask(Hres, Wres, 8, shift, torch.float64).to(DEV) if shift else None
    ctx, Mq, bsel = _prob_attention_given(q, k, v, idx, top, bias, mask)
    ctx = ctx.transpose(1, 2).reshape(B_, 64, C)
    aw = F.linear(ctx, prm["wo"], prm["bo"])
    aw.retain_grad()
    y = O.window_reverse(aw, 8, Hres, Wres)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    out = x + dscale.double()[:, None, None] * y.reshape(B, L, C)
    out.backward(dout.double())
    tok = lambda t: t.detach().reshape(-1, t.shape[-1]).abs()
    mean = x.detach().mean(-1, keepdim=True)
    xhat = (x.detach() - mean) / torch.sqrt(x.detach().var(-1, unbiased=False, keepdim=True) + 1e-5)
    mag = dict(gamma=(tok(xn.grad) * tok(xhat)).sum(0), beta=tok(xn.grad).sum(0), table=_table_mag(bsel, top, 1),
               wo=tok(aw.grad).t() @ tok(ctx), bo=tok(aw.grad).sum(0))
    for n in "qkv":
        mag["w" + n] = tok(lin[n].grad).t() @ tok(xw)
        mag["b" + n] = tok(lin[n].grad).sum(0)
    return out.detach(), x.grad, {n: prm[n].grad for n in PNAMES}, mag, Mq


@pytest.mark.parametrize("mode", ["rank", "all"])
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("p6", [False, True])
def test_fused_attention_c32_multi_trip(mode, shift, p6):
    """forward (inference, then the training saves of `mode`) and backward of the C = 32 attention branch on a non-square map
    (40 x 56: 35 windows per image, so the prefetched next window crosses image boundaries), DropPath factors with zeros"""
    from dehaze_hip import _lib, fused
    lib = _lib.load()
    Hres, Wres = 40, 56
    full = physical_cus()
    per_img = (Hres // 8) * (Wres // 8)
    B = -(-3 * MAX_WG_PER_CU * full // per_img) + 1
    nwin = B * per_img
    x, dout, dscale, idx, P = _attn_inputs(B, Hres, Wres, 100 + shift)
    keep = fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C
    fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C = p6, ((32, 64, 128) if p6 else keep[1])
    res = {}
    try:
        for lvl in LEVELS:
            with reserved_grid(lvl) as ncu:
                assert_trips("fused forward", nwin, MAX_WG_PER_CU * ncu, unit=ncu)
                if mode == "rank":
                    assert_trips("fused backward", nwin, lib.dhz_fused_attn_bwd_parts(nwin))
                else:
                    parts = lib.dhz_ps_attn_bwd_parts_d(nwin, 1, 32)
                    assert_trips("ps_attn forward", nwin, 3 * ncu)
                    assert_trips("ps_attn backward", nwin, parts)
                res[lvl] = _attn_hip(x, dout, dscale, idx, P, Hres, Wres, shift, mode)
    finally:
        fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C = keep
    out_inf0, out0, dx0, saves0, g0 = res[None]
    for lvl in LEVELS[1:]:                                                                    # (a), (b)
        out_inf, out, dx, saves, g = res[lvl]
        assert torch.equal(out_inf, out_inf0), lvl
        assert torch.equal(out, out0), lvl
        assert torch.equal(dx, dx0), lvl
        for n in saves0:
            assert torch.equal(saves[n], saves0[n]), (lvl, n)
    rank = saves0["rank"].view(nwin, 1, 64)
    ref_out, ref_dx, ref_g, mag, Mq = _attn_ref(x, dout, dscale, idx, P, Hres, Wres, shift, _top(rank).long())
    _check_selection("fused", rank, Mq)
    for lvl in LEVELS[1:]:
        for n in PNAMES:
            _check_red((lvl, n), res[lvl][4][n], g0[n], mag[n], 1e-6)
    assert torch.allclose(out0.double(), ref_out, atol=2e-5, rtol=1e-4), (out0.double() - ref_out).abs().max()   # (c)
    assert torch.allclose(out_inf0.double(), ref_out, atol=2e-5, rtol=1e-4), (out_inf0.double() - ref_out).abs().max()
    for lvl in LEVELS:
        dx = res[lvl][2].double()
        assert torch.allclose(dx, ref_dx, atol=5e-5, rtol=1e-3), (lvl, (dx - ref_dx).abs().max())
    for n in PNAMES:
        _check_red(("fp64", n), g0[n], ref_g[n], mag[n], 1e-5)


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. ProbSparse window attention (ps_attn fwd / bwd), fp32 and bf16
def _ps_hip(qkv, idx8, bias, mask, gout, B_, H, d, dt):
    from dehaze_hip import _lib
    lib = _lib.load()
    C = H * d
    es = qkv.element_size()
    nW = mask.shape[0] if mask is not None else 1
    out = torch.full((B_ * 64, C), float("nan"), device=DEV, dtype=qkv.dtype)
    rank = torch.empty(B_, H, 64, dtype=torch.uint8, device=DEV)
    b = qkv.data_ptr()
    _lib.call("dhz_ps_attn_fwd_dt", b, b + es * C, b + 2 * es * C, 3 * C, idx8.data_ptr(), _p(bias), _p(mask), out.data_ptr(), C,
              rank.data_ptr(), B_, H, nW, d, dt, _s())
    dqkv = torch.full_like(qkv, float("nan"))
    parts = lib.dhz_ps_attn_bwd_parts_d(B_, H, d)
    dpart = torch.empty(parts, 64, 64, device=DEV) if bias is not None else None
    gb = dqkv.data_ptr()
    _lib.call("dhz_ps_attn_bwd_dt", b, b + es * C, b + 2 * es * C, 3 * C, _p(bias), _p(mask), rank.data_ptr(), gout.data_ptr(), C,
              gb, gb + es * C, gb + 2 * es * C, 3 * C, _p(dpart), B_, H, nW, d, dt, _s())
    dtable = None
    if bias is not None:
        dtable = torch.zeros(225, H, device=DEV)
        _lib.call("dhz_bias_table_grad", dpart.data_ptr(), parts, dtable.data_ptr(), H, 0, _s())
    torch.cuda.synchronize()
    return out, rank, dqkv, dtable


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("H,d,use_mask,use_bias", [(2, 32, True, True), (2, 32, False, False), (2, 64, True, True),
                                                   (2, 16, True, False), (1, 64, False, True), (16, 32, True, True)])
def test_ps_attention_multi_trip(dtype, H, d, use_mask, use_bias):
    from dehaze_hip import _lib
    lib = _lib.load()
    full = physical_cus()
    B_ = 4 * (-(-3 * MAX_WG_PER_CU * full // (4 * H)) + 1)       # a multiple of nW = 4
    if B_ * H % (3 * full) == 0:
        B_ += 4
    C = H * d
    T = B_ * 64
    g = torch.Generator(device=DEV).manual_seed(B_ + 7 * H + d)
    dt = torch.float32 if dtype == "f32" else BF
    qkv = torch.randn(T, 3 * C, generator=g, device=DEV).to(dt)                    # bf16: representable inputs
    gout = torch.randn(T, C, generator=g, device=DEV).to(dt)
    table = 0.3 * torch.randn(225, H, generator=g, device=DEV)
    idx = torch.randint(64, (64, 25), generator=g, device=DEV)
    mask = O.shift_attn_mask(16, 16, 8, 4).to(DEV) if use_mask else None                # nW = 4
    ridx = O.relative_position_index(8).to(DEV).reshape(-1)
    bias = table[ridx].reshape(64, 64, H).permute(2, 0, 1).contiguous() if use_bias else None
    code = 0 if dtype == "f32" else 1
    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            parts = lib.dhz_ps_attn_bwd_parts_d(B_, H, d)
            assert parts % H == 0 and (lvl is None or H < 16 or parts == H)
            assert_trips("ps_attn forward", B_ * H, min(B_ * H, 3 * ncu))
            if parts > H:
                assert_trips("ps_attn backward (windows per head)", B_, parts // H)
            else:                                                  # one workgroup per head walks all of its windows
                assert B_ >= 3
            res[lvl] = _ps_hip(qkv, idx.to(torch.uint8), bias, mask, gout, B_, H, d, code)
    out0, rank0, dq0, dt0 = res[None]
    assert torch.isfinite(out0).all() and torch.isfinite(dq0).all()
    # float64 reference with the kernel's own selection: the values are checked whatever a near-tie did to the selection
    qkv64 = qkv.double().requires_grad_()
    t64 = table.double().requires_grad_()
    q, k, v = (qkv64[:, i * C:(i + 1) * C].view(B_, 64, H, d).transpose(1, 2) for i in range(3))
    b64 = t64[ridx].reshape(64, 64, H).permute(2, 0, 1) if use_bias else None
    ctx, Mq, bsel = _prob_attention_given(q, k, v, idx, _top(rank0).long(), b64, mask.double() if use_mask else None)
    ref = ctx.transpose(1, 2).reshape(T, C)
    ref.backward(gout.double())
    _check_selection("ps_attn", rank0, Mq)
    tmag = _table_mag(bsel, _top(rank0).long(), H) if use_bias else None
    for lvl in LEVELS[1:]:                                                                    # (a), (b)
        out, rank, dq, dtab = res[lvl]
        assert torch.equal(rank, rank0), lvl
        assert torch.equal(out, out0), lvl
        assert torch.equal(dq, dq0), lvl
        if use_bias:
            _check_red((lvl, "dtable"), dtab, dt0, tmag, 1e-6)
    if dtype == "f32":                                                                        # (c)
        assert torch.allclose(out0.double(), ref, atol=2e-5, rtol=1e-4), (out0.double() - ref).abs().max()
        assert torch.allclose(dq0.double(), qkv64.grad, atol=1e-4, rtol=1e-3), (dq0.double() - qkv64.grad).abs().max()
        if use_bias:
            _check_red("dtable vs fp64", dt0, t64.grad, tmag, 1e-5)
    else:
        # outputs rounded to bf16 (relative EPS / 2) after fp32 sums of bf16-rounded probabilities (EPS of sum |a||v| <= EPS max |v|)
        vmax = v.detach().abs().amax(-2, keepdim=True).expand(B_, H, 64, d).transpose(1, 2).reshape(T, C)
        err = (out0.double() - ref.detach()).abs()
        assert (err <= EPS * ref.detach().abs() + 2 * EPS * vmax + 1e-5).all(), (err / (ref.detach().abs() + vmax)).max().item()
        # gradients: within a few bf16 steps of the largest term of their window and head
        gref = qkv64.grad.view(B_, 64, 3, H, d)
        scale = gref.abs().amax(dim=(1, 4), keepdim=True)
        err = (dq0.double().view(B_, 64, 3, H, d) - gref).abs()
        assert (err <= 4 * EPS * scale + 1e-5).all(), (err / (scale + 1e-30)).max().item()
        if use_bias:
            err = (dt0.double() - t64.grad).abs()
            assert (err <= 4 * EPS * tmag + 1e-4).all(), (err / tmag).max().item()


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. token GEMMs with epilogues (persistent tile schedulers, XCD remap when grid % 8 == 0 and ntiles % 8 == 0)
def _gemm_T(N, per_cu, extra):
    """a token count whose tiles (128 / 256 rows x 64 / 128 features) make at least three trips of a per_cu x CUs grid at every level"""
    full = physical_cus()
    tiles = 3 * per_cu * full
    return 256 * -(-tiles // max(1, N // 128)) + extra


def _gemm_trips(what, T, N, per_cu, ncu):
    for bm, bn in ((256, 128), (128, 128), (128, 64)):
        if N % bn == 0:
            assert_trips(f"{what} ({bm} x {bn} tiles)", -(-T // bm) * (N // bn), per_cu * ncu, unit=ncu)


@pytest.mark.parametrize("kind,N,K,extra", [("split6", 256, 128, 96), ("split6", 128, 64, 32), ("split3", 256, 128, 96),
                                            ("split6x", 128, 256, 32), ("fp32", 128, 128, 96), ("bf16", 256, 128, 32),
                                            ("bf16", 128, 64, 160), ("bf16", 192, 128, 32)])
def test_gemm_forward_and_dgrad_multi_trip(kind, N, K, extra):
    """forward (bias) and backward-data of the token GEMMs: split6 planes (its own kernels), the split kernel with 3 / 6 terms, the
    fp32-pipe kernel, the bf16 kernels.  bf16 forwards with N % 128 == 0 and at least as many 256 x 128 tiles as CUs take the pipelined
    kernel (csrc/gemm_bf16_pipe.hip); N = 192 keeps the forward on linear_bf16.hip's own persistent scheduler in the multi-trip regime."""
    from dehaze_hip import _lib, ops
    T = _gemm_T(N, 2, extra)
    g = torch.Generator(device=DEV).manual_seed(T + N + K)
    dt = BF if kind == "bf16" else torch.float32
    x = torch.randn(T, K, generator=g, device=DEV).to(dt)
    w = (torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(dt)
    b = torch.randn(N, generator=g, device=DEV)
    dy = torch.randn(T, N, generator=g, device=DEV).to(dt)
    if kind in ("split6", "split6x"):
        hi, mid, lo = ops.split_planes(w)

    def run():
        y = torch.full((T, N), float("nan"), device=DEV, dtype=dt)
        dx = torch.full((T, K), float("nan"), device=DEV, dtype=dt)
        if kind in ("split6", "split6x"):
            _lib.call("dhz_linear_fwd_split6", x.data_ptr(), K, hi.data_ptr(), mid.data_ptr(), lo.data_ptr(), b.data_ptr(), y.data_ptr(), N,
                      T, N, K, _s())
            _lib.call("dhz_linear_dgrad_split6", dy.data_ptr(), N, hi.data_ptr(), mid.data_ptr(), lo.data_ptr(), dx.data_ptr(), K, T, N, K,
                      _s())
        elif kind == "split3":
            _lib.call("dhz_linear_fwd_split", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, T, N, K, 3, _s())
            _lib.call("dhz_linear_dgrad_split", dy.data_ptr(), N, w.data_ptr(), dx.data_ptr(), K, T, N, K, 3, _s())
        elif kind == "fp32":
            _lib.call("dhz_linear_fwd", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, T, N, K, _s())
            _lib.call("dhz_linear_dgrad", dy.data_ptr(), N, w.data_ptr(), dx.data_ptr(), K, T, N, K, _s())
        else:
            _lib.call("dhz_linear_fwd_bf16", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), y.data_ptr(), N, T, N, K, _s())
            _lib.call("dhz_linear_dgrad_bf16", dy.data_ptr(), N, w.data_ptr(), dx.data_ptr(), K, T, N, K, _s())
        torch.cuda.synchronize()
        return y, dx

    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            _gemm_trips(kind, T, N, 2 if lvl is None else MAX_WG_PER_CU, ncu)
            res[lvl] = run()
    for lvl in LEVELS[1:]:                                                                        # (a)
        assert torch.equal(res[lvl][0], res[None][0]), (lvl, "forward")
        assert torch.equal(res[lvl][1], res[None][1]), (lvl, "dgrad")
    y, dx = res[None]                                                                             # (c)
    ref = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    refd = dy.double() @ w.double()
    magd = dy.double().abs() @ w.double().abs()
    bound = {"split3": 2.0 ** -15, "bf16": EPS, "fp32": 2.0 ** -19}.get(kind, BOUND6)
    for got, r, m in ((y, ref, mag), (dx, refd, magd)):
        err = (got.double() - r).abs()
        assert (err <= bound * m + 1e-6).all(), (kind, (err / m).max().item())


@pytest.mark.parametrize("windowed,shift,scaled", [(1, 4, True), (1, 0, False), (0, 0, True)])
def test_residual_epilogue_multi_trip(windowed, shift, scaled):
    """out = res + factor * window_reverse(roll(x W^T + b)) in the epilogue of the split6 GEMM (dhz_linear_fwd_split6_res) and of the
    split kernel (dhz_linear_fwd_split_res), on a non-square map whose tile count is not a multiple of the grid"""
    from dehaze_hip import _lib, ops
    from test_gpu_epilogue import _window_reverse_roll
    Hm, Wm, K, N = 40, 56, 128, 128
    full = physical_cus()
    B = -(-3 * 2 * full * 256 // (Hm * Wm)) + 1                     # 256-row tiles, two workgroups per CU
    T = B * Hm * Wm
    g = torch.Generator(device=DEV).manual_seed(T + shift)
    x = torch.randn(T, K, generator=g, device=DEV)
    w = torch.randn(N, K, generator=g, device=DEV) / K ** 0.5
    b = torch.randn(N, generator=g, device=DEV)
    resid = torch.randn(T, N, generator=g, device=DEV)
    sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(B)], device=DEV) if scaled else None
    hi, mid, lo = ops.split_planes(w)

    def run():
        o6 = torch.full((T, N), float("nan"), device=DEV)
        o = torch.full((T, N), float("nan"), device=DEV)
        _lib.call("dhz_linear_fwd_split6_res", x.data_ptr(), K, hi.data_ptr(), mid.data_ptr(), lo.data_ptr(), b.data_ptr(), resid.data_ptr(),
                  _p(sc), o6.data_ptr(), N, T, N, K, Hm * Wm, Hm, Wm, shift, windowed, _s())
        _lib.call("dhz_linear_fwd_split_res", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), resid.data_ptr(), _p(sc), o.data_ptr(), N, T, N,
                  K, Hm * Wm, Hm, Wm, shift, windowed, 6, _s())
        torch.cuda.synchronize()
        return o6, o

    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            _gemm_trips("residual epilogue", T, N, 2 if lvl is None else MAX_WG_PER_CU, ncu)
            res[lvl] = run()
    for lvl in LEVELS[1:]:
        assert torch.equal(res[lvl][0], res[None][0]), (lvl, "split6_res")
        assert torch.equal(res[lvl][1], res[None][1]), (lvl, "split_res")
    y64 = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    f = sc.double().repeat_interleave(Hm * Wm)[:, None] if scaled else 1.0
    if windowed:
        ref = resid.double() + _window_reverse_roll(f * y64, B, Hm, Wm, shift)
        mag = _window_reverse_roll(f * mag, B, Hm, Wm, shift) + resid.double().abs()
    else:
        ref = resid.double() + f * y64
        mag = f * mag + resid.double().abs()
    for got in res[None]:
        err = (got.double() - ref).abs()
        assert (err <= BOUND6 * mag + 1e-7).all(), (err / mag).max().item()


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. weight gradients (split-T slabs, atomics per slab)
def _wgrad_plan(kind, T, nper, K, ncu):
    """(token slabs per tile, paired groups) of the dispatch of csrc/linear_split.hip (six terms) / csrc/linear_bf16.hip"""
    if kind == "split6":
        wm = 4 if nper % 128 == 0 else 2
        wn = 4 if K % 128 == 0 and wm == 2 else 2
        tiles, stage, min_stages = (nper // (32 * wm)) * (K // (32 * wn)), 32, 8
    else:
        tiles, stage, min_stages = (nper // (128 if nper % 128 == 0 else 64)) * (K // (128 if K % 128 == 0 else 64)), 64, 4
    nsplit = max(1, min(2 * ncu // tiles, max(1, T // (stage * min_stages))))
    paired = nsplit >= 2 and (nsplit % 2 == 0 or nsplit >= 16) and T // stage // nsplit <= 32
    return nsplit, paired


# (T, nper, K): 512 x 640 weights have at least 20 tiles of 128 x 128 or smaller, so at 8 and 9 CUs every kernel's split count
# (<= 2 x CUs / tiles) falls to one slab over the whole T; T = 4736 at the whole device: short slabs on the paired-group path
@pytest.mark.parametrize("kind,T,nper,K", [("split6", 65536 + 4736, 512, 640), ("split3", 65536 + 4736, 512, 640),
                                           ("fp32", 65536 + 4736, 512, 640), ("bf16", 65536 + 4736, 512, 640),
                                           ("split6", 4736, 128, 128), ("bf16", 4736, 128, 128)])
def test_wgrad_multi_trip(kind, T, nper, K):
    from dehaze_hip import _lib
    g = torch.Generator(device=DEV).manual_seed(T + nper + K)
    N = nper
    dt = BF if kind == "bf16" else torch.float32
    dy = torch.randn(T, N, generator=g, device=DEV).to(dt)
    x = torch.randn(T, K, generator=g, device=DEV).to(dt)

    def run():
        dw = torch.zeros(nper, K, device=DEV)
        db = torch.zeros(nper, device=DEV)
        pw = ctypes.cast((ctypes.c_void_p * 1)(dw.data_ptr()), ctypes.c_void_p)
        pb = ctypes.cast((ctypes.c_void_p * 1)(db.data_ptr()), ctypes.c_void_p)
        if kind == "bf16":
            _lib.call("dhz_linear_wgrad_bf16", dy.data_ptr(), N, x.data_ptr(), K, T, 1, nper, K, pw, pb, _s())
        elif kind == "fp32":
            _lib.call("dhz_linear_wgrad_multi", dy.data_ptr(), N, x.data_ptr(), K, T, 1, nper, K, pw, pb, _s())
        else:
            _lib.call("dhz_linear_wgrad_split", dy.data_ptr(), N, x.data_ptr(), K, T, 1, nper, K, pw, pb, None, 0,
                      3 if kind == "split3" else 6, _s())
        torch.cuda.synchronize()
        return dw, db

    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            if T == 4736:
                assert lvl is not None or _wgrad_plan(kind, T, nper, K, ncu)[1], "short slabs: the paired-group path"
            elif lvl is not None:
                assert (nper // 128) * (K // 128) >= 2 * ncu, "one slab per tile at this grid"
                if kind in ("split6", "bf16"):
                    assert _wgrad_plan(kind, T, nper, K, ncu)[0] == 1
            else:
                assert (nper // 128) * (K // 128) < ncu, "several slabs per tile on the whole device"
            res[lvl] = run()
    ref = dy.double().t() @ x.double()
    mag = dy.double().abs().t() @ x.double().abs()
    refb, magb = dy.double().sum(0), dy.double().abs().sum(0)
    bound = 2.0 ** -15 if kind == "split3" else RED
    for lvl in LEVELS:
        dw, db = res[lvl]
        for name, got, r, m in (("dW", dw, ref, mag), ("db", db, refb, magb)):
            err = (got.double() - r).abs()
            assert (err <= bound * m + 1e-5).all(), (kind, lvl, name, (err / m).max().item())
        if lvl is not None:
            _check_red((lvl, "dW"), dw, res[None][0], mag, 1e-6)
            _check_red((lvl, "db"), db, res[None][1], magb, 1e-6)


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. LayerNorm + partition backward (capped grid of 2 x CUs, two token groups per trip; dgamma / dbeta atomics per workgroup)
@pytest.mark.parametrize("dtype,C,shift", [("f32", 32, 4), ("f32", 128, 0), ("bf16", 64, 4), ("bf16", 256, 0)])
def test_ln_partition_backward_multi_trip(dtype, C, shift):
    from dehaze_hip import _lib
    Hm, Wm = 40, 56
    full = physical_cus()
    B = -(-3 * 8 * 8 * 2 * full // (Hm * Wm)) + 2                   # 8 tokens per group, 8 groups per workgroup and trip, 2 x CUs workgroups
    T = B * Hm * Wm
    g = torch.Generator(device=DEV).manual_seed(C + shift)
    dt = BF if dtype == "bf16" else torch.float32
    code = 1 if dtype == "bf16" else 0
    x = torch.randn(T, C, generator=g, device=DEV).to(dt)
    gamma = 1.0 + 0.1 * torch.randn(C, generator=g, device=DEV)
    beta = 0.1 * torch.randn(C, generator=g, device=DEV)
    dxw = torch.randn(T, C, generator=g, device=DEV).to(dt)
    dres = torch.randn(T, C, generator=g, device=DEV).to(dt)
    xn = torch.empty_like(x)
    stats = torch.empty(T, 2, device=DEV)
    _lib.call("dhz_ln_partition_fwd_dt", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), xn.data_ptr(), stats.data_ptr(), B, Hm, Wm, C,
              shift, 1, code, _s())

    def run():
        dx = torch.full_like(x, float("nan"))
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        _lib.call("dhz_ln_partition_bwd_lay", dxw.data_ptr(), x.data_ptr(), gamma.data_ptr(), stats.data_ptr(), dres.data_ptr(),
                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), B, Hm, Wm, C, shift, 1, 0, 0, 0, code, _s())
        torch.cuda.synchronize()
        return dx, dg, db

    lpt = {("f32", 32): 8, ("f32", 128): 32, ("bf16", 64): 8, ("bf16", 256): 32}[(dtype, C)]   # lanes per token (elementwise.hip)
    groups = -(-T // (64 // lpt))                                   # token groups of one wave
    res = {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            grid = min(2 * ncu, max(64, -(-T * lpt // 2048)))       # the launcher's capped grid
            assert_trips("LayerNorm backward (two groups per wave and trip)", groups, 2 * 4 * grid)
            res[lvl] = run()
    for lvl in LEVELS[1:]:
        assert torch.equal(res[lvl][0], res[None][0]), lvl                                       # (a)
    # float64 reference: dxw arrives in the window order of `shift`; dx = LN backward of it (in token order) + dres
    def unperm(t):
        m = t.double().view(B, Hm // 8, Wm // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hm, Wm, C)
        if shift:
            m = torch.roll(m, shifts=(shift, shift), dims=(1, 2))
        return m.reshape(T, C)
    x64 = x.double()
    dyt = unperm(dxw)
    mean = x64.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + 1e-5)
    xhat = (x64 - mean) * rstd
    dxhat = dyt * gamma.double()
    ref_dx = rstd * (dxhat - dxhat.mean(-1, keepdim=True) - xhat * (dxhat * xhat).mean(-1, keepdim=True)) + dres.double()
    ref_dg, ref_db = (dyt * xhat).sum(0), dyt.sum(0)
    mag_dg, mag_db = (dyt * xhat).abs().sum(0), dyt.abs().sum(0)
    dx0 = res[None][0].double()
    if dtype == "f32":
        assert torch.allclose(dx0, ref_dx, atol=2e-5, rtol=1e-4), (dx0 - ref_dx).abs().max()
    else:
        err = (dx0 - ref_dx).abs()
        assert (err <= EPS * ref_dx.abs() + 1e-4 * rstd * (dxhat.abs().amax(-1, keepdim=True) + 1)).all(), err.max().item()
    for lvl in LEVELS:
        _, dg, db = res[lvl]
        _check_red((lvl, "dgamma"), dg, ref_dg, mag_dg, 1e-5)
        _check_red((lvl, "dbeta"), db, ref_db, mag_db, 1e-5)


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. one whole training step
class _MagF:
    """torch.nn.functional for the oracle, with the parameter products recording the magnitude of their gradient's terms: for
    out = f(x, w) + b (linear / conv2d / conv_transpose2d, linear in w), mag(w) = the w-gradient of <|dy|, f(|x|, w)> and
    mag(b) = sum |dy|; for layer_norm, mag(gamma) = sum |dy xhat|, mag(beta) = sum |dy|"""

    def __init__(self, mag, nterms):
        self._mag, self._n = mag, nterms

    def __getattr__(self, name):
        return getattr(F, name)

    def _add(self, p, m, n):
        if p is not None and p.requires_grad:
            self._mag[id(p)] = self._mag.get(id(p), 0) + m.detach()
            self._n[id(p)] = self._n.get(id(p), 0) + n

    def _bilinear(self, fn, chan, x, w, b=None, *a, **kw):
        out = fn(x, w, b, *a, **kw)
        if out.requires_grad:
            ax = x.detach().abs()

            def hook(dy):
                ady = dy.abs()
                with torch.enable_grad():
                    wd = w.detach().clone().requires_grad_()
                    (gw,) = torch.autograd.grad((fn(ax, wd, None, *a, **kw) * ady).sum(), wd)
                n = ady.numel() // ady.shape[chan]              # terms per element: the output positions (x tokens)
                self._add(w, gw, n)
                if b is not None:
                    self._add(b, ady.movedim(chan, -1).reshape(-1, ady.shape[chan]).sum(0), n)
            out.register_hook(hook)
        return out

    def linear(self, x, w, b=None):
        return self._bilinear(F.linear, -1, x, w, b)

    def conv2d(self, x, w, b=None, *a, **kw):
        return self._bilinear(F.conv2d, 1, x, w, b, *a, **kw)

    def conv_transpose2d(self, x, w, b=None, *a, **kw):
        return self._bilinear(F.conv_transpose2d, 1, x, w, b, *a, **kw)

    def layer_norm(self, x, shape, weight=None, bias=None, eps=1e-5):
        out = F.layer_norm(x, shape, weight, bias, eps)
        if out.requires_grad:
            xd = x.detach()
            xhat = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps)

            def hook(dy):
                n = dy.numel() // xhat.shape[-1]
                self._add(weight, (dy * xhat).abs().reshape(-1, xhat.shape[-1]).sum(0), n)
                self._add(bias, dy.abs().reshape(-1, xhat.shape[-1]).sum(0), n)
            out.register_hook(hook)
        return out


def _oracle_grad_magnitudes(P, hazy, gt):
    """{parameter name: (sum over the terms of its gradient of |term|, number of terms)} for one oracle training step (Charbonnier, DropPath off), so that
    two gradients of the same step that differ only in the order of their sums can be compared elementwise; the bias tables' terms come
    from the per-window bias rows of each attention core"""
    P = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in P.items()}
    mag, nterms, tables = {}, {}, []
    keep = O.F, O.prob_attention, O.window_attention
    pre = [None]

    def window_attention(xw, P_, pre_, *a, **kw):
        pre[0] = pre_
        return keep[2](xw, P_, pre_, *a, **kw)

    def prob_attention(q, k, v, idx, bias=None, mask=None, return_aux=False):
        assert not return_aux
        B_, H, N, d = q.shape
        ks = k[:, :, idx, :]
        Mq = torch.matmul(q.unsqueeze(-2), ks.transpose(-2, -1)).squeeze(-2)
        top = (Mq.max(-1)[0] - Mq.sum(-1) / N).topk(idx.shape[1], sorted=False)[1]
        ctx, _, bsel = _prob_attention_given(q, k, v, idx, top, bias, mask)
        if bsel is not None:
            tables.append((pre[0] + "relative_position_bias_table", bsel, top, H))
        return ctx

    O.F, O.prob_attention, O.window_attention = _MagF(mag, nterms), prob_attention, window_attention
    try:
        torch.manual_seed(500)
        loss, _ = O.train_step_loss(P, hazy, gt, training=True, drop_path_rate=0.)
        loss.backward()
    finally:
        O.F, O.prob_attention, O.window_attention = keep
    out = {k: (mag[id(v)], nterms[id(v)]) for k, v in P.items() if id(v) in mag}
    for name, bsel, top, H in tables:                    # (an entry sums over at most 25 x 64 bias positions of every window)
        out[name] = (_table_mag(bsel, top, H).to(P[name].dtype), top.shape[0] * 25 * 64)
    return out


# 7. one whole training step: B = 3 at 128 x 128 (768 windows on the fused kernels' 2 x CUs grids), then the same step at 8 CUs
def test_training_step_multi_trip_vs_oracle():
    import My_model_1 as M1
    from dehaze_hip import _lib
    from dehaze_hip.train import FlatAdamW
    from losses import CharbonnierLoss
    lib = _lib.load()
    torch.manual_seed(1234)
    model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff', drop_path_rate=0.).to(DEV)
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    P = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(3, 3, 128, 128, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(3, 1, 1, 1, generator=g)).clamp(0, 1)
    crit = CharbonnierLoss()
    nwin = 3 * 16 * 16
    parts = lib.dhz_fused_attn_bwd_parts(nwin)
    assert nwin > parts and nwin % parts != 0, (nwin, parts)                # a ragged second trip at level 0 (512 on 256 CUs)

    def step():
        model.load_state_dict(state0)
        model.zero_grad(set_to_none=True)
        model.eval()
        torch.manual_seed(77)
        with torch.no_grad():
            y = model(hazy.to(DEV))
        model.train()
        torch.manual_seed(500)
        loss, _ = crit.forward_clamped(model(hazy.to(DEV)), gt.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        return y, loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    y0, loss0, g0 = step()
    with reserved_grid(8):
        y8, loss8, g8 = step()
    assert torch.equal(y8, y0)                                                                    # (a) eval output
    assert g8.keys() == g0.keys()
    mag = _oracle_grad_magnitudes(P, hazy, gt)
    assert set(g0) <= set(mag), sorted(set(g0) - set(mag))
    # (b) elementwise: at 8 CUs one token slab per tile replaces many - sums of n terms reordered and regrouped, whose fp32 error is
    # of the order sqrt(n) u mag (measured up to 0.9 of it); 8 sqrt(n) u mag still sees a lost slab, which the worst case n u mag would not
    for n in g0:
        m, nt = mag[n]
        err = (g8[n].cpu().double() - g0[n].cpu().double()).abs()
        bad = err > 8 * nt ** 0.5 * 2.0 ** -24 * m.double() + 1e-10
        assert not bad.any(), (n, nt, int(bad.sum()), (err / (m.double() * nt ** 0.5 * 2.0 ** -24 + 1e-30)).max().item())
    # (c) the oracle on the CPU, then one AdamW step each
    torch.manual_seed(500)
    loss_ref, _ = O.train_step_loss(P, hazy, gt, training=True, drop_path_rate=0.)
    assert abs(loss0.item() - loss_ref.item()) < 5e-5, (loss0.item(), loss_ref.item())
    ref_params = [P[n] for n, _ in model.named_parameters()]
    opt_ref = torch.optim.AdamW(ref_params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    loss_ref.backward()
    opt_ref.step()
    model.load_state_dict(state0)
    opt = FlatAdamW(model, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    model.train()
    opt.zero_grad()
    torch.manual_seed(500)
    loss, _ = crit.forward_clamped(model(hazy.to(DEV)), gt.to(DEV))
    loss.backward()
    opt.step()
    sd = model.state_dict()
    worst = max((sd[k].cpu() - P[k].detach()).abs().max().item() for k in P if P[k].dtype.is_floating_point)
    assert worst < 5e-4, worst
