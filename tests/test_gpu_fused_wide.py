"""-m gpu: the fused window-attention forward at C = 64 / 128 (csrc/fused_attn.hip), every exported instance, against float64.

At these widths the kernel runs one workgroup per window with a head loop (2 / 4 heads, the out-projection accumulated across heads),
weights from the fp32 fragment pack or brought by LDS-DMA as six-term planes, and two epilogue passes at C = 128.  The twelve
instances (C x {fp32 pipe, six-term} x {no saves, rank_save alone, all five saves}) are launched through the raw C-ABI on four small
geometries, each the smallest at which one kind of indexing mistake shows:

  drop    B = 3, 16 x 24, shift 0, bias, DropPath factors [1/0.9, 0, 1/0.9]: the image index of drop_scale (B > 1), a dropped image
          returns x bit for bit; 2 x 3 windows per image;
  mask    B = 2, 24 x 16, shift 4, bias, mask, two different DropPath factors: 3 x 2 windows (rows and columns the other way round),
          the mask row of the window INSIDE its image;
  row     B = 2, 8 x 24, shift 3, mask, no bias, no DropPath vector: a single row of windows, an odd shift (the oracle's mask:
          dhz_shift_mask takes only maps of more than one window each way; everywhere else the mask is ops.shift_mask's, and equal);
  nomask  B = 1, 16 x 16, shift 4, bias, mask = NULL: a shifted call without a mask.

SELECTION PRECONDITION.  The top-25 selection is a discontinuous function of the inputs, so every case first asserts - on the inputs
alone, in float64 - that in every window-head the 25th and the 26th largest sparsity measure are at least GAP = 1e-4 max|M| apart (ten
times the near-tie tolerance of _check_selection; fp32 measures are off by ~1e-6 max|M|).  The seeds below were found by a search on
the CPU (inputs come from a CPU generator) and are hard-coded; about one seed in three passes.  Gaps INSIDE the top 25 go down to 1e-7,
so ranks are never compared in order, only the selected set.  With the precondition holding no check has an exception share: every
element is inside its bound.

Every bound is one stage's own (each save is compared with float64 computed from the PREVIOUS stage's saved tensor):
  out         end-to-end float64 branch with the float64 selection: |err| <= 2e-5 + 1e-4 |ref| (test_fused_attention_c32_multi_trip)
  xn_save     float64 LayerNorm of x, rolled and partitioned: atol 1e-5, rtol 1e-5 (test_ln_partition)
  stats_save  by SOURCE token: mean |err| <= (C + 2) 2^-24 mean_i |x_i|; rstd relative <= (2 C + 16) 2^-24 (fp32 summation of C terms
              in any order, one rsqrt)
  qkv_save    float64 xn_save W^T + b: six-term |err| <= BOUND6 (sum |xn||w| + |b|); fp32 pipe |err| <= (2e-6 sqrt(C) + 1e-5) max(1,
              max |ref|) (test_linear_gemm_c_abi)
  ctx_save    float64 ProbSparse core on qkv_save with the kernel's selection: |err| <= 2e-5 + 1e-4 |ref|
  rank_save   the values below 25 are a permutation of 0..24, all others 255, the selected set is the float64 top-25
Every output and save buffer is pre-filled with NaN (ranks: an invalid value) and followed by 64 guard elements that must survive;
operands the header declares unread (wo_p of dhz_fused_window_attn_fwd6 at C = 64) are NaN.

The second part runs the branch as a training step does at these widths - fused._attn_fused_fwd with all five saves, then the
backward kernel chain of fused._attn_bwd - against float64 gradients, with both arithmetic forms.  The third part checks that the
argument check refuses what the header forbids and launches nothing.  Measured errors: profiles/fused_wide_tests.txt.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import uformer_oracle as O
from test_gpu_persistent import BOUND6, PNAMES, _check_red, _check_selection, _prob_attention_given, _table_mag, _top

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
U = 2.0 ** -24
GAP = 1e-4
PAD = 64
EINVAL = -22

GEOM = {
    "drop": dict(B=3, Hres=16, Wres=24, shift=0, bias=True, mask=False, dscale=(1 / 0.9, 0.0, 1 / 0.9)),
    "mask": dict(B=2, Hres=24, Wres=16, shift=4, bias=True, mask=True, dscale=(1 / 0.8, 1 / 0.9)),
    "row": dict(B=2, Hres=8, Wres=24, shift=3, bias=False, mask=True, dscale=None),
    "nomask": dict(B=1, Hres=16, Wres=16, shift=4, bias=True, mask=False, dscale=None),
    # the two cases of the training-step part
    "step64": dict(B=3, Hres=16, Wres=24, shift=4, bias=True, mask=True, dscale=(1 / 0.9, 0.0, 1 / 0.9)),
    "step128": dict(B=2, Hres=24, Wres=16, shift=0, bias=True, mask=False, dscale=(1 / 0.9, 0.0)),
}
# (C, geometry) -> seed whose inputs hold the selection precondition (searched on the CPU: the lowest seed from 1 whose smallest gap is
# at least 1.5 GAP, so that the float64 gap does not sit on the threshold itself; the gaps found: 1.5e-4 .. 2.6e-3 max|M|)
SEEDS = {
    (64, "drop"): 1, (64, "mask"): 1, (64, "row"): 2, (64, "nomask"): 1,
    (128, "drop"): 1, (128, "mask"): 6, (128, "row"): 3, (128, "nomask"): 3,
    (64, "step64"): 1, (128, "step128"): 2,
}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _inputs(C, geo, seed):
    """the distribution of test_gpu_persistent._attn_inputs at width C, from a CPU generator"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    L = geo["Hres"] * geo["Wres"]
    P = dict(gamma=1 + 0.1 * r(C), beta=0.1 * r(C), wq=r(C, C) / C ** 0.5, bq=0.1 * r(C), wk=r(C, C) / C ** 0.5, bk=0.1 * r(C),
             wv=r(C, C) / C ** 0.5, bv=0.1 * r(C), wo=r(C, C) / C ** 0.5, bo=0.1 * r(C), table=0.3 * r(225, C // 32))
    x = r(geo["B"], L, C)
    dout = r(geo["B"], L, C)
    idx = torch.randint(64, (64, 25), generator=g)
    return x, dout, idx, P


def _windows(t, geo):
    """[B, L, C] tokens -> [B * nW, 64, C]: rolled by -shift and partitioned, rows (b nW + w) 64 + token"""
    B, _, C = t.shape
    y = t.view(B, geo["Hres"], geo["Wres"], C)
    if geo["shift"]:
        y = torch.roll(y, shifts=(-geo["shift"], -geo["shift"]), dims=(1, 2))
    return O.window_partition(y, 8)


def _heads(t, H):
    """[B_, 64, 32 H] -> [B_, H, 64, 32]: head h is columns 32 h .. 32 h + 31"""
    return t.view(t.shape[0], 64, H, 32).transpose(1, 2)


def _measure(q, k, idx):
    """float64 sparsity measure [B_, H, 64]: max - sum / 64 of the 25 sampled scores of every query"""
    S = torch.matmul(q.unsqueeze(-2), k[:, :, idx, :].transpose(-2, -1)).squeeze(-2)
    return S.max(-1)[0] - S.sum(-1) / 64


def _gap_share(M):
    """smallest gap between the 25th and the 26th largest measure over the window-heads, as a share of max|M| of its window-head"""
    srt = M.sort(-1, descending=True)[0]
    return ((srt[..., 24] - srt[..., 25]) / M.abs().amax(-1)).min().item()


def _core64(q, k, v, idx, top, table, geo, H):
    """float64 ProbSparse core with the selection `top`, bias rows of `table` [225, H] and the oracle's shift mask"""
    bias = mask = None
    if geo["bias"]:
        bias = table[O.relative_position_index(8).reshape(-1)].reshape(64, 64, H).permute(2, 0, 1)
    if geo["mask"]:
        mask = O.shift_attn_mask(geo["Hres"], geo["Wres"], 8, geo["shift"], torch.float64)
    ctx, _, bsel = _prob_attention_given(q, k, v, idx, top, bias, mask)
    return ctx.transpose(1, 2).reshape(q.shape[0], 64, 32 * H), bsel


def _ref64(x, P, idx, geo, top=None, dout=None):
    """float64 attention branch on the CPU (O.lewin_block's first half).  top = None: the float64 top-25.  With dout: the gradients
    and the magnitudes of their terms as well (test_gpu_persistent._attn_ref at any width)."""
    B, L, C = x.shape
    H = C // 32
    x = x.double().requires_grad_()
    prm = {n: t.double().requires_grad_() for n, t in P.items()}
    xn = F.layer_norm(x, (C,), prm["gamma"], prm["beta"], 1e-5)
    xn.retain_grad()
    xw = _windows(xn, geo)
    lin = {}
    for n in "qkv":
        lin[n] = F.linear(xw, prm["w" + n], prm["b" + n])
        lin[n].retain_grad()
    q, k, v = (_heads(lin[n], H) for n in "qkv")
    M = _measure(q.detach(), k.detach(), idx)
    if top is None:
        top = M.topk(25, sorted=False)[1]
    ctx, bsel = _core64(q, k, v, idx, top, prm["table"], geo, H)
    aw = F.linear(ctx, prm["wo"], prm["bo"])
    aw.retain_grad()
    y = O.window_reverse(aw, 8, geo["Hres"], geo["Wres"])
    if geo["shift"]:
        y = torch.roll(y, shifts=(geo["shift"], geo["shift"]), dims=(1, 2))
    f = torch.tensor(geo["dscale"], dtype=torch.float32).double()[:, None, None] if geo["dscale"] else 1.0
    out = x + f * y.reshape(B, L, C)
    res = dict(out=out.detach(), M=M, top=top, xw=xw.detach())
    if dout is not None:
        out.backward(dout.double())
        tok = lambda t: t.detach().reshape(-1, t.shape[-1]).abs()
        xd = x.detach()
        xhat = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
        mag = dict(gamma=(tok(xn.grad) * tok(xhat)).sum(0), beta=tok(xn.grad).sum(0), table=_table_mag(bsel, top, H),
                   wo=tok(aw.grad).t() @ tok(ctx), bo=tok(aw.grad).sum(0))
        for n in "qkv":
            mag["w" + n] = tok(lin[n].grad).t() @ tok(xw)
            mag["b" + n] = tok(lin[n].grad).sum(0)
        res.update(dx=x.grad, grads={n: prm[n].grad for n in PNAMES}, mag=mag)
    return res


@functools.lru_cache(maxsize=None)
def _case(C, name):
    """inputs and the end-to-end float64 reference of one (width, geometry), computed once and shared; read-only.  The selection
    precondition is asserted here, on the inputs alone, before any kernel output is looked at."""
    geo = GEOM[name]
    x, dout, idx, P = _inputs(C, geo, SEEDS[(C, name)])
    ref = _ref64(x, P, idx, geo)
    share = _gap_share(ref["M"])
    assert share >= GAP, f"C = {C}, {name}: the 25th and 26th largest measure are {share:.2e} max|M| apart in some window-head: pick another seed"
    return x, dout, idx, P, ref


def _within(label, got, ref, bound, text):
    """every element of got within `bound` (a tensor or a number) of ref; prints the worst error and its share of the bound"""
    err = (got.double() - ref).abs()
    share = (err / bound).max().item()
    print(f"{label}: worst error {err.max().item():.3e}, {share:.3f} of the bound ({text})")
    assert share <= 1.0, (label, share, int((err > bound).sum()))           # (a NaN fails too)


def _guarded(n, dtype=torch.float32):
    """n elements of 'never written' (NaN; an invalid rank for bytes) followed by PAD guard elements holding a pattern"""
    if dtype == torch.uint8:
        buf = torch.full((n + PAD,), 99, dtype=torch.uint8)
        buf[n:] = torch.arange(100, 100 + PAD, dtype=torch.uint8)
    else:
        buf = torch.full((n + PAD,), NAN)
        buf[n:] = torch.arange(PAD, dtype=torch.float32) + 0.5
    return buf.to(DEV)


def _guard_ok(buf, n):
    want = torch.arange(100, 100 + PAD, dtype=torch.uint8) if buf.dtype == torch.uint8 else torch.arange(PAD, dtype=torch.float32) + 0.5
    return torch.equal(buf[n:].cpu(), want)


def _operands(C, form, P, geo):
    """device operands of one raw call: (weights argument, wo_p, bqkv, bias tile or None, mask or None, drop_scale or None) and the
    parameters on the device"""
    from dehaze_hip import _lib, fused, ops
    H = C // 32
    d = {n: t.to(DEV) for n, t in P.items()}
    w4 = [d[n].data_ptr() for n in ("wq", "wk", "wv", "wo")]
    wqkv_p = torch.full((3 * C * C,), NAN, device=DEV)
    wo_p = torch.full((C * C,), NAN, device=DEV)
    _lib.call("dhz_fused_attn_prepack", *w4, wqkv_p.data_ptr(), wo_p.data_ptr(), C, _s())
    warg = wqkv_p
    if form == "p6":
        warg = torch.full((fused._n6(C),), NAN, device=DEV).to(torch.bfloat16)
        _lib.call("dhz_fused_attn_prepack6", *w4, warg.data_ptr(), C, _s())
        if C == 64:
            wo_p = torch.full((C * C,), NAN, device=DEV)                    # include/dehaze_hip.h: not read
    torch.cuda.synchronize()
    assert not torch.isnan(warg.float()).any()
    bqkv = torch.cat([d["bq"], d["bk"], d["bv"]])
    bias = mask = dscale = None
    if geo["bias"]:
        bias = torch.full((H * 64 * 64,), NAN, device=DEV)
        _lib.call("dhz_bias_gather", d["table"].data_ptr(), bias.data_ptr(), H, _s())
        want = P["table"][O.relative_position_index(8).reshape(-1)].reshape(64, 64, H).permute(2, 0, 1)
        assert torch.equal(bias.view(H, 64, 64).cpu(), want)
    if geo["mask"]:
        want = O.shift_attn_mask(geo["Hres"], geo["Wres"], 8, geo["shift"])
        if min(geo["Hres"], geo["Wres"]) > 8:
            mask = ops.shift_mask(geo["Hres"], geo["Wres"], geo["shift"], DEV)
            assert torch.equal(mask.cpu(), want)
        else:                              # dhz_shift_mask takes maps of more than one window each way: the single row gets the oracle's mask
            mask = want.to(DEV)
    if geo["dscale"]:
        dscale = torch.tensor(geo["dscale"], dtype=torch.float32, device=DEV)
    return d, warg, wo_p, bqkv, bias, mask, dscale


ENTRY = {"f32": "dhz_fused_window_attn_fwd", "p6": "dhz_fused_window_attn_fwd6"}


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. the raw C-ABI forward, all twelve C = 64 / 128 instances
@pytest.mark.parametrize("name", ["drop", "mask", "row", "nomask"])
@pytest.mark.parametrize("mode", ["none", "rank", "all"])
@pytest.mark.parametrize("form", ["f32", "p6"])
@pytest.mark.parametrize("C", [64, 128])
def test_fused_forward_wide_vs_float64(C, form, mode, name):
    from dehaze_hip import _lib
    geo = GEOM[name]
    x, _, idx, P, ref = _case(C, name)                                      # (asserts the selection precondition)
    H = C // 32
    B, Hres, Wres, shift = geo["B"], geo["Hres"], geo["Wres"], geo["shift"]
    T = B * Hres * Wres
    B_ = T // 64
    d, warg, wo_p, bqkv, bias, mask, dscale = _operands(C, form, P, geo)
    xd = x.to(DEV)
    idx8 = idx.to(torch.uint8).to(DEV)
    sizes = dict(out=T * C, xn=T * C, qkv=T * 3 * C, ctx=T * C, stats=T * 2, rank=B_ * H * 64)
    buf = {n: _guarded(sz, torch.uint8 if n == "rank" else torch.float32) for n, sz in sizes.items()}
    given = {"none": (), "rank": ("rank",), "all": ("xn", "qkv", "ctx", "stats", "rank")}[mode]
    sp = lambda n: buf[n].data_ptr() if n in given else None
    _lib.call(ENTRY[form], xd.data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), warg.data_ptr(), bqkv.data_ptr(), wo_p.data_ptr(),
              d["bo"].data_ptr(), idx8.data_ptr(), _p(bias), _p(mask), _p(dscale), buf["out"].data_ptr(), sp("xn"), sp("qkv"), sp("ctx"),
              sp("stats"), sp("rank"), B, Hres, Wres, C, shift, _s())
    torch.cuda.synchronize()
    label = f"fused_wide C={C} {form} saves={mode} {name}"
    # untouched memory: the guards behind every buffer, and the buffers of the saves that were not asked for
    for n, sz in sizes.items():
        assert _guard_ok(buf[n], sz), (label, n, "written behind the buffer")
        if n != "out" and n not in given:
            assert (buf[n][:sz] == 99).all() if n == "rank" else torch.isnan(buf[n][:sz]).all(), (label, n, "written without being asked for")
    _check_forward(label, C, form, mode, name, {n: buf[n][:sizes[n]].cpu() for n in ("out",) + given})


def _check_forward(label, C, form, mode, name, got):
    """got: what one forward call wrote (flat CPU tensors: out, and the saves of `mode`), against the float64 references"""
    geo = GEOM[name]
    x, _, idx, P, ref = _case(C, name)
    H = C // 32
    B, Hres, Wres = geo["B"], geo["Hres"], geo["Wres"]
    T = B * Hres * Wres
    B_ = T // 64
    for n in got:
        if n != "rank":
            assert not torch.isnan(got[n]).any(), (label, n, "elements left unwritten")

    out = got["out"].view(B, Hres * Wres, C)
    _within(f"{label} out", out, ref["out"], 2e-5 + 1e-4 * ref["out"].abs(), "atol 2e-5, rtol 1e-4")
    if geo["dscale"]:
        for b, f in enumerate(geo["dscale"]):
            if f == 0.0:
                assert torch.equal(out[b], x[b]), (label, "a dropped image is not x bit for bit")
    if mode == "none":
        return
    rank = got["rank"].view(B_, H, 64)
    sel = rank < 25
    assert (rank[~sel] == 255).all(), (label, "rank_save: a value that is neither below 25 nor 255")
    assert torch.equal(rank.masked_fill(~sel, 255).sort(-1)[0][..., :25].long(), torch.arange(25).expand(B_, H, 25)) \
        and (sel.sum(-1) == 25).all(), (label, "rank_save: the values below 25 are not a permutation of 0..24")
    _check_selection(label, rank, ref["M"])
    want = torch.zeros(B_, H, 64, dtype=torch.bool).scatter_(-1, ref["top"], True)
    assert torch.equal(sel, want), (label, "the selected set is not the float64 top-25", int((sel != want).sum()))
    if mode == "rank":
        return

    # xn_save: float64 LayerNorm of x in window order
    xn = got["xn"].view(B_, 64, C)
    _within(f"{label} xn_save", xn, ref["xw"], 1e-5 + 1e-5 * ref["xw"].abs(), "atol 1e-5, rtol 1e-5")
    # stats_save: (mean, rstd) by source token
    x64 = x.double().view(T, C)
    stats = got["stats"].view(T, 2)
    mean = x64.mean(-1)
    rstd = 1.0 / torch.sqrt(x64.var(-1, unbiased=False) + 1e-5)
    _within(f"{label} stats_save mean", stats[:, 0], mean, (C + 2) * U * x64.abs().mean(-1), f"(C + 2) 2^-24 mean|x| = {(C + 2) * U:.2e} mean|x|")
    _within(f"{label} stats_save rstd", stats[:, 1], rstd, (2 * C + 16) * U * rstd, f"relative (2 C + 16) 2^-24 = {(2 * C + 16) * U:.2e}")
    # qkv_save: float64 product of the kernel's own xn_save
    qkv = got["qkv"].view(B_, 64, 3 * C)
    w64 = torch.cat([P["wq"], P["wk"], P["wv"]]).double()
    b64 = torch.cat([P["bq"], P["bk"], P["bv"]]).double()
    rq = xn.double() @ w64.t() + b64
    if form == "p6":
        _within(f"{label} qkv_save", qkv, rq, BOUND6 * (xn.double().abs() @ w64.abs().t() + b64.abs()), "2^-21 (sum |xn||w| + |b|)")
    else:
        tol = (2e-6 * C ** 0.5 + 1e-5) * max(1.0, rq.abs().max().item())
        _within(f"{label} qkv_save", qkv, rq, tol, f"(2e-6 sqrt(C) + 1e-5) max(1, max|ref|) = {tol:.2e}")
    # ctx_save: float64 ProbSparse core on the kernel's own qkv_save with the kernel's own selection
    q, k, v = (_heads(qkv[..., i * C:(i + 1) * C].double().contiguous(), H) for i in range(3))
    rc, _ = _core64(q, k, v, idx, _top(rank).long(), P["table"].double().requires_grad_(), geo, H)
    rc = rc.detach()
    _within(f"{label} ctx_save", got["ctx"].view(B_, 64, C), rc, 2e-5 + 1e-4 * rc.abs(), "atol 2e-5, rtol 1e-4")


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the branch as the training step runs it: fused forward with all five saves, then the backward kernel chain
@pytest.mark.parametrize("p6", [False, True])
@pytest.mark.parametrize("C,name", [(64, "step64"), (128, "step128")])
def test_fused_branch_wide_forward_backward_vs_float64(C, name, p6):
    """one grid level: at these widths the forward is one workgroup per window, and the chain's persistent kernels have their
    multi-trip tests (test_gpu_persistent.py)"""
    from dehaze_hip import _lib, fused, ops
    geo = GEOM[name]
    H = C // 32
    x, dout, idx, P, ref0 = _case(C, name)
    B, Hres, Wres, shift = geo["B"], geo["Hres"], geo["Wres"], geo["shift"]
    assert 0.0 in geo["dscale"]
    mask = ops.shift_mask(Hres, Wres, shift, DEV) if shift else None
    prm = {n: t.to(DEV).requires_grad_() for n, t in P.items()}
    dscale = torch.tensor(geo["dscale"], dtype=torch.float32, device=DEV)
    args = (x.to(DEV), prm["gamma"], prm["beta"], prm["wq"], prm["bq"], prm["wk"], prm["bk"], prm["wv"], prm["bv"], prm["wo"], prm["bo"],
            prm["table"], idx.to(torch.uint8).to(DEV), mask, dscale, Hres, Wres, shift, H)
    called = []
    keep = fused.ATTN_FUSED_P6, _lib.call

    def spy(entry, *a):
        called.append(entry)
        return keep[1](entry, *a)

    fused.ATTN_FUSED_P6, _lib.call = p6, spy
    try:
        with torch.no_grad():
            out, rec = fused._attn_fused_fwd(True, *args)
    finally:
        fused.ATTN_FUSED_P6, _lib.call = keep
    assert ENTRY["p6" if p6 else "f32"] in called and ENTRY["f32" if p6 else "p6"] not in called, called
    assert rec.kind == "attn_chain_bwd"
    rank = rec.saved[6].clone().view(-1, H, 64).cpu()
    with torch.no_grad():
        ret = fused._attn_bwd(rec, dout.to(DEV))
    for n, gr in zip(PNAMES, ret[1:]):
        if gr is not None:
            prm[n].grad = gr if prm[n].grad is None else prm[n].grad + gr
    torch.cuda.synchronize()
    label = f"fused_wide branch C={C} {'p6' if p6 else 'f32'} {name}"
    _check_selection(label, rank, ref0["M"])
    want = torch.zeros_like(rank, dtype=torch.bool).scatter_(-1, ref0["top"], True)
    assert torch.equal(rank < 25, want), (label, "the selected set is not the float64 top-25")
    ref = _ref64(x, P, idx, geo, top=_top(rank).long(), dout=dout)
    _within(f"{label} out", out.cpu(), ref["out"], 2e-5 + 1e-4 * ref["out"].abs(), "atol 2e-5, rtol 1e-4")
    _within(f"{label} dx", ret[0].cpu(), ref["dx"], 5e-5 + 1e-3 * ref["dx"].abs(), "atol 5e-5, rtol 1e-3")
    for b, f in enumerate(geo["dscale"]):
        if f == 0.0:
            assert torch.equal(out[b].cpu(), x[b]) and torch.equal(ret[0][b].cpu(), dout[b]), (label, "a dropped image: out = x, dx = dout")
    for n in PNAMES:
        got, mg = prm[n].grad.cpu().double(), ref["mag"][n]
        err = (got - ref["grads"][n]).abs()
        print(f"{label} d{n}: worst error {err.max().item():.3e}, {(err / (2.0 ** -18 * mg + 1e-5)).max().item():.3f} of the bound "
              f"(2^-18 of the summed magnitudes + 1e-5)")
        _check_red((label, n), got, ref["grads"][n], mg, 1e-5)


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. what the argument check refuses, for both entries: DHZ_EINVAL and nothing launched
@pytest.mark.parametrize("form", ["f32", "p6"])
def test_fused_forward_refusals(form):
    from dehaze_hip import _lib
    lib = _lib.load()
    C, geo = 64, GEOM["nomask"]
    x, _, idx, P, _ = _case(C, "nomask")
    d, warg, wo_p, bqkv, bias, _, _ = _operands(C, form, P, geo)
    B, Hres, Wres = 1, 16, 16
    T = B * Hres * Wres
    xd = x.to(DEV)
    idx8 = idx.to(torch.uint8).to(DEV)
    mask = torch.zeros(4, 64, 64, device=DEV)
    out = torch.full((T * C,), NAN, device=DEV)
    sv = dict(xn=torch.empty(T * C, device=DEV), qkv=torch.empty(T * 3 * C, device=DEV), ctx=torch.empty(T * C, device=DEV),
              stats=torch.empty(T * 2, device=DEV), rank=torch.empty(T * (C // 32), dtype=torch.uint8, device=DEV))

    def rc(saves=(), mask_=None, Hres_=Hres, shift=4, C_=C):
        sp = lambda n: sv[n].data_ptr() if n in saves else None
        r = getattr(lib, ENTRY[form])(xd.data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), warg.data_ptr(), bqkv.data_ptr(),
                                      wo_p.data_ptr(), d["bo"].data_ptr(), idx8.data_ptr(), bias.data_ptr(), _p(mask_), None, out.data_ptr(),
                                      sp("xn"), sp("qkv"), sp("ctx"), sp("stats"), sp("rank"), B, Hres_, Wres, C_, shift, _s())
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "a refused call launched the kernel"
        return r

    for one in ("xn", "qkv", "ctx", "stats"):
        assert rc(saves=(one,)) == EINVAL, one
        assert rc(saves=(one, "rank")) == EINVAL, one
    assert b"save buffers" in lib.dhz_last_error()
    assert rc(saves=("xn", "qkv", "ctx", "stats")) == EINVAL
    assert rc(mask_=mask, shift=0) == EINVAL and b"mask" in lib.dhz_last_error()
    assert rc(Hres_=12) == EINVAL and b"geometry" in lib.dhz_last_error()
    assert rc(shift=8) == EINVAL and b"geometry" in lib.dhz_last_error()
    assert rc(C_=48) == EINVAL and b"C=48" in lib.dhz_last_error()
    # and the same operands are accepted when nothing is wrong with the call
    assert getattr(lib, ENTRY[form])(
        xd.data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(), warg.data_ptr(), bqkv.data_ptr(), wo_p.data_ptr(), d["bo"].data_ptr(),
        idx8.data_ptr(), bias.data_ptr(), None, None, out.data_ptr(), None, None, None, None, None, B, Hres, Wres, C, 4, _s()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
