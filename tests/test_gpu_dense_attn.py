"""-m gpu: the dense 8 x 8 window attention of the My_model.Uformer twin (csrc/dense_attn.hip: dhz_dense_attn_fwd / dhz_dense_attn_bwd)
through the raw C-ABI against oracle.uformer_oracle.dense_attention in float64 with autograd.

The model tests reach these entries with head dim 32, a bias and 4 or 8 windows only.  Here: all three forward instances (d = 16, 32, 64)
and all six backward instances (d x HAS_BIAS), with and without the shift mask; output / gradient row strides that differ from the input's
(views into wider NaN-filled buffers whose padding must stay NaN); and the persistent backward grid on 8 / 9 compute units, where a
workgroup walks several windows and sums their bias gradient in LDS.

Bounds: those of test_ps_attention_oracle (tests/test_gpu_kernels.py:122-124; the kernels have the same structure) -
out atol 2e-5 / rtol 1e-4, dq dk dv atol 1e-4 / rtol 1e-3, table gradient atol 2e-4 * sqrt(B_) / rtol 2e-3.  Every case prints its worst
absolute error and the worst error in units of its bound."""
import pytest
import torch

from _grid import assert_trips, reserved_grid
from oracle import uformer_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
# (B_, H, d, bias, mask)
CASES = [(4, 1, 16, True, True), (4, 2, 16, False, False), (8, 2, 32, False, True), (4, 4, 32, True, False),
         (4, 1, 64, True, True), (4, 2, 64, False, False)]
STRIDED = [(4, 1, 16, True, True), (4, 4, 32, True, False), (4, 2, 64, False, False)]        # one per head dim
MULTI_TRIP = [(52, 2, 32), (28, 1, 16)]

_REF = {}


def reference(B_, H, d, use_bias, use_mask):
    """inputs (fp32, CPU) and the float64 results of one case, computed once and shared (never modified)"""
    key = (B_, H, d, use_bias, use_mask)
    if key not in _REF:
        g = torch.Generator().manual_seed(B_ * 1009 + H * 31 + d + 2 * use_bias + use_mask)
        C = H * d
        qkv = torch.randn(B_ * 64, 3 * C, generator=g)
        table = 0.3 * torch.randn(225, H, generator=g)
        gout = torch.randn(B_ * 64, C, generator=g)
        mask = O.shift_attn_mask(16, 16, 8, 4) if use_mask else None                       # nW = 4
        ridx = O.relative_position_index(8).reshape(-1)
        qkv64 = qkv.double().requires_grad_()
        table64 = table.double().requires_grad_()
        q, k, v = (qkv64[:, i * C:(i + 1) * C].view(B_, 64, H, d).transpose(1, 2) for i in range(3))
        bias64 = table64[ridx].reshape(64, 64, H).permute(2, 0, 1) if use_bias else torch.zeros(H, 64, 64, dtype=torch.float64)
        out = O.dense_attention(q, k, v, bias64, mask.double() if use_mask else None, d ** -0.5).transpose(1, 2).reshape(B_ * 64, C)
        (out * gout.double()).sum().backward()
        bias = table[ridx].reshape(64, 64, H).permute(2, 0, 1).contiguous() if use_bias else None
        _REF[key] = dict(qkv=qkv, gout=gout, mask=mask, bias=bias, out=out.detach(), dqkv=qkv64.grad,
                         dtable=table64.grad if use_bias else None)
    return _REF[key]


def run(B_, H, d, r, ldo=None, ldg=None):
    """forward and backward through the C-ABI with NaN canaries in every output (and in the padding columns of strided buffers);
    returns out [T, C], dqkv [T, 3C], the table gradient [225, H] or None, and the workgroup count of the backward"""
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    C, T = H * d, B_ * 64
    ldo, ldg = ldo or C, ldg or 3 * C
    p = lambda t: None if t is None else t.data_ptr()
    qkv = r["qkv"].cuda()
    bias = None if r["bias"] is None else r["bias"].cuda()
    mask = None if r["mask"] is None else r["mask"].cuda()
    nW = 4 if mask is not None else 1
    outw = torch.full((T, ldo), NAN, device="cuda")
    doutw = torch.full((T, ldo), NAN, device="cuda")
    doutw[:, :C] = r["gout"].cuda()
    dqkvw = torch.full((T, ldg), NAN, device="cuda")
    base, gb = qkv.data_ptr(), dqkvw.data_ptr()
    scale = d ** -0.5
    _lib.call("dhz_dense_attn_fwd", base, base + 4 * C, base + 8 * C, 3 * C, p(bias), p(mask), outw.data_ptr(), ldo, B_, H, nW, d, scale, s)
    parts = lib.dhz_ps_attn_bwd_parts(B_, H)
    dpart = torch.full((parts, 64, 64), NAN, device="cuda") if bias is not None else None
    _lib.call("dhz_dense_attn_bwd", base, base + 4 * C, base + 8 * C, 3 * C, p(bias), p(mask), doutw.data_ptr(), ldo, gb, gb + 4 * C,
              gb + 8 * C, ldg, p(dpart), B_, H, nW, d, scale, s)
    dtable = None
    if bias is not None:
        dtable = torch.full((225, H), NAN, device="cuda")
        _lib.call("dhz_bias_table_grad", dpart.data_ptr(), parts, dtable.data_ptr(), H, 0, s)
    torch.cuda.synchronize()
    # "every element written": nothing of the live region is left NaN, nothing of the padding is touched
    assert not torch.isnan(outw[:, :C]).any() and torch.isnan(outw[:, C:]).all()
    assert not torch.isnan(dqkvw[:, :3 * C]).any() and torch.isnan(dqkvw[:, 3 * C:]).all()
    assert torch.isnan(doutw[:, C:]).all()
    if dpart is not None:
        assert not torch.isnan(dpart).any() and not torch.isnan(dtable).any()
    return outw[:, :C].cpu(), dqkvw[:, :3 * C].cpu(), None if dtable is None else dtable.cpu(), parts


def check(what, got, ref, atol, rtol):
    err = (got.double() - ref).abs()
    units = (err / (atol + rtol * ref.abs())).max().item()
    print(f"{what}: worst error {err.max().item():.3e}, {units:.3f} of the bound (atol {atol:.1e}, rtol {rtol:.0e})")
    assert units <= 1.0, (what, err.max().item(), units)


def check_all(tag, B_, H, d, r, out, dqkv, dtable):
    C = H * d
    check(f"{tag} out", out, r["out"], 2e-5, 1e-4)
    for i, name in enumerate(("dq", "dk", "dv")):
        check(f"{tag} {name}", dqkv[:, i * C:(i + 1) * C], r["dqkv"][:, i * C:(i + 1) * C], 1e-4, 1e-3)
    if r["dtable"] is not None:
        check(f"{tag} dtable", dtable, r["dtable"], 2e-4 * B_ ** 0.5, 2e-3)


@pytest.mark.parametrize("B_,H,d,use_bias,use_mask", CASES)
def test_dense_attention_matches_float64(B_, H, d, use_bias, use_mask):
    r = reference(B_, H, d, use_bias, use_mask)
    out, dqkv, dtable, _ = run(B_, H, d, r)
    check_all(f"dense_attn B_={B_} H={H} d={d} bias={use_bias} mask={use_mask}", B_, H, d, r, out, dqkv, dtable)


@pytest.mark.parametrize("B_,H,d,use_bias,use_mask", STRIDED)
def test_dense_attention_row_strides(B_, H, d, use_bias, use_mask):
    """ld = 3C, ldo = C + 8, ldg = 3C + 4: three different row strides; the padding columns stay NaN (asserted in run) and the
    values are those of the packed call, bit for bit - a stride moves no arithmetic"""
    r = reference(B_, H, d, use_bias, use_mask)
    C = H * d
    out, dqkv, dtable, _ = run(B_, H, d, r, ldo=C + 8, ldg=3 * C + 4)
    check_all(f"dense_attn strided B_={B_} H={H} d={d}", B_, H, d, r, out, dqkv, dtable)
    out0, dqkv0, _, _ = run(B_, H, d, r)
    assert torch.equal(out, out0) and torch.equal(dqkv, dqkv0)


@pytest.mark.parametrize("B_,H,d", MULTI_TRIP)
def test_dense_attention_backward_multi_trip(B_, H, d):
    """grids sized for 8 / 9 compute units: dhz_ps_attn_bwd_parts gives 2 x CUs / H workgroups per head, so each walks several windows
    (ragged last trip) and sums their bias gradient in LDS.  Same float64 bounds; dq dk dv are computed per window without atomics,
    so they are bit-equal to the run on the whole device, whatever the trip layout."""
    from dehaze_hip import _lib
    lib = _lib.load()
    r = reference(B_, H, d, True, False)
    out0, dqkv0, dtable0, parts0 = run(B_, H, d, r)
    check_all(f"dense_attn B_={B_} H={H} d={d} whole device ({parts0} workgroups)", B_, H, d, r, out0, dqkv0, dtable0)
    for ncu in (8, 9):
        with reserved_grid(ncu):
            parts = lib.dhz_ps_attn_bwd_parts(B_, H)
            assert parts % H == 0 and parts // H == 2 * ncu // H, (parts, ncu)
            per_head = parts // H
            if B_ >= 3 * per_head:
                assert_trips(f"dense backward on {ncu} CUs", B_, per_head)
            else:                                   # two trips are all this shape reaches: more windows than workgroups, ragged
                assert B_ > per_head and B_ % per_head != 0, (B_, per_head)
            out, dqkv, dtable, parts_run = run(B_, H, d, r)
        assert parts_run == parts
        check_all(f"dense_attn B_={B_} H={H} d={d} on {ncu} CUs ({per_head} workgroups per head)", B_, H, d, r, out, dqkv, dtable)
        assert torch.equal(out, out0) and torch.equal(dqkv, dqkv0), f"{ncu} CUs"


def test_dense_attention_refusals():
    """bad arguments return DHZ_EINVAL before any launch: the outputs keep their canaries"""
    from dehaze_hip import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    B_, H, d = 4, 2, 32
    C, T = H * d, B_ * 64
    qkv = torch.randn(T, 3 * C + 4, device="cuda")
    bias = torch.zeros(H, 64, 64, device="cuda")
    mask = torch.zeros(4, 64, 64, device="cuda")
    out = torch.full((T, C + 4), NAN, device="cuda")
    dqkv = torch.full((T, 3 * C + 4), NAN, device="cuda")
    dpart = torch.full((lib.dhz_ps_attn_bwd_parts(B_, H), 64, 64), NAN, device="cuda")
    b, gb, o = qkv.data_ptr(), dqkv.data_ptr(), out.data_ptr()

    def fwd(ld=3 * C, ldo=C, B=B_, nW=1, dd=d, m=None):
        return lib.dhz_dense_attn_fwd(b, b + 4 * C, b + 8 * C, ld, bias.data_ptr(), m, o, ldo, B, H, nW, dd, dd ** -0.5, s)

    def bwd(ld=3 * C, ldo=C, ldg=3 * C, B=B_, nW=1, dd=d, m=None, part=dpart.data_ptr()):
        return lib.dhz_dense_attn_bwd(b, b + 4 * C, b + 8 * C, ld, bias.data_ptr(), m, o, ldo, gb, gb + 4 * C, gb + 8 * C, ldg, part,
                                      B, H, nW, dd, dd ** -0.5, s)

    assert fwd(dd=8) == -22 and bwd(dd=8) == -22                                           # head dim 8: no instance
    assert fwd(ld=3 * C + 2) == -22 and fwd(ldo=C + 2) == -22                              # row strides in float4s
    assert bwd(ld=3 * C + 2) == -22 and bwd(ldo=C + 2) == -22 and bwd(ldg=3 * C + 2) == -22
    assert fwd(B=3, nW=4, m=mask.data_ptr()) == -22 and bwd(B=3, nW=4, m=mask.data_ptr()) == -22   # windows not in whole images
    assert bwd(part=None) == -22                                                           # a bias without room for its gradient
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(dqkv).all() and torch.isnan(dpart).all()
