"""-m gpu: K4 inside the GEMMs (round 6).  The out-projection / linear2 product whose epilogue is window reverse + un-roll + DropPath
factor + residual (dhz_linear_fwd_split6_res / dhz_linear_fwd_split_res, csrc/tok_epilogue.h; M1:859-873), the row-factor form of
the backward-data product, the gradient layouts of dhz_ln_partition_bwd_lay, and the whole-block autograd node (fused.block)
against the two-node form it replaces.  References are float64 restatements in torch of the reference's own op sequence
(window_reverse M1:577-601, torch.roll M1:866, shortcut + drop_path M1:872)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND6 = 2.0 ** -21          # same elementwise bound as tests/test_gpu_split.py (relative to sum |a||b|)


def _window_reverse_roll(yw, B, H, W, shift):
    """[B*nW*64, C] window-ordered rows -> [B*H*W, C] token order: window_reverse (M1:577-601) then roll(+shift) (M1:866)"""
    C = yw.shape[1]
    y = yw.view(B, H // 8, W // 8, 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2))
    return y.reshape(B * H * W, C)


# (B, H, W, K, N): token counts, widths and map geometries of the model's blocks, and the few-tile kernel of csrc/linear_split.hip
# (through its own entry point).  The kernel of csrc/split6_gemm.hip named behind each shape is what dhz_linear_split6_tile answers on
# the whole device (256 CUs): there these shapes never fill the 256 x 128 kernel and never meet the demotion to 128 x 64 -
# tests/test_gpu_split6_instances.py runs every instance of that file, epilogue form included, under reserved grids.
SHAPES = [(8, 64, 64, 128, 128),      # T = 32768: 128 x 128 (128 tiles of 256 rows < CUs)
          (2, 32, 32, 512, 128),      # T = 2048, N = 128: 128 x 128, 16 tiles; long contraction (LeFF linear2 shape)
          (8, 16, 16, 256, 256),      # T = 2048: 128 x 128, 32 tiles
          (32, 16, 16, 512, 512),     # T = 8192, N = 512: 128 x 128, 256 tiles
          (4, 24, 40, 64, 96),        # N = 96: 128 x 32 tiles; a non-square, non-power-of-two map
          (3, 8, 8, 128, 64)]         # 128 x 64: two tiles, the last one partial (T = 192)
SPLIT6_TILE_256 = dict(zip(SHAPES, (44, 44, 44, 44, 41, 42)))


@pytest.mark.parametrize("windowed,shift,scaled", [(1, 0, False), (1, 4, True), (1, 3, True), (0, 0, True), (0, 0, False)])
@pytest.mark.parametrize("B,H,W,K,N", SHAPES)
def test_residual_epilogue_vs_fp64(B, H, W, K, N, windowed, shift, scaled):
    from dehaze_hip import _lib, ops
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    T = B * H * W
    g = torch.Generator().manual_seed(T + K + N + shift)
    x = torch.randn(T, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    res = torch.randn(T, N, generator=g).to(dev)
    sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(B)]).to(dev) if scaled else None   # DropPath: 0 or 1 / keep
    y64 = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    f = sc.double().repeat_interleave(H * W)[:, None] if scaled else 1.0
    if windowed:
        ref = res.double() + _window_reverse_roll(f * y64, B, H, W, shift)
        mag = _window_reverse_roll(f * mag, B, H, W, shift) + res.double().abs()
    else:
        ref = res.double() + f * y64
        mag = f * mag + res.double().abs()
    hi, mid, lo = ops.split_planes(w)
    lib = _lib.load()
    if lib.dhz_grid_cus() + lib.dhz_get_reserved_cus() == 256:             # the instance comments over SHAPES hold for 256 CUs
        assert lib.dhz_linear_split6_tile(1, T, N, K) == SPLIT6_TILE_256[(B, H, W, K, N)]
    out = torch.full((T, N), float("nan"), device=dev)
    _lib.call("dhz_linear_fwd_split6_res", x.data_ptr(), K, hi.data_ptr(), mid.data_ptr(), lo.data_ptr(), b.data_ptr(), res.data_ptr(),
              sc.data_ptr() if scaled else None, out.data_ptr(), N, T, N, K, H * W, H, W, shift, windowed, s)
    err = (out.double() - ref).abs()
    assert torch.isfinite(out).all()
    assert (err <= BOUND6 * mag + 1e-7).all(), (err / mag).max().item()
    # dropped images return the shortcut bit for bit
    if scaled:
        rows = torch.arange(T, device=dev).view(B, H * W)[1]
        assert torch.equal(out[rows], res[rows])
    if K % 64 == 0 and N % 64 == 0:
        out2 = torch.full((T, N), float("nan"), device=dev)
        _lib.call("dhz_linear_fwd_split_res", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), res.data_ptr(), sc.data_ptr() if scaled else None,
                  out2.data_ptr(), N, T, N, K, H * W, H, W, shift, windowed, 6, s)
        err = (out2.double() - ref).abs()
        assert torch.isfinite(out2).all()
        assert (err <= BOUND6 * mag + 1e-7).all(), (err / mag).max().item()


def test_residual_epilogue_equals_the_two_launch_form():
    """the epilogue form against the GEMM + dhz_reverse_residual_fwd pair it replaces, same kernels' products: equal to the last
    fp32 rounding of the final add"""
    from dehaze_hip import ops
    dev = torch.device("cuda:0")
    B, H, W, C = 4, 32, 32, 128
    T = B * H * W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(T, C, generator=g).to(dev)
    w = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev)
    b = torch.randn(C, generator=g).to(dev)
    res = torch.randn(T, C, generator=g).to(dev)
    sc = torch.tensor([1.25, 0.0, 1.25, 1.25]).to(dev)
    old = ops.RES_EPILOGUE
    try:
        ops.RES_EPILOGUE = True
        a = ops.gemm_fwd_res(x, w, b, res, sc, B, H, W, 4, True)
        ops.RES_EPILOGUE = False
        r = ops.gemm_fwd_res(x, w, b, res, sc, B, H, W, 4, True)
    finally:
        ops.RES_EPILOGUE = old
    assert (a - r).abs().max().item() <= 2e-6 * (1.0 + r.abs().max().item())


def test_epilogue_argument_checks():
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    x = torch.zeros(192, 64, device=dev)
    pl = torch.zeros(3, 64 * 64, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(192, 64, device=dev)
    args = lambda hw, Hm, Wm, sh: (x.data_ptr(), 64, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), None, out.data_ptr(), None,
                                   out.data_ptr(), 64, 192, 64, 64, hw, Hm, Wm, sh, 1, None)
    for bad in ((60, 6, 10, 0), (64, 8, 8, 9), (64, 4, 16, 0), (128, 8, 16, 0)):       # HW % 64, shift range, H % 8, T % HW
        with pytest.raises(_lib.DehazeHipError):
            _lib.call("dhz_linear_fwd_split6_res", *args(*bad))


@pytest.mark.parametrize("T,N,K,rows", [(8192, 256, 256, 1024), (32768, 128, 128, 4096), (2048, 512, 512, 64), (4096, 64, 64, 1024)])
def test_scaled_dgrad_vs_fp64(T, N, K, rows):
    """dx = scale[image] * (dy . W): ops.gemm_dgrad(row_scale=...) on every route (the forward kernel on the planes of W^T, the few-tile
    kernel, the extra-pass fallback)"""
    from dehaze_hip import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(T + N)
    dy = torch.randn(T, N, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / N ** 0.5).to(dev)
    sc = (0.5 + torch.rand(T // rows, generator=g)).to(dev)
    sc[0] = 0.0
    dx = ops.gemm_dgrad(dy, w, (sc, rows))
    f = sc.double().repeat_interleave(rows)[:, None]
    ref = f * (dy.double() @ w.double())
    mag = f * (dy.double().abs() @ w.double().abs())
    err = (dx.double() - ref).abs()
    assert (err <= BOUND6 * mag + 1e-7).all(), (err / (mag + 1e-30)).max().item()


@pytest.mark.parametrize("C", [64, 128, 512])
@pytest.mark.parametrize("shift,dshift", [(0, 4), (4, 0)])
def test_ln_backward_layouts(C, shift, dshift):
    """dhz_ln_partition_bwd_lay: (a) dx written in the window order of dshift == the plain call followed by the partition permutation;
    (b) dres read in the call's own window order == the plain call on the un-permuted dres."""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    B, H, W = 3, 16, 24
    T = B * H * W
    g = torch.Generator().manual_seed(C + shift)
    x = torch.randn(T, C, generator=g).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).to(dev)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev)
    xn = torch.empty_like(x)
    stats = torch.empty(T, 2, device=dev)
    dy = torch.randn(T, C, generator=g).to(dev)
    dres = torch.randn(T, C, generator=g).to(dev)

    def perm(t, sh):        # token order -> window order of shift sh (roll(-sh) + window_partition, M1:846-852)
        m = t.view(B, H, W, C)
        if sh:
            m = torch.roll(m, shifts=(-sh, -sh), dims=(1, 2))
        return m.view(B, H // 8, 8, W // 8, 8, C).permute(0, 1, 3, 2, 4, 5).reshape(T, C).contiguous()

    def run(part, sh, dresw, dxw, dxs, dres_t):
        dx = torch.empty_like(x)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        _lib.call("dhz_ln_partition_bwd_lay", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), stats.data_ptr(), dres_t.data_ptr(), dx.data_ptr(),
                  dg.data_ptr(), db.data_ptr(), B, H, W, C, sh, part, dresw, dxw, dxs, 0, s)
        return dx, dg, db

    for part, sh in ((0, 0), (1, shift)):
        _lib.call("dhz_ln_partition_fwd_dt", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), xn.data_ptr(), stats.data_ptr(), B, H, W, C, sh,
                  part, 0, s)
        base = run(part, sh, 0, 0, 0, dres)
        a = run(part, sh, 0, 1, dshift, dres)
        assert torch.equal(a[0], perm(base[0], dshift))
        for u, v in ((a[1], base[1]), (a[2], base[2])):                 # d(gamma), d(beta): atomic sums, order varies run to run
            assert torch.allclose(u, v, rtol=1e-4, atol=1e-3)
        if part:
            bres = run(part, sh, 1, 0, 0, perm(dres, sh))
            assert torch.equal(bres[0], base[0])


def _block_grads(use_block, C, heads, res, shift, drop, seed=3):
    import My_model_1 as M1
    from dehaze_hip import fused
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    blk = M1.LeWinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=heads, win_size=8, shift_size=shift, mlp_ratio=4.,
                                   drop_path=drop, token_projection='linear', token_mlp='leff').to(dev)
    blk.train()
    B = 4
    x = torch.randn(B, res * res, C, generator=torch.Generator().manual_seed(seed + 1)).to(dev).requires_grad_(True)
    gy = torch.randn(B, res * res, C, generator=torch.Generator().manual_seed(seed + 2)).to(dev)
    old = fused.BLOCK_NODE
    fused.BLOCK_NODE = use_block
    try:
        torch.manual_seed(99)                 # the ProbSparse sample and the DropPath draws
        y = blk(x)
        y.backward(gy)
    finally:
        fused.BLOCK_NODE = old
    return [y.detach(), x.grad.detach()] + [p.grad.detach() for p in blk.parameters() if p.grad is not None]


@pytest.mark.parametrize("C,heads,res,shift,drop", [(128, 4, 32, 4, 0.3),      # chain forward + chain backward, DropPath live
                                                    (256, 8, 16, 0, 0.0),      # no DropPath factor
                                                    (64, 2, 16, 4, 0.3),       # fused forward, chain backward
                                                    (32, 1, 16, 4, 0.3),       # fused forward AND backward: token-order hand-over stays
                                                    (512, 16, 8, 0, 0.3)])     # single-window map, few-tile kernels
def test_block_node_equals_two_nodes(C, heads, res, shift, drop):
    """fused.block (window-order gradient hand-over, row-factor products) against attn_branch + leff_branch: same forward bits, the
    gradients equal up to the regrouping of the DropPath factor (s * (g . W) against (s * g) . W: one fp32 rounding per product)"""
    a = _block_grads(True, C, heads, res, shift, drop)
    b = _block_grads(False, C, heads, res, shift, drop)
    assert len(a) == len(b)
    assert torch.equal(a[0], b[0])
    for i, (u, v) in enumerate(zip(a[1:], b[1:])):
        tol = 2e-5 * v.abs().max().item() + 1e-7          # (+ absolute floor: d(b_k) is zero in exact arithmetic, ~1e-9 of rounding noise)
        assert (u - v).abs().max().item() <= tol, (i, (u - v).abs().max().item(), tol)

@pytest.mark.parametrize("windowed,shift,scaled", [(1, 4, True), (0, 0, True), (1, 0, False)])
@pytest.mark.parametrize("B,H,W,K,N", [(8, 64, 64, 128, 128),     # 256 x 128 tiles of the software-pipelined kernel
                                       (2, 32, 32, 512, 128),     # few tiles: csrc/linear_bf16.hip's kernel
                                       (4, 16, 24, 64, 64),       # 64-wide output
                                       (3, 8, 8, 128, 192)])      # partial last tile
def test_residual_epilogue_bf16_vs_fp64(B, H, W, K, N, windowed, shift, scaled):
    """config 4's form (dhz_linear_fwd_bf16_res): bf16 operands / shortcut / result, fp32 accumulation; the result is ONE bf16 rounding of
    res + scale (x . w^T + bias) evaluated in fp32"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    T = B * H * W
    g = torch.Generator().manual_seed(T + K + N + shift)
    x = torch.randn(T, K, generator=g).to(dev).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev).bfloat16()
    b = torch.randn(N, generator=g).to(dev)
    res = torch.randn(T, N, generator=g).to(dev).bfloat16()
    sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(B)]).to(dev) if scaled else None
    y64 = x.double() @ w.double().t() + b.double()
    f = sc.double().repeat_interleave(H * W)[:, None] if scaled else 1.0
    ref = res.double() + (_window_reverse_roll(f * y64, B, H, W, shift) if windowed else f * y64)
    out = torch.full((T, N), float("nan"), device=dev, dtype=torch.bfloat16)
    _lib.call("dhz_linear_fwd_bf16_res", x.data_ptr(), K, w.data_ptr(), b.data_ptr(), res.data_ptr(), sc.data_ptr() if scaled else None,
              out.data_ptr(), N, T, N, K, H * W, H, W, shift, windowed, s)
    assert torch.isfinite(out.float()).all()
    err = (out.double() - ref).abs()
    assert (err <= 2.0 ** -8 * ref.abs() + 1e-3).all(), (err / (ref.abs() + 1e-3)).max().item()      # half an ulp of bf16 + fp32 accumulation
    if scaled:
        rows = torch.arange(T, device=dev).view(B, H * W)[1]
        assert torch.equal(out[rows], res[rows])


def test_bf16_block_dual_gradient_copy():
    """bf16 storage (config 4): the LeFF LayerNorm backward writes the scaled, window-ordered gradient copy for the attention branch's
    backward (dhz_ln_partition_bwd_lay2) instead of a dhz_reverse_residual_bwd pass: same gradients up to one bf16 rounding (the copy is
    rounded once from fp32, not from the rounded token-order gradient)."""
    import My_model_1 as M1
    from dehaze_hip import fused
    dev = torch.device("cuda:0")
    res = {}
    for dual in (True, False):
        torch.manual_seed(5)
        blk = M1.LeWinTransformerBlock(dim=128, input_resolution=(32, 32), num_heads=4, win_size=8, shift_size=4, mlp_ratio=4., drop_path=0.3,
                                       token_projection='linear', token_mlp='leff').to(dev).train()
        x = torch.randn(4, 1024, 128, generator=torch.Generator().manual_seed(6)).to(dev).bfloat16().requires_grad_(True)
        gy = torch.randn(4, 1024, 128, generator=torch.Generator().manual_seed(7)).to(dev).bfloat16()
        old = fused.DUAL_BF16
        fused.DUAL_BF16 = dual
        try:
            torch.manual_seed(99)
            y = blk(x)
            y.backward(gy)
        finally:
            fused.DUAL_BF16 = old
        res[dual] = [y.detach().float(), x.grad.detach().float()] + [p.grad.detach().float() for p in blk.parameters() if p.grad is not None]
    assert torch.equal(res[True][0], res[False][0])
    for i, (u, v) in enumerate(zip(res[True][1:], res[False][1:])):
        # bf16 has 8 significant bits: one rounding more or less per element of the hand-over is 2^-9 relative per element
        # (absolute floors: d(b_k) is zero in exact arithmetic - bf16 rounding noise of ~1e-4 against gradients of O(1))
        assert (u - v).abs().max().item() <= 5e-2 * v.abs().max().item() + 1e-3, (i, (u - v).abs().max().item(), v.abs().max().item())
        assert (u - v).abs().mean().item() <= 1e-2 * v.abs().mean().item() + 1e-4, i


@pytest.mark.parametrize("C,heads,res", [(32, 1, 32), (64, 2, 32), (128, 4, 16)])
@pytest.mark.parametrize("shift", [0, 4])
def test_fused_attention_six_term_equals_fp32_pipe(C, heads, res, shift):
    """the fused window-attention forward with its weight products as six-term bf16-pipe products (dhz_fused_window_attn_fwd6: LDS-DMA planes
    at C = 64 / 128, register-resident planes at C = 32) against the fp32-pipe form of the same kernel: outputs and gradients equal to fp32
    rounding, except where a near-tie of the sparsity measure flips a selection (a handful of tokens at most)"""
    import My_model_1 as M1
    from dehaze_hip import fused
    dev = torch.device("cuda:0")
    out = {}
    saved = (fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C)
    try:
        for p6 in (False, True):
            fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C = p6, (32, 64, 128)
            torch.manual_seed(C + shift)
            blk = M1.LeWinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=heads, win_size=8, shift_size=shift, mlp_ratio=4.,
                                           drop_path=0.2, token_projection='linear', token_mlp='leff').to(dev).train()
            x = torch.randn(4, res * res, C, generator=torch.Generator().manual_seed(1)).to(dev).requires_grad_(True)
            gy = torch.randn(4, res * res, C, generator=torch.Generator().manual_seed(2)).to(dev)
            idx = torch.randint(64, (64, 25), generator=torch.Generator().manual_seed(3)).to(torch.uint8).to(dev)
            mask = blk._shift_mask(res, res, dev) if shift else None
            sc = torch.tensor([1.25, 0.0, 1.25, 1.25], device=dev)
            y = fused.fused_attn_branch(x, blk.norm1, blk.attn.ProbSpare, blk.attn.relative_position_bias_table, idx, mask, sc, res, res, shift, heads)
            y.backward(gy)
            with torch.no_grad():
                ye = fused.fused_attn_branch(x.detach(), blk.norm1, blk.attn.ProbSpare, blk.attn.relative_position_bias_table, idx, mask, None, res, res,
                                             shift, heads)
            out[p6] = [y.detach(), ye, x.grad.detach()] + [p.grad.detach() for p in blk.attn.ProbSpare.parameters() if p.grad is not None]
    finally:
        fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C = saved
    assert len(out[True]) == len(out[False]) > 5
    for i, (u, v) in enumerate(zip(out[True], out[False])):
        d = (u - v).abs()
        scale = max(v.abs().max().item(), 1e-3)
        assert d.mean().item() <= 2e-6 * scale + 1e-7, (i, d.mean().item(), scale)   # (+ floor: d(b_k) is zero in exact arithmetic, ~1e-9 of noise)
        assert (d > 1e-4 * scale).float().mean().item() <= 2e-3, (i, (d > 1e-4 * scale).float().mean().item())
