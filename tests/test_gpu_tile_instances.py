"""-m gpu: every tile instance of csrc/conv_gemm.hip (dhz_conv4s2_fwd / _dgrad / _wgrad) and csrc/linear_gemm.hip (dhz_linear_fwd /
_dgrad) against float64, through the raw C-ABI.

Both files pick their instance <WM, WN> from the problem size and the CU count, and on the whole device every small problem gets the
smallest tiles on one trip of the persistent loop.  The cases of tests/_tile_cases.py run at the three levels of tests/_grid.py (whole
device, grids sized for 8 and for 9 CUs); at the reserved levels they select every reachable instance and make two or three trips, so
the carry between tiles (the next tile's prefetch inside the last stage of the previous one, the double-buffer parity, the re-zeroed
accumulators), the XCD remap and the ragged last row tile are compared by value.  Which instance ran is asked of the library
(dhz_conv4s2_tile, dhz_linear_tile: the function the dispatch calls) and, at the reserved levels, is what the table claims
(tests/test_tile_instances_host.py proves the tables complete without a GPU).

Reference: float64 on the device, plain indexing and matmul (no library convolution):
    y = sum_(ky,kx) xpad[:, ky:ky+2Ho:2, kx:kx+2Wo:2, :] @ w[:, :, ky, kx]^T + b
`mag` is the same expression over absolute values; gradients and their magnitudes are the autograd of the two expressions.
Bounds, on every element: forward, backward-data and GEMM |err| <= 2^-19 mag + 1e-6 (the fp32 line of
test_gpu_persistent.py::test_gemm_forward_and_dgrad_multi_trip, here at contractions up to 2048); weight gradient and db
|err| <= 2^-18 mag + 1e-5 (test_wgrad_multi_trip).  Outputs are NaN before every call, 64 guard rows behind each stay NaN, and the
padding columns of strided operands are NaN on the input side too.  Un-reduced outputs of two levels that ran the same instance are
bit-equal; reduced ones (dw, db) agree within 2^-18 mag + 1e-6.  Each case prints its worst err / bound share per level
(profiles/tile_instances.txt).
"""
import pytest
import torch
import torch.nn.functional as F

from _grid import LEVELS, reserved_grid
import _tile_cases as TC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
EINVAL = -22
GUARD = 64
FWD, FWD_FLOOR = 2.0 ** -19, 1e-6
RED, RED_FLOOR, RED_FLOOR_LEVELS = 2.0 ** -18, 1e-5, 1e-6


def _s():
    return torch.cuda.current_stream().cuda_stream


def _share(got, ref, mag, rel, floor):
    """worst |err| / bound over all elements; NaN (an element never written) counts as infinite"""
    err = (got.double() - ref).abs()
    share = (err / (rel * mag + floor)).max().item()
    return share if share == share else float("inf")


def _guarded(rows, cols, ld=None, fill=NAN):
    """[rows + GUARD, ld] of NaN whose first `rows` x `cols` block is `fill`"""
    t = torch.full((rows + GUARD, ld or cols), NAN, device=DEV)
    if fill == fill:
        t[:rows, :cols] = fill
    return t


def _untouched(t, rows, cols):
    return bool(torch.isnan(t[rows:]).all() and torch.isnan(t[:rows, cols:]).all())


def _strided(t, ld):
    """t [rows, cols] in a [rows, ld] buffer whose padding columns are NaN"""
    buf = torch.full((t.shape[0], ld), NAN, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf


def _check_levels(name, res, tiles):
    """res[lvl] = un-reduced output, tiles[lvl] = the instance that wrote it: bit-equal wherever two levels ran the same instance"""
    for i, a in enumerate(LEVELS):
        for b in LEVELS[i + 1:]:
            if tiles[a] == tiles[b]:
                assert torch.equal(res[a], res[b]), (name, a, b, tiles[a])


# ----------------------------------------------------------------------------------------------------------------------------------
def _conv_expr(x4, w, b):
    """x4 [B,H,W,Cin], w [Cout,Cin,4,4], b [Cout] -> [B, Ho*Wo, Cout]: the 4x4 / stride-2 / pad-1 convolution, tap by tap"""
    B, H, W, _ = x4.shape
    Ho, Wo = H // 2, W // 2
    xp = F.pad(x4, (0, 0, 1, 1, 1, 1))
    y = b
    for ky in range(4):
        for kx in range(4):
            y = y + xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2, :] @ w[:, :, ky, kx].t()
    return y.reshape(B, Ho * Wo, -1)


def _conv_case(B, H, W, Cin, Cout, seed):
    """inputs on the device and the float64 reference of every output with its magnitude"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, H * W, Cin, generator=g, device=DEV)
    w = torch.randn(Cout, Cin, 4, 4, generator=g, device=DEV) * 0.05
    b = torch.randn(Cout, generator=g, device=DEV) * 0.1
    gy = torch.randn(B, (H // 2) * (W // 2), Cout, generator=g, device=DEV)
    ref = {}
    for key, f in (("val", lambda t: t.double()), ("mag", lambda t: t.double().abs())):
        x64, w64, b64 = (f(t).requires_grad_() for t in (x, w, b))
        y = _conv_expr(x64.view(B, H, W, Cin), w64, b64)
        y.backward(f(gy))
        ref[key] = dict(y=y.detach().reshape(-1, Cout), dx=x64.grad.reshape(-1, Cin),
                        dw=w64.grad.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin), db=b64.grad)
    return x, w, b, gy, ref["val"], ref["mag"]


@pytest.mark.parametrize("Cin,Cout", TC.CONV_PAIRS)
@pytest.mark.parametrize("case", sorted(TC.CONV_MAPS))
def test_conv4s2_fwd_dgrad_every_instance(case, Cin, Cout):
    from dehaze_hip import _lib
    lib = _lib.load()
    B, H, W = TC.CONV_MAPS[case]
    M, T = TC.conv_rows(case), B * H * W
    x, w, b, gy, ref, mag = _conv_case(B, H, W, Cin, Cout, 1000 + 7 * M + Cin)
    wp = w.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).contiguous()
    wq = w.permute(2, 3, 0, 1).contiguous()
    ys, dxs, ty, tdx = {}, {}, {}, {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            ty[lvl] = lib.dhz_conv4s2_tile(1, B, H, W, Cin, Cout)
            tdx[lvl] = lib.dhz_conv4s2_tile(2, B, H, W, Cin, Cout)
            if lvl is not None:
                k = TC.RESERVED.index(lvl)
                for N, got in ((Cout, ty[lvl]), (Cin, tdx[lvl])):
                    if N in TC.CONV_TABLE[case]:
                        assert got == TC.CONV_TABLE[case][N][k][0], (case, N, lvl, got)
                        assert TC.plan(got, M, N, ncu)[2] == TC.CONV_TABLE[case][N][k][1]
            y = _guarded(M, Cout)
            dx = _guarded(T, Cin)
            _lib.call("dhz_conv4s2_fwd", x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), B, H, W, Cin, Cout, _s())
            _lib.call("dhz_conv4s2_dgrad", gy.data_ptr(), wq.data_ptr(), dx.data_ptr(), B, H, W, Cin, Cout, _s())
            torch.cuda.synchronize()
        assert _untouched(y, M, Cout) and _untouched(dx, T, Cin), (lvl, "a guard row was written")
        ys[lvl], dxs[lvl] = y[:M], dx[:T]
        sy = _share(ys[lvl], ref["y"], mag["y"], FWD, FWD_FLOOR)
        sdx = _share(dxs[lvl], ref["dx"], mag["dx"], FWD, FWD_FLOOR)                    # inf where a parity launch left a NaN
        print(f"TILE conv case={case} Cin={Cin} Cout={Cout} level={lvl} fwd={ty[lvl]} share={sy:.3f} dgrad={tdx[lvl]} share={sdx:.3f}")
        assert sy <= 1.0, (lvl, "forward", ty[lvl], sy)
        assert sdx <= 1.0, (lvl, "backward-data", tdx[lvl], sdx)
    _check_levels("y", ys, ty)
    _check_levels("dx", dxs, tdx)


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", TC.GEMM_CASES)
def test_linear_gemm_every_instance(M, N):
    """N output features of the forward (with bias, WT) and of the backward-data (!WT), contraction GEMM_CONTRACTION[N]"""
    from dehaze_hip import _lib
    lib = _lib.load()
    K = TC.GEMM_CONTRACTION[N]
    pad = M in TC.GEMM_PADDED_ROWS
    ld_in, ld_out = (K + 8, N + 4) if pad else (K, N)
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N)
    x = torch.randn(M, K, generator=g, device=DEV)                       # forward: y[M,N] = x w^T + b, w [N,K]
    w = torch.randn(N, K, generator=g, device=DEV) / K ** 0.5
    b = torch.randn(N, generator=g, device=DEV)
    dy = torch.randn(M, K, generator=g, device=DEV)                      # backward-data of a Linear(N -> K): dx[M,N] = dy w2, w2 [K,N]
    w2 = torch.randn(K, N, generator=g, device=DEV) / K ** 0.5
    xs, dys = _strided(x, ld_in), _strided(dy, ld_in)
    ref = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    refd = dy.double() @ w2.double()
    magd = dy.double().abs() @ w2.double().abs()
    ys, dxs, tiles = {}, {}, {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            tiles[lvl] = lib.dhz_linear_tile(M, N)
            if lvl is not None:
                assert tiles[lvl] == TC.GEMM_TABLE[M][N][0], (M, N, lvl, tiles[lvl])
                assert TC.plan(tiles[lvl], M, N, ncu)[2] == TC.GEMM_TABLE[M][N][1]
            y = _guarded(M, N, ld_out)
            dx = _guarded(M, N, ld_out)
            _lib.call("dhz_linear_fwd", xs.data_ptr(), ld_in, w.data_ptr(), b.data_ptr(), y.data_ptr(), ld_out, M, N, K, _s())
            _lib.call("dhz_linear_dgrad", dys.data_ptr(), ld_in, w2.data_ptr(), dx.data_ptr(), ld_out, M, K, N, _s())
            torch.cuda.synchronize()
        assert _untouched(y, M, N) and _untouched(dx, M, N), (lvl, "a guard row or a padding column was written")
        ys[lvl], dxs[lvl] = y[:M, :N], dx[:M, :N]
        sy = _share(ys[lvl], ref, mag, FWD, FWD_FLOOR)
        sdx = _share(dxs[lvl], refd, magd, FWD, FWD_FLOOR)
        rag = int(M % (32 * (tiles[lvl] // 10)) != 0)
        print(f"TILE gemm rows={M} features={N} contraction={K} level={lvl} tile={tiles[lvl]} ragged={rag} fwd share={sy:.3f} "
              f"dgrad share={sdx:.3f}")
        assert sy <= 1.0, (lvl, "forward", tiles[lvl], sy)
        assert sdx <= 1.0, (lvl, "backward-data", tiles[lvl], sdx)
    _check_levels("y", ys, tiles)
    _check_levels("dx", dxs, tiles)


# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", TC.WGRAD_CIN)
@pytest.mark.parametrize("Cout", TC.WGRAD_COUT)
def test_conv4s2_wgrad_every_instance(Cout, Cin):
    from dehaze_hip import _lib
    lib = _lib.load()
    B, H, W = TC.WGRAD_MAP
    x, w, b, gy, ref, mag = _conv_case(B, H, W, Cin, Cout, 5000 + Cout + 3 * Cin)
    K = 16 * Cin
    runs = [True] + ([False] if (Cout, Cin) in TC.WGRAD_NO_DB else [])          # with db, then with db = NULL
    dws, dbs = {}, {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            assert lib.dhz_conv4s2_tile(3, B, H, W, Cin, Cout) == TC.wgrad_instance(Cout, Cin)
            assert TC.wgrad_splits(Cout, Cin, ncu) == (1 if lvl else 3)
            for with_db in runs:
                dw = _guarded(Cout, K, fill=0.0)                                # accumulated outputs: zeros in front of the NaN guard
                db = _guarded(1, Cout, fill=0.0)
                _lib.call("dhz_conv4s2_wgrad", gy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr() if with_db else None,
                          B, H, W, Cin, Cout, _s())
                torch.cuda.synchronize()
                assert _untouched(dw, Cout, K) and _untouched(db, 1, Cout), (lvl, with_db, "a guard row was written")
                sw = _share(dw[:Cout], ref["dw"], mag["dw"], RED, RED_FLOOR)
                assert sw <= 1.0, (lvl, with_db, "dw", sw)
                if with_db:
                    dws[lvl], dbs[lvl] = dw[:Cout], db[0]
                    sb = _share(db[0], ref["db"], mag["db"], RED, RED_FLOOR)
                    print(f"TILE wgrad Cout={Cout} Cin={Cin} level={lvl} tile={TC.wgrad_instance(Cout, Cin)} "
                          f"splits={TC.wgrad_splits(Cout, Cin, ncu)} dw share={sw:.3f} db share={sb:.3f}")
                    assert sb <= 1.0, (lvl, "db", sb)
                else:
                    assert bool((db[0] == 0).all()), (lvl, "db = NULL, yet the bias gradient was written")
    for lvl in LEVELS[1:]:
        assert _share(dws[lvl], dws[None].double(), mag["dw"], RED, RED_FLOOR_LEVELS) <= 1.0, (lvl, "dw across levels")
        assert _share(dbs[lvl], dbs[None].double(), mag["db"], RED, RED_FLOOR_LEVELS) <= 1.0, (lvl, "db across levels")


# ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """a refused shape answers DHZ_EINVAL, its tile query answers 0, and the outputs are still NaN"""
    from dehaze_hip import _lib
    lib = _lib.load()
    B, H, W, Cin, Cout = 2, 12, 20, 32, 64
    x = torch.randn(B, (H + 1) * W, Cin + 16, device=DEV)
    wp = torch.randn(Cout, 16 * (Cin + 16), device=DEV)
    gy = torch.randn(B, H * W, Cout, device=DEV)
    y = torch.full((B * H * W, Cout), NAN, device=DEV)
    dx = torch.full((B * (H + 1) * W, Cin + 16), NAN, device=DEV)
    dw = torch.full((Cout, 16 * (Cin + 16)), NAN, device=DEV)
    for h, cin in ((H + 1, Cin), (H, Cin + 16)):                                # odd H; Cin % 32 != 0
        assert lib.dhz_conv4s2_fwd(x.data_ptr(), wp.data_ptr(), None, y.data_ptr(), B, h, W, cin, Cout, _s()) == EINVAL
        assert lib.dhz_conv4s2_dgrad(gy.data_ptr(), wp.data_ptr(), dx.data_ptr(), B, h, W, cin, Cout, _s()) == EINVAL
        assert lib.dhz_conv4s2_wgrad(gy.data_ptr(), x.data_ptr(), dw.data_ptr(), None, B, h, W, cin, Cout, _s()) == EINVAL
        assert [lib.dhz_conv4s2_tile(m, B, h, W, cin, Cout) for m in (1, 2, 3)] == [0, 0, 0]
    # weight gradient: Ho = 6 is no power of two (forward and backward-data take the map)
    assert lib.dhz_conv4s2_wgrad(gy.data_ptr(), x.data_ptr(), dw.data_ptr(), None, B, H, 32, Cin, Cout, _s()) == EINVAL
    assert [lib.dhz_conv4s2_tile(m, B, H, 32, Cin, Cout) > 0 for m in (1, 2, 3)] == [True, True, False]
    # GEMM: ldy < N
    M, N, K = 100, 64, 32
    a = torch.randn(M, K, device=DEV)
    wl = torch.randn(N, K, device=DEV)
    yl = torch.full((M, N), NAN, device=DEV)
    dxl = torch.full((M, K), NAN, device=DEV)
    assert lib.dhz_linear_fwd(a.data_ptr(), K, wl.data_ptr(), None, yl.data_ptr(), N - 4, M, N, K, _s()) == EINVAL
    assert lib.dhz_linear_dgrad(yl.data_ptr(), N, wl.data_ptr(), dxl.data_ptr(), K - 4, M, N, K, _s()) == EINVAL
    torch.cuda.synchronize()
    for t in (y, dx, dw, yl, dxl):
        assert bool(torch.isnan(t).all())
