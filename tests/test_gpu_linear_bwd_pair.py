"""-m gpu: dx, dW and db of a token Linear from one pass over dy (dhz_linear_bwd_pair, csrc/linear_bwd_pair.hip) against float64, against the
two launches it replaces (ops.gemm_dgrad + the weight-gradient launch of ops.linear_wgrad), over the CU reservation levels of tests/_grid.py,
and through fused.leff_branch / fused.attn_branch with the planes of a FlatAdamW.

Bounds (the project's own, none of them measured on this kernel; mag = the reference computed over absolute values):
  dx     the six-term bound S6_BOUND * mag + S6_FLOOR of tests/_tile_cases.py (2^-21 sum |dy||W| + 1e-7);
  dW/db  the reordering bound of tests/test_gpu_persistent.py, RED * mag + 1e-5 against float64 and RED * mag + 1e-6 between grids;
  chain  the two-launch chain has the same bounds, except that its dx comes from the fp32 pipe at K = 32: 2^-19 * mag (BOUND_F32 of
         tests/test_gpu_leff_bwd_dz.py); pair and chain may differ by the sum of both bounds;
  branch through a whole branch the switch moves d(xn) and the weight gradients of one Linear by those amounts, and d(xn) passes the
         LayerNorm backward: the branch-level tolerance of tests/test_gpu_leff_bwd_dz.py::test_through_leff_branch, 3e-5 + 3e-5 max |ref|
         (times sqrt(T) for sums over all tokens), taken against the switch-off result."""
import contextlib
import copy
import ctypes
import functools
import math

import pytest
import torch

from _grid import LEVELS, assert_trips, reserved_grid
from _tile_cases import S6_BOUND, S6_FLOOR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RED = 2.0 ** -18
BOUND_F32 = 2.0 ** -19
INSTANCES = [(1, 128, 32), (1, 256, 64), (3, 64, 64)]          # (nmat, nper, K): linear1 at C = 32 / 64, Q / K / V at C = 64


def _s():
    return torch.cuda.current_stream().cuda_stream


def _arr(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]), ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _case(nmat, nper, K, T, pad=0):
    """inputs (dy as a column block of a tensor `pad` columns wider), the planes of W^T, and the float64 references with their magnitudes"""
    from dehaze_hip import _lib
    N = nmat * nper
    g = torch.Generator().manual_seed(7 * N + K + T + pad)
    wide = torch.randn(T, N + pad, generator=g).to(DEV)
    d = dict(nmat=nmat, nper=nper, N=N, K=K, T=T, wide=wide, off=pad // 2)
    d["dy"] = wide[:, d["off"]: d["off"] + N]
    d["x"] = torch.randn(T, K, generator=g).to(DEV)
    d["W"] = (torch.randn(N, K, generator=g) / math.sqrt(N)).to(DEV)
    wt = d["W"].t().contiguous()
    pl = torch.empty((3, wt.numel()), device=DEV, dtype=torch.bfloat16)
    _lib.call("dhz_split3_planes", wt.data_ptr(), wt.numel(), pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _s())
    d["planes"] = pl
    dy, x, W = d["dy"].double(), d["x"].double(), d["W"].double()
    d["ref"] = (dy @ W, dy.t() @ x, dy.sum(0))
    d["mag"] = (dy.abs() @ W.abs(), dy.abs().t() @ x.abs(), dy.abs().sum(0))
    return d


def _targets(d, start):
    """(dW [nmat, nper, K], db [nmat, nper]) zeroed, or filled with a known non-zero pattern"""
    dw = torch.zeros(d["nmat"], d["nper"], d["K"], device=DEV)
    db = torch.zeros(d["nmat"], d["nper"], device=DEV)
    if start:
        dw += torch.linspace(-2.0, 3.0, dw.numel(), device=DEV).view_as(dw)
        db += torch.linspace(5.0, -1.0, db.numel(), device=DEV).view_as(db)
    return dw, db


def _run_pair(d, start=False, db_null=()):
    """db_null: indices of matrices whose db pointer is null, or None for a null table"""
    from dehaze_hip import _lib
    dw, db = _targets(d, start)
    dx = torch.full((d["T"], d["K"]), float("nan"), device=DEV)
    pl = d["planes"]
    dbs = None if db_null is None else _arr([None if m in db_null else db[m] for m in range(d["nmat"])])
    _lib.call("dhz_linear_bwd_pair", d["dy"].data_ptr(), d["wide"].stride(0), d["x"].data_ptr(), d["K"], pl[0].data_ptr(), pl[1].data_ptr(),
              pl[2].data_ptr(), dx.data_ptr(), d["T"], d["nmat"], d["nper"], d["K"], _arr([dw[m] for m in range(d["nmat"])]), dbs, _s())
    torch.cuda.synchronize()
    return dx, dw.view(d["N"], d["K"]), db.view(d["N"])


def _run_chain(d, start=False):
    from dehaze_hip import ops
    dw, db = _targets(d, start)
    dx = ops.gemm_dgrad(d["dy"], d["W"])
    ops._wgrad_launch(d["wide"], d["off"], d["x"], [(d["nper"], dw[m], db[m]) for m in range(d["nmat"])], None)
    torch.cuda.synchronize()
    return dx, dw.view(d["N"], d["K"]), db.view(d["N"])


def _bounds(d, dx_bound=S6_BOUND, floor=1e-5):
    return (dx_bound * d["mag"][0] + S6_FLOOR, RED * d["mag"][1] + floor, RED * d["mag"][2] + floor)


def _check(tag, got, d, dx_bound=S6_BOUND, start=False, db_live=None):
    assert torch.isfinite(got[0]).all(), (tag, "dx was not written in full")
    t0 = _targets(d, start)
    base = (0.0, t0[0].view(d["N"], d["K"]).double(), t0[1].view(d["N"]).double())
    bounds = _bounds(d, dx_bound)
    for k, name in enumerate(("dx", "dW", "db")):
        ref = d["ref"][k] + base[k]
        if name == "db" and db_live is not None:
            ref = torch.where(db_live, ref, base[k])
        e = (got[k].double() - ref).abs()
        print(tag, name, "max err / bound", (e / bounds[k]).max().item())
        assert (e <= bounds[k]).all(), (tag, name, (e / bounds[k]).max().item())
    return bounds


@pytest.mark.parametrize("nmat,nper,K", INSTANCES)
@pytest.mark.parametrize("T", [32, 32 * 12])
def test_vs_fp64_and_chain(nmat, nper, K, T):
    """T = 32: one stage, every workgroup but one idle (the chain's six-term kernels take tokens in 64s: pair alone); 12 stages: slabs of
    one stage on a grid below the CU count, against the chain"""
    from dehaze_hip import _lib
    d = _case(nmat, nper, K, T)
    assert _lib.load().dhz_linear_bwd_pair_grid(T, d["N"], K) == T // 32
    pair = _run_pair(d)
    if T % 64:
        _check("pair", pair, d)
        return
    chain = _run_chain(d)
    f32_dx = BOUND_F32 if K == 32 else S6_BOUND
    bp, bc = _check("pair", pair, d), _check("chain", chain, d, f32_dx)
    for k, name in enumerate(("dx", "dW", "db")):
        e = (pair[k].double() - chain[k].double()).abs()
        assert (e <= bp[k] + bc[k]).all(), (name, (e / (bp[k] + bc[k])).max().item())


@pytest.mark.parametrize("nmat,nper,K", INSTANCES)
def test_multi_trip(nmat, nper, K):
    """every reservation level with T = 32 (3 grid + 1): three trips and a ragged last slab; and one problem on all three grids"""
    from dehaze_hip import _lib
    lib = _lib.load()
    N = nmat * nper
    T_of, res = {}, {}
    for lvl in LEVELS:
        with reserved_grid(lvl) as ncu:
            grid = lib.dhz_linear_bwd_pair_grid(32 * 8 * ncu, N, K)
            assert grid == ncu
            T_of[lvl] = T = 32 * (3 * grid + 1)
            assert lib.dhz_linear_bwd_pair_grid(T, N, K) == grid
            assert_trips("linear backward pair", T // 32, grid)
            d = _case(nmat, nper, K, T)
            _check(f"level {lvl}", _run_pair(d), d)
    d = _case(nmat, nper, K, T_of[8])
    for lvl in LEVELS:
        with reserved_grid(lvl):
            res[lvl] = _run_pair(d)
    for lvl in LEVELS[1:]:
        assert torch.equal(res[lvl][0], res[None][0]), (lvl, "dx depends on the grid")
        for k, name in ((1, "dW"), (2, "db")):
            e = (res[lvl][k].double() - res[None][k].double()).abs()
            assert (e <= RED * d["mag"][k] + 1e-6).all(), (lvl, name)


@pytest.mark.parametrize("nmat,nper,K", INSTANCES)
def test_dy_as_a_column_block_of_a_wider_tensor(nmat, nper, K):
    d = _case(nmat, nper, K, 32 * 6, pad=64)
    assert d["wide"].stride(0) == d["N"] + 64 and d["off"] == 32
    pair, chain = _run_pair(d), _run_chain(d)
    bp = _check("pair, ldy > N", pair, d)
    bc = _check("chain, ldy > N", chain, d, BOUND_F32 if K == 32 else S6_BOUND)
    for k, name in enumerate(("dx", "dW", "db")):
        e = (pair[k].double() - chain[k].double()).abs()
        assert (e <= bp[k] + bc[k]).all(), (name, (e / (bp[k] + bc[k])).max().item())


@pytest.mark.parametrize("nmat,nper,K,db_null", [(1, 256, 64, None), (1, 128, 32, (0,)), (3, 64, 64, (1,)), (3, 64, 64, None)])
def test_null_db(nmat, nper, K, db_null):
    d = _case(nmat, nper, K, 32 * 5)
    live = torch.ones(d["N"], dtype=torch.bool, device=DEV)
    for m in (range(nmat) if db_null is None else db_null):
        live[m * nper: (m + 1) * nper] = False
    got = _run_pair(d, start=True, db_null=db_null)
    _check("null db", got, d, start=True, db_live=live)
    untouched = _targets(d, True)[1].view(-1)
    assert torch.equal(got[2][~live], untouched[~live])


@pytest.mark.parametrize("nmat,nper,K", INSTANCES)
def test_accumulates_onto_nonzero_targets(nmat, nper, K):
    d = _case(nmat, nper, K, 32 * 5)
    _check("accumulate", _run_pair(d, start=True), d, start=True)


# ---- through the branches
def _scale(B):
    sc = torch.ones(B)
    sc[-1] = 1.0 / 0.7
    return sc


@contextlib.contextmanager
def _switch(on):
    from dehaze_hip import ops
    saved = (ops.LINEAR_BWD_PAIR, ops.LINEAR_BWD_PAIR_SHAPES)
    try:
        ops.LINEAR_BWD_PAIR, ops.LINEAR_BWD_PAIR_SHAPES = on, ops.LINEAR_BWD_PAIR_BUILT
        yield
    finally:
        ops.LINEAR_BWD_PAIR, ops.LINEAR_BWD_PAIR_SHAPES = saved


def _branch_run(kind, net, x, gout, on, deterministic=False):
    """gradients of one branch (fresh copy of the module, a FlatAdamW's planes) and the names of the library calls of its backward"""
    from dehaze_hip import _lib, fused, ops
    from dehaze_hip.train import FlatAdamW
    B, H, W, C = 2, 16, 16, 64
    saved = (ops.SPLIT_SHADOW, ops.SHADOW_OWNER, _lib.call)
    names = []

    def spy(name, *args):
        names.append(name)
        return saved[2](name, *args)

    nd = copy.deepcopy(net).to(DEV)
    opt = FlatAdamW(nd)
    try:
        if deterministic:
            ops.set_deterministic(True, None)
            ops._stream()
        with _switch(on):
            opt.zero_grad()
            opt.enable_split_shadow()
            xd = x.to(DEV).requires_grad_()
            sc = _scale(B).to(DEV)
            if kind == "leff":
                assert ops.split_planes_t(nd["mlp"].linear1[0].weight) is not None
                y = fused.leff_branch(xd, nd["norm"], nd["mlp"], sc, H, W)
            else:
                blk = nd["blk"]
                idx = torch.randint(64, (64, 25), generator=torch.Generator().manual_seed(3)).to(torch.uint8).to(DEV)
                y = fused.attn_branch(xd, blk.norm1, blk.attn.ProbSpare, blk.attn.relative_position_bias_table, idx, None, sc, H, W, 0, C // 32)
            _lib.call = spy
            (y * gout.to(DEV)).sum().backward()
            _lib.call = saved[2]
            torch.cuda.synchronize()
        out = {"dx": xd.grad.clone()}
        out.update({n_: p.grad.clone() for n_, p in nd.named_parameters() if p.grad is not None})
        return out, names
    finally:
        _lib.call = saved[2]
        if deterministic:
            ops.set_deterministic(False)
        ops.SPLIT_SHADOW, ops.SHADOW_OWNER = saved[0], saved[1]


@functools.lru_cache(maxsize=None)
def _branch_net(kind):
    import My_model_1 as M1
    C, H = 64, 16
    torch.manual_seed(11 if kind == "leff" else 12)
    if kind == "leff":
        net = torch.nn.ModuleDict({"norm": torch.nn.LayerNorm(C), "mlp": M1.LeFF(C, 4 * C)})
    else:
        net = torch.nn.ModuleDict({"blk": M1.LeWinTransformerBlock(dim=C, input_resolution=(H, H), num_heads=C // 32, win_size=8, shift_size=0,
                                                                   mlp_ratio=4., drop_path=0.2, token_projection='linear', token_mlp='leff')})
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return net, torch.randn(2, H * H, C), torch.randn(2, H * H, C)


@pytest.mark.parametrize("kind", ["leff", "attn"])
def test_through_branch_switch_on_against_off(kind):
    net, x, gout = _branch_net(kind)
    (on, on_names), (off, off_names) = _branch_run(kind, net, x, gout, True), _branch_run(kind, net, x, gout, False)
    assert on_names.count("dhz_linear_bwd_pair") == 1 and "dhz_linear_bwd_pair" not in off_names
    # the one kernel stands for two launches: a token-Linear product and a weight gradient
    extra = sorted(off_names)
    for n in on_names:
        if n != "dhz_linear_bwd_pair":
            extra.remove(n)
    assert len(extra) == 2 and all(n.startswith("dhz_linear_") for n in extra) and sum("wgrad" in n for n in extra) == 1, extra
    assert set(on) == set(off) and len(on) >= 9
    T = x.shape[0] * x.shape[1]
    for k, r in off.items():
        tol = 3e-5 + 3e-5 * r.abs().max().item()
        if k != "dx":
            tol *= T ** 0.5
        e = (on[k] - r).abs().max().item()
        print(kind, k, e, tol)
        assert e <= tol, (kind, k, e, tol)


@pytest.mark.parametrize("kind", ["leff", "attn"])
def test_deterministic_mode_takes_the_chain(kind):
    net, x, gout = _branch_net(kind)
    (a, names), (b, _) = _branch_run(kind, net, x, gout, True, True), _branch_run(kind, net, x, gout, True, True)
    assert "dhz_linear_bwd_pair" not in names
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
