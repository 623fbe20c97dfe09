"""-m gpu: the fp32 token-Linear weight gradients with a 16-token tail (T % 32 == 16: `16 * batch` tokens of a 4 x 4 bottleneck at an
odd batch) through the raw C-ABI, against fp64.  Tolerance: the one tests/test_gpu_linear.py uses against fp64, 2e-5 sqrt(T) + 1e-4.

The operands of the canary tests are followed by 32 rows of NaN: a kernel that folds a row at or beyond T into a sum returns NaN."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TAILS = [16, 48, 80, 1040]
# wm = 1, 3, 2, 4 and wn = 1, 2, 4 of csrc/linear_wgrad.hip's dispatch, 256 rows (two row tiles); then the narrow (16-wide) forms
SHAPES = [(32, 32), (96, 64), (64, 128), (128, 128), (256, 32), (16, 48), (48, 16), (16, 16)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def tol(T):
    return 2e-5 * T ** 0.5 + 1e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operands(T, N, K, dev, seed, pad_cols=0, canary=True):
    """dy [T, N] (row stride N + pad_cols), x [T, K] on the device and their fp64 products; canary: 32 rows of NaN behind row T,
    else the operands end where their own exactly-sized allocation ends"""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(T, N + pad_cols, generator=g)
    x = torch.randn(T, K, generator=g)
    ref_w = dy[:, :N].double().t() @ x.double()
    ref_b = dy[:, :N].double().sum(0)
    if canary:
        dyd = torch.full((T + 32, N + pad_cols), float("nan"), device=dev)
        xd = torch.full((T + 32, K), float("nan"), device=dev)
    else:
        dyd, xd = torch.empty(T, N + pad_cols, device=dev), torch.empty(T, K, device=dev)
    dyd[:T].copy_(dy)
    xd[:T].copy_(x)
    return dyd, xd, ref_w, ref_b


def _check(dw, db, ref_w, ref_b, T, what):
    ew = (dw.double().cpu() - ref_w).abs().max().item()
    assert ew < tol(T), (what, "dw", ew)                 # (NaN fails the comparison)
    if db is not None:
        eb = (db.double().cpu() - ref_b).abs().max().item()
        assert eb < tol(T), (what, "db", eb)


def _launch(dyd, xd, T, N, K, dev, bias=True):
    from dehaze_hip import _lib
    dw = torch.zeros(N, K, device=dev)
    db = torch.zeros(N, device=dev) if bias else None
    _lib.call("dhz_linear_wgrad", dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), xd.stride(0), T, N, K, dw.data_ptr(),
              db.data_ptr() if bias else None, _stream())
    return dw, db


# ----------------------------------------------------------------------------- 1. tail vs fp64
@pytest.mark.parametrize("T", TAILS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_wgrad_tail_canary_rows(dev, T, N, K):
    dyd, xd, ref_w, ref_b = _operands(T, N, K, dev, T + 7 * N + K)
    for bias in (True, False):
        dw, db = _launch(dyd, xd, T, N, K, dev, bias)
        _check(dw, db, ref_w, ref_b, T, (T, N, K, bias))
    assert torch.isnan(dyd[T:]).all() and torch.isnan(xd[T:]).all()


def test_wgrad_tail_strided_dy(dev):
    """ldy > N: dy is the first 96 columns of a 128-column buffer"""
    T, N, K = 48, 96, 64
    dyd, xd, ref_w, ref_b = _operands(T, N, K, dev, 5, pad_cols=32)
    assert dyd.stride(0) == N + 32
    dw, db = _launch(dyd, xd, T, N, K, dev)
    _check(dw, db, ref_w, ref_b, T, "ldy")


@pytest.mark.parametrize("T", TAILS)
@pytest.mark.parametrize("N,K", SHAPES)
def test_wgrad_tail_operands_end_at_row_T(dev, T, N, K):
    """the operands are torch.empty(T, .): row T is the end of their allocation, nothing may be read behind them (values only)"""
    dyd, xd, ref_w, ref_b = _operands(T, N, K, dev, T + 3 * N + K, canary=False)
    dw, db = _launch(dyd, xd, T, N, K, dev)
    _check(dw, db, ref_w, ref_b, T, (T, N, K))


# ----------------------------------------------------------------------------- 2. two token groups per workgroup
def test_wgrad_tail_two_group_instance(dev):
    """N = K = 512 (16 tiles of 128 x 128): wgrad_dispatch takes the two-group instance from 8 stages per slab; the smallest
    T = 16 (mod 32) with (T / 32) / (CUs / tiles) >= 8 - 4112 on a full 256-CU part"""
    from dehaze_hip import _lib
    N = K = 512
    tiles = (N // 128) * (K // 128)
    splits2 = max(_lib.load().dhz_grid_cus() // tiles, 1)
    T = 32 * 8 * splits2 + 16
    assert T % 32 == 16 and (T // 32) // splits2 >= 8 and ((T - 32) // 32) // splits2 < 8
    dyd, xd, ref_w, ref_b = _operands(T, N, K, dev, 21)
    dw, db = _launch(dyd, xd, T, N, K, dev)
    _check(dw, db, ref_w, ref_b, T, ("two groups", T))


# ----------------------------------------------------------------------------- 3. multi
def test_wgrad_multi_tail(dev):
    from dehaze_hip import _lib
    T, n, N, K = 48, 3, 32, 32
    dyd, xd, ref_w, ref_b = _operands(T, n * N, K, dev, 31)
    dws = [torch.zeros(N, K, device=dev) for _ in range(n)]
    dbs = [torch.zeros(N, device=dev) for _ in range(n)]
    aw = (ctypes.c_void_p * n)(*[w.data_ptr() for w in dws])
    ab = (ctypes.c_void_p * n)(*[b.data_ptr() for b in dbs])
    _lib.call("dhz_linear_wgrad_multi", dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), K, T, n, N, K, ctypes.cast(aw, ctypes.c_void_p),
              ctypes.cast(ab, ctypes.c_void_p), _stream())
    for i in range(n):
        sw, sb = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        _lib.call("dhz_linear_wgrad", dyd.data_ptr() + 4 * i * N, dyd.stride(0), xd.data_ptr(), K, T, N, K, sw.data_ptr(), sb.data_ptr(),
                  _stream())
        assert (dws[i] - sw).abs().max().item() < tol(T) and (dbs[i] - sb).abs().max().item() < tol(T), i
        _check(dws[i], dbs[i], ref_w[i * N:(i + 1) * N], ref_b[i * N:(i + 1) * N], T, ("multi", i))


# ----------------------------------------------------------------------------- 4. deterministic mode
@pytest.fixture()
def deterministic(dev):
    from dehaze_hip import ops
    torch.zeros(1, device=dev)                            # the GPU is up: set_deterministic allocates the workspace at once
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("T", [48, 1040, 1024])           # 1024: the slab arithmetic for an aligned T (passes before the tail existed)
@pytest.mark.parametrize("N,K", [(96, 64), (16, 48)])
def test_wgrad_tail_deterministic(dev, deterministic, T, N, K):
    dyd, xd, ref_w, ref_b = _operands(T, N, K, dev, T + N)
    dw1, db1 = _launch(dyd, xd, T, N, K, dev)
    dw2, db2 = _launch(dyd, xd, T, N, K, dev)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    _check(dw1, db1, ref_w, ref_b, T, ("deterministic", T, N, K))


# ----------------------------------------------------------------------------- 5. refusals that remain
def test_wgrad_refusals_remain(dev):
    from dehaze_hip import _lib, ops
    lib = _lib.load()
    s = _stream()
    dy, x = torch.zeros(128, 64, device=dev), torch.zeros(128, 64, device=dev)
    dw, db, sc = torch.zeros(64, 64, device=dev), torch.zeros(64, device=dev), torch.ones(8, device=dev)
    for T in (100, 8):
        assert lib.dhz_linear_wgrad(dy.data_ptr(), 64, x.data_ptr(), 64, T, 64, 64, dw.data_ptr(), db.data_ptr(), s) == -22
        assert b"multiple of 16" in lib.dhz_last_error()
    assert lib.dhz_linear_wgrad_rs(dy.data_ptr(), 64, x.data_ptr(), 64, 128, 64, 64, dw.data_ptr(), db.data_ptr(), sc.data_ptr(), 16, s) == -22
    assert b"rows_per_scale" in lib.dhz_last_error()
    assert not dw.any() and not db.any()
    W = torch.nn.Parameter(torch.zeros(64, 64, device=dev))
    b = torch.nn.Parameter(torch.zeros(64, device=dev))
    with pytest.raises(RuntimeError, match="T in 64s"):
        ops.linear_wgrad(torch.zeros(48, 64, device=dev, dtype=torch.bfloat16), 0, torch.zeros(48, 64, device=dev, dtype=torch.bfloat16),
                         [(W, b)])
