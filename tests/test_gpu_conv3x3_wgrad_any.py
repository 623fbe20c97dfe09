"""-m gpu: dhz_conv3x3_wgrad_any - the dense 3x3 weight and bias gradient on maps of any size (csrc/conv3x3_wgrad.hip, the ragged
instance: ceil(H / 4) x ceil(W / 16) chunks per image, dy positions outside the map zeros in LDS) - against float64
torch.nn.grad.conv2d_weight and the float64 sum of dy on the CPU.  Bounds: those of tests/test_gpu_conv3x3_wgrad.py:81-82, T = B H W.

Shapes (B, Cin, Kout, H, W): one partly filled chunk (5 x 7); a last chunk row of 2 rows and a last chunk column of 4 (18 x 20); ragged
in one axis only, each way (16 x 24, 22 x 32); FFA-Net's channels on 38 x 52 with 3 x 10 x 4 = 120 chunks - several slabs of several
chunks, asserted from the parts query; a small map that is not the packed 8 x 8 case (12 x 12).
Every input map has 64 NaN floats behind it in its allocation (a read past a map would put NaN into the sums); dw, db and the floats behind
the queried workspace start as NaN.  On shapes the old entry takes the `_any` entry and its queries give the same bits and numbers."""
import pytest
import torch

from _grid import LEVELS, reserved_grid

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32, 5, 7), (2, 32, 64, 18, 20), (1, 32, 32, 16, 24), (1, 32, 32, 22, 32), (3, 64, 64, 38, 52), (2, 32, 32, 12, 12)]
MANY = (3, 64, 64, 38, 52)
REGULAR = [(2, 32, 64, 16, 32), (3, 64, 32, 8, 8)]
CANARY = 4096            # floats of NaN behind the queried workspace
TAIL = 64                # floats of NaN behind each input map


def blocked(t):
    """[B, C, H, W] -> the kernels' [B, C/8, H, W, 8]"""
    B, C, H, W = t.shape
    return t.view(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def with_tail(t):
    """t on the device with TAIL NaN floats behind it in the same allocation; returns (view, whole buffer)"""
    buf = torch.full((t.numel() + TAIL,), float("nan"), device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf[:t.numel()].view(t.shape), buf


_CASES = {}


def case(shape):
    """inputs and the float64 reference of one shape, computed once and shared (never modified)"""
    if shape not in _CASES:
        B, Cin, Kout, H, W = shape
        g = torch.Generator().manual_seed(2000 + B + Cin + Kout + 3 * H + 7 * W)
        x = torch.randn(B, Cin, H, W, generator=g)
        dy = torch.randn(B, Kout, H, W, generator=g)
        dw = torch.nn.grad.conv2d_weight(x.double(), (Kout, Cin, 3, 3), dy.double(), stride=1, padding=1)
        db = dy.double().sum((0, 2, 3))
        _CASES[shape] = (with_tail(blocked(x)), with_tail(blocked(dy)), dw, db)
    (xb, xbuf), (dyb, dybuf), dw, db = _CASES[shape]
    assert torch.isnan(xbuf[-TAIL:]).all() and torch.isnan(dybuf[-TAIL:]).all()
    return xb, dyb, dw, db


def run(shape, xb, dyb, with_db=True, ws=None, entry="dhz_conv3x3_wgrad_any"):
    """one call with NaN canaries in the outputs and behind the workspace; returns (dw, db) on the device"""
    from dehaze_hip import _lib
    B, Cin, Kout, H, W = shape
    lib = _lib.load()
    if entry == "dhz_conv3x3_wgrad_any":
        need = lib.dhz_conv3x3_wgrad_workspace_bytes_any(B, H, W, Cin, Kout)
    else:
        need = lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout)
    assert need > 0 and need % 4 == 0
    if ws is None:
        ws = torch.full((need // 4 + CANARY,), float("nan"), device="cuda")
    dw = torch.full((Kout, Cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((Kout,), float("nan"), device="cuda")
    _lib.call(entry, xb.data_ptr(), dyb.data_ptr(), dw.data_ptr(), db.data_ptr() if with_db else None, ws.data_ptr(), need, B, H, W, Cin,
              Kout, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(ws[need // 4:]).all(), "the kernel wrote behind the queried workspace"
    return dw, db


@pytest.mark.parametrize("shape", SHAPES)
def test_conv3x3_wgrad_any_matches_float64(shape):
    B, Cin, Kout, H, W = shape
    xb, dyb, dwref, dbref = case(shape)
    dw, db = run(shape, xb, dyb)
    T = B * H * W
    edw = (dw.cpu().double() - dwref).abs().max().item()
    edb = (db.cpu().double() - dbref).abs().max().item()
    bdw = 3e-6 * T ** 0.5 * max(1.0, dwref.abs().max().item() / T ** 0.5) + 1e-4
    bdb = 3e-5 * T ** 0.5 + 1e-4
    print(f"conv3x3_wgrad_any {shape}: dW error {edw:.3e} (bound {bdw:.3e}), db error {edb:.3e} (bound {bdb:.3e})")
    assert edw < bdw                                   # a NaN (a read past a map, an element not written) fails these too
    assert edb < bdb
    # db == NULL leaves dW bit-equal (and db untouched)
    dw2, db2 = run(shape, xb, dyb, with_db=False)
    assert torch.equal(dw2, dw)
    assert torch.isnan(db2).all()


def test_conv3x3_wgrad_any_cut_has_slabs_and_chunks():
    """(3, 64, 64, 38, 52): 3 x ceil(38 / 4) x ceil(52 / 16) = 120 chunks in min(ceil(512 / 4), 120 / 4) = 30 slabs of 4 chunks"""
    from dehaze_hip import _lib
    lib = _lib.load()
    B, Cin, Kout, H, W = MANY
    chunks = B * ((H + 3) // 4) * ((W + 15) // 16)
    assert chunks == 120
    parts = lib.dhz_conv3x3_wgrad_parts_any(B, H, W, Cin, Kout)
    tiles = (Kout // 32) * (Cin // 32)
    assert parts == min((512 + tiles - 1) // tiles, max(chunks // 4, 1))
    assert parts > 1 and chunks // parts > 1, (parts, chunks)
    assert lib.dhz_conv3x3_wgrad_workspace_bytes_any(B, H, W, Cin, Kout) == parts * (Kout * Cin * 9 + Kout) * 4
    assert lib.dhz_conv3x3_wgrad_parts_any(1, 5, 7, 32, 32) == 1
    assert lib.dhz_conv3x3_wgrad_parts(B, H, W, Cin, Kout) == 0 and lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_conv3x3_wgrad_any_same_bits(shape):
    """run to run, on grids sized for the whole device / 8 / 9 CUs, and with the deterministic mode on: bit-equal"""
    from dehaze_hip import ops
    xb, dyb, _, _ = case(shape)
    dw0, db0 = run(shape, xb, dyb)
    dw1, db1 = run(shape, xb, dyb)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    for level in LEVELS:
        with reserved_grid(level):
            dw, db = run(shape, xb, dyb)
        assert torch.equal(dw, dw0) and torch.equal(db, db0), f"grid level {level}"
    assert not ops.DETERMINISTIC
    try:
        ops.set_deterministic(True)
        ops._stream()                                   # hands the mode's workspace to the library
        nan_ws = torch.full((16,), float("nan"), device="cuda")      # the caller's workspace is not used in this mode
        dw, db = run(shape, xb, dyb, ws=nan_ws)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(dw, dw0) and torch.equal(db, db0)


@pytest.mark.parametrize("shape", REGULAR)
def test_conv3x3_wgrad_any_equals_the_old_entry_where_that_answers(shape):
    from dehaze_hip import _lib
    lib = _lib.load()
    B, Cin, Kout, H, W = shape
    assert lib.dhz_conv3x3_wgrad_workspace_bytes_any(B, H, W, Cin, Kout) == lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout) > 0
    assert lib.dhz_conv3x3_wgrad_parts_any(B, H, W, Cin, Kout) == lib.dhz_conv3x3_wgrad_parts(B, H, W, Cin, Kout) > 0
    assert lib.dhz_conv3x3_wgrad_parts_any(4, 32, 32, 32, 32) == lib.dhz_conv3x3_wgrad_parts(4, 32, 32, 32, 32) == 16
    xb, dyb, dwref, _ = case(shape)
    dwa, dba = run(shape, xb, dyb)
    dwo, dbo = run(shape, xb, dyb, entry="dhz_conv3x3_wgrad")
    assert torch.equal(dwa, dwo) and torch.equal(dba, dbo)
    assert (dwa.cpu().double() - dwref).abs().max().item() < 1e-2      # and it is the gradient, not two equal blanks
