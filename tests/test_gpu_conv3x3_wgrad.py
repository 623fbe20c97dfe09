"""-m gpu: the dense 3x3 / stride 1 / pad 1 weight and bias gradient on the channel-blocked layout (csrc/conv3x3_wgrad.hip,
dhz_conv3x3_wgrad) against float64 torch.nn.grad.conv2d_weight and the float64 sum of dy, both computed on the CPU.

Shapes (B, Cin, Kout, H = W): the smallest at which each mechanism can go wrong - one 16 x 16 block per image; two output-channel
tiles; the 8 x 8 geometry (a chunk is a whole image) at an odd batch; the widest contraction operand (16 input-channel tiles); and a map
with 64 chunks, which the cut splits into 16 slabs of 4 chunks: more than one chunk per work item (the accumulation loop runs on) and
more than one work item per tile (the second pass has something to sum) - asserted from the parts query below.  Under
reserved_grid(8 / 9) the persistent grid has at most 32 / 36 workgroups: MANY_ITEMS (40 chunks, 10 slabs x 4 tiles = 40 items) makes
workgroups of both grids walk on to a second item, with a ragged last trip.
NONSQUARE, (B, Cin, Kout, H, W) with H != W: the chunk walk (bxn = W / 16 chunks per row group, cpi = (H / 4) * bxn per image) and the row
pitch of the planes tell the two apart only there; Cin != Kout as well."""
import pytest
import torch

from _grid import LEVELS, reserved_grid

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32, 32, 16), (1, 32, 64, 16), (3, 64, 32, 8), (2, 512, 32, 8), (4, 32, 32, 32)]
MANY_ITEMS = (10, 64, 64, 16)
NONSQUARE = [(2, 32, 64, 16, 32), (2, 32, 64, 32, 16)]
CANARY = 4096            # floats of NaN behind the queried workspace


def blocked(t):
    """[B, C, H, W] -> the kernels' [B, C/8, H, W, 8]"""
    B, C, H, W = t.shape
    return t.view(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def dims(shape):
    """(B, Cin, Kout, H, W) of a shape given with or without W"""
    return shape if len(shape) == 5 else shape + (shape[3],)


_CASES = {}


def case(shape):
    """inputs and the float64 reference of one shape, computed once and shared (never modified)"""
    if shape not in _CASES:
        B, Cin, Kout, H, W = dims(shape)
        g = torch.Generator().manual_seed(1000 + B + Cin + Kout + H + 7 * (W - H))
        x = torch.randn(B, Cin, H, W, generator=g)
        dy = torch.randn(B, Kout, H, W, generator=g)
        dw = torch.nn.grad.conv2d_weight(x.double(), (Kout, Cin, 3, 3), dy.double(), stride=1, padding=1)
        db = dy.double().sum((0, 2, 3))
        _CASES[shape] = (blocked(x).cuda(), blocked(dy).cuda(), dw, db)
    return _CASES[shape]


def run(shape, xb, dyb, with_db=True, ws=None):
    """one call with NaN canaries in the outputs and behind the workspace; returns (dw, db) on the device"""
    from dehaze_hip import _lib
    B, Cin, Kout, H, W = dims(shape)
    lib = _lib.load()
    need = lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout)
    assert need > 0 and need % 4 == 0
    if ws is None:
        ws = torch.full((need // 4 + CANARY,), float("nan"), device="cuda")
    dw = torch.full((Kout, Cin, 3, 3), float("nan"), device="cuda")
    db = torch.full((Kout,), float("nan"), device="cuda")
    _lib.call("dhz_conv3x3_wgrad", xb.data_ptr(), dyb.data_ptr(), dw.data_ptr(), db.data_ptr() if with_db else None, ws.data_ptr(), need,
              B, H, W, Cin, Kout, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(ws[need // 4:]).all(), "the kernel wrote behind the queried workspace"
    return dw, db


@pytest.mark.parametrize("shape", SHAPES + [MANY_ITEMS] + NONSQUARE)
def test_conv3x3_wgrad_matches_float64(shape):
    B, Cin, Kout, H, W = dims(shape)
    xb, dyb, dwref, dbref = case(shape)
    dw, db = run(shape, xb, dyb)
    T = B * H * W
    # the bounds of the existing convolution weight-gradient check, tests/test_gpu_conv.py:47-48 (dhz_conv4s2_wgrad):
    #   assert (dwp.cpu().double() - 0.5 - dwref).abs().max() < 3e-6 * T ** 0.5 * max(1.0, dwref.abs().max().item() / T ** 0.5) + 1e-4
    #   assert (db.cpu().double() + 1.0 - br.grad).abs().max() < 3e-5 * T ** 0.5 + 1e-4
    edw = (dw.cpu().double() - dwref).abs().max().item()
    edb = (db.cpu().double() - dbref).abs().max().item()
    bdw = 3e-6 * T ** 0.5 * max(1.0, dwref.abs().max().item() / T ** 0.5) + 1e-4
    bdb = 3e-5 * T ** 0.5 + 1e-4
    print(f"conv3x3_wgrad {shape}: dW error {edw:.3e} (bound {bdw:.3e}), db error {edb:.3e} (bound {bdb:.3e})")
    assert edw < bdw
    assert edb < bdb
    # db == NULL leaves dW bit-equal (and db untouched)
    dw2, db2 = run(shape, xb, dyb, with_db=False)
    assert torch.equal(dw2, dw)
    assert torch.isnan(db2).all()


def test_conv3x3_wgrad_cut_has_slabs_and_chunks():
    """(4, 32, 32, 32): 64 chunks of 64 positions in 16 slabs - several chunks per work item, several work items per tile; the
    workspace is slabs x (dW + db) floats"""
    from dehaze_hip import _lib
    lib = _lib.load()
    B, Cin, Kout, H = (4, 32, 32, 32)
    parts = lib.dhz_conv3x3_wgrad_parts(B, H, H, Cin, Kout)
    chunks = B * (H // 4) * (H // 16)
    assert parts > 1 and chunks // parts > 1, (parts, chunks)
    assert lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, H, Cin, Kout) == parts * (Kout * Cin * 9 + Kout) * 4
    assert lib.dhz_conv3x3_wgrad_parts(2, 8, 8, 512, 32) >= 1
    B, Cin, Kout, H = MANY_ITEMS
    items = lib.dhz_conv3x3_wgrad_parts(B, H, H, Cin, Kout) * (Kout // 32) * (Cin // 32)
    assert items > 4 * 9 and items % 32 != 0 and items % 36 != 0          # more items than 4 workgroups on each of 8 / 9 CUs


@pytest.mark.parametrize("shape", [(2, 512, 32, 8), (4, 32, 32, 32), MANY_ITEMS] + NONSQUARE)
def test_conv3x3_wgrad_same_bits(shape):
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


@pytest.mark.parametrize("shape", [(2, 32, 32, 16), (3, 64, 32, 8)])
def test_conv3x3_wgrad_never_reads_the_halo(shape):
    """x inside a larger allocation whose memory just before its first plane and just behind its last is NaN / 1e30: the rows above the
    first and below the last plane are padding that is never loaded, so the result is bit-equal.  The halo of interior planes and the
    column halo alias real data of neighbouring rows and planes: a stray read there shows only in the float64 comparison above."""
    B, Cin, Kout, H = shape
    xb, dyb, _, _ = case(shape)
    dw0, db0 = run(shape, xb, dyb)
    pad = 2 * H * 8 + 64                                # two map rows of one plane, and a little more
    for poison in (float("nan"), 1e30):
        big = torch.full((xb.numel() + 2 * pad,), poison, device="cuda")
        big[pad:pad + xb.numel()] = xb.reshape(-1)
        dw, db = run(shape, big[pad:pad + xb.numel()].view_as(xb), dyb)
        assert torch.equal(dw, dw0) and torch.equal(db, db0)
