"""-m gpu: every kernel instantiation of csrc/split6_gemm.hip - the 256 x 128 two-slot kernel and the 128 x 128 / 64 / 32 instances
of the three-slot ring, each as forward (dhz_linear_fwd_split6), backward-data (dhz_linear_dgrad_split6) and forward + residual
epilogue (dhz_linear_fwd_split6_res): eleven, 128 x 32 has no backward-data - against float64, through the raw C-ABI.

A persistent workgroup treats its (tile, stage) pairs as one stream, looks three to four stages ahead across tile boundaries and
takes ring slot, register set and fragment set from the stream position mod 6.  The cases of tests/_tile_cases.py (S6_TABLE) run at
five levels - the whole device, grids sized for 8 and for 9 CUs, and deterministic mode at both reservations (the tile chosen for 256
CUs on the reserved grid) - with 1, 2, 3, 5, 6 and 7 stages per tile, so every instantiation walks several tiles per workgroup with
tile boundaries on every stream position, ragged last trips and row tiles, the XCD remap on and off, and changing column tiles
(tests/test_split6_instances_host.py proves that from the table without a GPU).  Which kernel ran is asked of the library
(dhz_linear_split6_tile: the function the dispatch calls) and, at the reserved and deterministic levels, is what the table claims.

Reference: float64 on the device, plain matmul on the fp32 operands: x @ W^T + b, dy @ W.  Epilogue: res + window_reverse / roll of
scale * (x @ W^T + b), by _window_reverse_roll of tests/test_gpu_epilogue.py.  `mag` is the same expression over absolute values (the
shortcut's magnitude added).  Bound on every element: |err| <= 2^-21 mag + 1e-7 (BOUND6 of tests/test_gpu_epilogue.py and
tests/test_gpu_persistent.py).  The weight planes come from dhz_split3_planes.  Outputs are NaN before every call and 64 guard rows
behind them stay NaN; every other contraction runs with ld > width on both sides, NaN in the padding columns, which stay NaN in the
output; forward runs with and without bias; results of two levels that ran the same instance are bit-equal.  Each case prints its
worst err / bound share per level (profiles/split6_instances.txt)."""
import pytest
import torch

import _tile_cases as TC
from test_gpu_epilogue import BOUND6, _window_reverse_roll

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
GUARD = 64
assert BOUND6 == TC.S6_BOUND

ROWS = list(TC.S6_TABLE)
CASES = [(T, F, mode) for (T, F) in ROWS for mode in TC.s6_modes(F)]
# epilogue argument forms: (windowed, shift, map (None: token order), scale, bias, shortcut)
EPI_FORMS = ((1, 0, (8, 8), False, True, True),
             (1, 4, (8, 8), True, True, True),
             (1, 3, (8, 24), True, True, True),        # an image of 192 tokens straddles 128-row tile boundaries (8 x 8 where T % 192 != 0)
             (0, 0, None, True, True, True),
             (0, 0, None, False, False, True),
             (0, 0, None, True, False, False))         # res == NULL, bias == NULL, scale: the row-scaled backward-data of ops.gemm_dgrad
EPI_ANY_T = ((0, 0, None, False, False, True), (0, 0, None, False, True, True))      # rows that are not whole images of 64 tokens


def _s():
    return torch.cuda.current_stream().cuda_stream


def _strided(t, ld):
    """t [rows, cols] in a [rows, ld] buffer whose padding columns are NaN"""
    buf = torch.full((t.shape[0], ld), NAN, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf


def _planes(w):
    """the three bf16 truncation planes of a contiguous fp32 matrix by dhz_split3_planes; they sum to it exactly"""
    from dehaze_hip import _lib
    pl = torch.empty((3, w.numel()), device=DEV, dtype=torch.bfloat16)
    _lib.call("dhz_split3_planes", w.data_ptr(), w.numel(), pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _s())
    assert torch.equal(pl.double().sum(0), w.double().reshape(-1))
    return pl


def _name(ncu, det):
    return ("det" if det else "") + ("whole" if ncu is None else str(ncu))


def _epi_form(T, ri, ci):
    if T % 64:
        return EPI_ANY_T[ci % 2]
    win, shift, hw, scaled, biased, shortcut = EPI_FORMS[(ri + ci) % 6]
    if hw == (8, 24) and T % 192:
        hw = (8, 8)
    return win, shift, hw, scaled, biased, shortcut


@pytest.mark.parametrize("T,F,mode", CASES)
def test_split6_every_instantiation(T, F, mode):
    from dehaze_hip import _lib
    TC.s6_no_override()
    lib = _lib.load()
    ri = ROWS.index((T, F))
    seen = set()
    for ci, KC in enumerate(TC.S6_CONTRACTIONS):
        x, w, b = TC.s6_operands(T, F, KC, DEV, seed=100 * T + F + KC)
        pad = ci % 2 == 1
        ld_in, ld_out = (KC + 8, F + 4) if pad else (KC, F)
        xs = _strided(x, ld_in)
        y64 = x.double() @ w.double().t()
        mag = x.double().abs() @ w.double().abs().t()
        what, res, sc, form = "", None, None, None
        if mode == "dgrad":                                   # dx[T, F] = dy[T, KC] W[KC, F]: the planes of W as it lies
            pl = _planes(w.t().contiguous())
            biased = False
        else:
            pl = _planes(w)
            biased = ci % 2 == 0
        if mode == "epi":
            form = _epi_form(T, ri, ci)
            win, shift, hw, scaled, biased, shortcut = form
            HW = hw[0] * hw[1] if hw else (64 if scaled else T)
            nimg = T // HW
            what = f" form={'win' if win else 'tok'}{shift}/{HW}{'/scale' if scaled else ''}{'' if shortcut else '/nores'}"
        if biased:
            y64 = y64 + b.double()
            mag = mag + b.double().abs()
        if mode == "epi":
            g = torch.Generator(device=DEV).manual_seed(T + KC)
            if scaled:
                sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(nimg)], device=DEV)
                dropped = (sc == 0).repeat_interleave(HW)            # rows of the dropped images, in every trip and ragged tile
                assert bool(dropped.any())
                f = sc.double().repeat_interleave(HW)[:, None]
                y64, mag = f * y64, f * mag
            if win:
                y64, mag = (_window_reverse_roll(t.contiguous(), nimg, hw[0], hw[1], shift) for t in (y64, mag))
            if shortcut:
                res = torch.randn(T, F, generator=g, device=DEV)
                y64, mag = y64 + res.double(), mag + res.double().abs()
                ress = _strided(res, ld_out)
        bound = BOUND6 * mag + 1e-7
        outs, tiles, shares = {}, {}, []
        for k, (ncu, det) in enumerate(TC.S6_LEVELS):
            with TC.s6_level(ncu, det) as n:
                tile = TC.s6_query(lib, mode, T, F, KC)
                if ncu is not None:
                    inst, trips = TC.S6_TABLE[(T, F)][k - 1]
                    assert tile == inst, (T, F, mode, KC, ncu, det, tile)
                    assert TC.s6_plan(tile, T, F, n)[2] == trips
                assert tile in TC.S6_INSTANCES
                out = torch.full((T + GUARD, ld_out), NAN, device=DEV)
                bp = b.data_ptr() if biased else None
                if mode == "fwd":
                    _lib.call("dhz_linear_fwd_split6", xs.data_ptr(), ld_in, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), bp,
                              out.data_ptr(), ld_out, T, F, KC, _s())
                elif mode == "dgrad":
                    _lib.call("dhz_linear_dgrad_split6", xs.data_ptr(), ld_in, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(),
                              out.data_ptr(), ld_out, T, KC, F, _s())
                else:
                    _lib.call("dhz_linear_fwd_split6_res", xs.data_ptr(), ld_in, pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), bp,
                              ress.data_ptr() if shortcut else None, sc.data_ptr() if scaled else None, out.data_ptr(), ld_out, T, F, KC,
                              HW, hw[0] if win else 0, hw[1] if win else 0, shift, win, _s())
                torch.cuda.synchronize()
            lvl = _name(ncu, det)
            assert bool(torch.isnan(out[T:]).all()), (KC, lvl, "a guard row was written")
            assert bool(torch.isnan(out[:T, F:]).all()), (KC, lvl, "a padding column was written")
            got = out[:T, :F]
            share = ((got.double() - y64).abs() / bound).max().item()
            share = share if share == share else float("inf")               # NaN: an element never written
            shares.append(f"{lvl} {tile} {share:.3f}")
            outs[lvl], tiles[lvl] = got, tile
            seen.add(tile)
            assert share <= 1.0, (T, F, mode, KC, lvl, tile, share)
            if mode == "epi" and scaled:                                     # every dropped image returns the shortcut bit for bit
                assert torch.equal(got[dropped], res[dropped] if shortcut else torch.zeros_like(got[dropped])), (KC, lvl, "a dropped image")
        print(f"S6 rows={T} features={F} mode={mode} contraction={KC} ld={'padded' if pad else 'exact'} bias={int(biased)}{what} | "
              + " | ".join(shares))
        names = list(outs)
        for i, a in enumerate(names):
            for c in names[i + 1:]:
                if tiles[a] == tiles[c]:
                    assert torch.equal(outs[a], outs[c]), (T, F, mode, KC, a, c, tiles[a])
    assert seen >= {inst for inst, _ in TC.S6_TABLE[(T, F)]}


def test_refused_shapes_launch_nothing():
    """a shape the dispatch refuses answers an error, its tile query answers 0, and the output is still NaN"""
    from dehaze_hip import _lib
    lib = _lib.load()
    T = 128
    x = torch.randn(T, 96, device=DEV)
    pl = torch.zeros((3, 96 * 96), device=DEV, dtype=torch.bfloat16)
    out = torch.full((T, 96), NAN, device=DEV)
    p = [pl[i].data_ptr() for i in range(3)]
    for N, K in ((48, 64), (64, 48)):
        assert lib.dhz_linear_split6_tile(1, T, N, K) == 0 and lib.dhz_linear_split6_tile(2, T, N, K) == 0
        assert lib.dhz_linear_fwd_split6(x.data_ptr(), 96, *p, None, out.data_ptr(), 96, T, N, K, _s()) != 0
        assert lib.dhz_linear_dgrad_split6(x.data_ptr(), 96, *p, out.data_ptr(), 96, T, N, K, _s()) != 0
        assert lib.dhz_linear_fwd_split6_res(x.data_ptr(), 96, *p, None, None, None, out.data_ptr(), 96, T, N, K, T, 0, 0, 0, 0, _s()) != 0
    # backward-data: 96 output features (w's columns) are a multiple of 32 but not of 64
    assert lib.dhz_linear_split6_tile(2, T, 64, 96) == 0 and lib.dhz_linear_split6_tile(1, T, 96, 64) == 41
    assert lib.dhz_linear_dgrad_split6(x.data_ptr(), 96, *p, out.data_ptr(), 96, T, 64, 96, _s()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
