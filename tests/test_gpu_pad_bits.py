"""-m gpu: the padding mask of any-size evaluation as one 64-bit word per window (bit i: token i is padding).

dhz_pad_window_bits against F.interpolate + window_partition; the padding-word forms of the chain kernels (dhz_ps_attn_fwd_dt_pad,
dhz_ps_attn_bwd_dt_pad, dhz_ps_attn_fwd_w_pad, dhz_ps_attn_bwd_w_pad) bit for bit against the entries without `_pad` given the
materialised padding + shift mask tensor, and against the float64 oracle; the fused forward (dhz_fused_window_attn_fwd_pad) against the
chain; the model at batch 2 against the oracle at batch 1; peak memory; autograd against the tensor route (DHZ_PAD_BITS=0).

The words are hand-chosen: between them 0, all ones, only bit 63, only bits 32..63, only bit 0, a ragged pattern, the two bits either
side of the 32-bit boundary - a 32-bit shift on the word passes every test whose padding lies in tokens 0..31 and fails here."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import uformer_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")

ALL = (1 << 64) - 1
WORDS = [0, ALL, 1 << 63, 0xFFFFFFFF00000000, 1, 0x8421F00F0FF0A5C3, (1 << 31) | (1 << 32), 0x00FF00FF0000FFFF]


def _L():
    from dehaze_hip import _lib
    return _lib


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _words_tensor(words):
    """python uint64 values -> int64 tensor with the same bit patterns"""
    return torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in words], dtype=torch.int64)


def _flags(words, N):
    """[len(words), N] bool: bit i of word b (4 x 4 windows: the low 16 bits)"""
    return torch.tensor([[(w >> i) & 1 for i in range(N)] for w in words], dtype=torch.bool)


def _materialised(words, N, sm):
    """the tensor the reference builds (M1:791-800): -100 where query AND key are padding, plus the shift mask of window b % nW"""
    f = _flags(words, N)
    am = torch.where(f[:, :, None] & f[:, None, :], torch.tensor(-100.0), torch.tensor(0.0))
    return am if sm is None else am + sm[torch.arange(len(words)) % sm.shape[0]]


def _mask_image(words, B, H, W, win):
    """[B, 1, H, W] image-space mask (1 = padding) whose windows carry `words`: the inverse of window_partition at the block's resolution"""
    N = win * win
    f = _flags(words, N).float().view(B, H // win, W // win, win, win)
    return f.permute(0, 1, 3, 2, 4).reshape(B, 1, H, W).contiguous()


def _pack_host(mask, H, win):
    """the words of a block on an H x H map, packed on the host from F.interpolate + window_partition"""
    from dehaze_hip import model
    im = F.interpolate(mask, size=(H, H)).permute(0, 2, 3, 1)
    am = model.window_partition(im, win).reshape(-1, win * win)
    return _words_tensor([sum(1 << i for i in range(win * win) if row[i] != 0) for row in am.tolist()])


# ----------------------------------------------------------------------------- 1. the words
def _padding_mask(valid=1.0, other=None):
    """[2, 1, 32, 32], 1 - mask of the eval script: 0 on an off-centre valid rectangle that differs per image, `valid` elsewhere"""
    m = torch.full((2, 1, 32, 32), valid)
    if other is not None:
        m[1] = other
    m[0, :, 3:25, 7:30] = 0
    m[1, :, 10:32, 0:13] = 0
    return m


@pytest.mark.parametrize("H,win", [(32, 8), (16, 8), (8, 8), (16, 4), (4, 4)])
def test_pad_window_bits_equal_interpolate_and_partition(H, win):
    from dehaze_hip import ops
    mask = _padding_mask()
    ref = _pack_host(mask, H, win)
    got = ops.pad_window_bits(mask.to(DEV), H, H, win)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref)
    if H == 32:
        assert int((ref != 0).sum()) > 0 and int((ref == 0).sum()) > 0                # windows with and without padding
    # the raw entry, into a poisoned buffer: every word is written
    bits = torch.full((ref.numel(),), 0x5555555555555555, dtype=torch.int64, device=DEV)
    md = mask.to(DEV)
    _L().call("dhz_pad_window_bits", _p(md), _p(bits), 2, 32, 32, H, H, win, _s())
    assert torch.equal(bits.cpu(), ref)
    if win == 4:
        assert int((ref >> 16).abs().max()) == 0                                      # 4 x 4 windows use the low 16 bits


def test_pad_window_bits_flag_is_nonzero_not_one():
    from dehaze_hip import ops
    mask = _padding_mask(valid=0.5, other=-3.0)
    for H, win in ((32, 8), (16, 4)):
        assert torch.equal(ops.pad_window_bits(mask.to(DEV), H, H, win).cpu(), _pack_host(_padding_mask(), H, win))
    with pytest.raises(_L().DehazeHipError, match="Himg"):
        ops.pad_window_bits(torch.zeros(1, 1, 40, 40, device=DEV), 16, 16, 8)


# ----------------------------------------------------------------------------- 2. / 3. chain kernels
CHAIN = [(64, 2, 32), (64, 1, 16), (64, 2, 64), (16, 2, 32), (16, 1, 16), (16, 2, 64)]          # (N, H, d)


def _entries(N):
    return ("dhz_ps_attn_fwd_dt", "dhz_ps_attn_bwd_dt", "dhz_bias_gather", "dhz_bias_table_grad") if N == 64 else \
        ("dhz_ps_attn_fwd_w", "dhz_ps_attn_bwd_w", "dhz_bias_gather_w", "dhz_bias_table_grad_w")


@functools.lru_cache(maxsize=None)
def _chain_inputs(N, H, d):
    win = 8 if N == 64 else 4
    u = O.n_top(N)
    g = torch.Generator().manual_seed(1000 * N + 10 * H + d)
    B_ = len(WORDS)
    q, k, v = (torch.randn(B_, H, N, d, generator=g) for _ in range(3))
    idx = torch.randint(N, (N, u), generator=g)
    table = 0.3 * torch.randn((2 * win - 1) ** 2, H, generator=g)
    gout = torch.randn(B_, H, N, d, generator=g)
    sm = O.shift_attn_mask(2 * win, 2 * win, win, win // 2)                            # nW = 4: two images of four windows
    return dict(win=win, u=u, B_=B_, q=q, k=k, v=v, idx=idx, table=table, gout=gout, sm=sm, full=_materialised(WORDS, N, sm))


def _tok(t):
    B_, H, n, d = t.shape
    return t.transpose(1, 2).reshape(B_ * n, H * d)


def _run_chain(N, H, d, dtype, pad):
    """forward + backward + table gradient through the raw ABI: pad = False the existing entries with the materialised [B_, N, N] mask
    (nW = B_), pad = True the padding-word entries with the [4, N, N] shift mask and the words (nW = 4)"""
    from dehaze_hip import ops
    c = _chain_inputs(N, H, d)
    win, B_, C = c["win"], c["B_"], H * d
    fwd, bwd, gather, tgrad = _entries(N)
    qkv = torch.cat([_tok(c["q"]), _tok(c["k"]), _tok(c["v"])], 1).to(DEV).to(dtype).contiguous()
    gout = _tok(c["gout"]).to(DEV).to(dtype).contiguous()
    idx = c["idx"].to(torch.uint8).to(DEV)
    table = c["table"].to(DEV)
    bias = torch.empty(H, N, N, device=DEV)
    _L().call(gather, _p(table), _p(bias), H, *(() if N == 64 else (win,)), _s())
    mask = (c["sm"] if pad else c["full"]).to(DEV).contiguous()
    nW = mask.shape[0]
    words = _words_tensor(WORDS).to(DEV)
    out = torch.full((B_ * N, C), float("nan"), device=DEV, dtype=dtype)
    rank = torch.full((B_, H, N), 77, device=DEV, dtype=torch.uint8)
    dqkv = torch.full((B_ * N, 3 * C), float("nan"), device=DEV, dtype=dtype)
    parts = _L().load().dhz_ps_attn_bwd_parts_w(B_, H, d, win)
    dpart = torch.full((parts, N, N), float("nan"), device=DEV)
    es, base, gb, dt = qkv.element_size(), qkv.data_ptr(), dqkv.data_ptr(), 1 if dtype == BF else 0
    wtail = () if N == 64 else (win,)
    padarg = (_p(words),) if pad else ()
    _L().call(fwd + ("_pad" if pad else ""), base, base + es * C, base + 2 * es * C, 3 * C, _p(idx), _p(bias), _p(mask), *padarg, _p(out), C,
              _p(rank), B_, H, nW, d, *wtail, dt, _s())
    _L().call(bwd + ("_pad" if pad else ""), base, base + es * C, base + 2 * es * C, 3 * C, _p(bias), _p(mask), *padarg, _p(rank), _p(gout), C,
              gb, gb + es * C, gb + 2 * es * C, 3 * C, _p(dpart), B_, H, nW, d, *wtail, dt, _s())
    # the table gradient in a fixed order of summation (the 64-token reduction uses fp32 atomics otherwise)
    dtable = torch.full(((2 * win - 1) ** 2, H), float("nan"), device=DEV)
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        _L().call(tgrad, _p(dpart), parts, _p(dtable), H, 0, *wtail, _s())
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    return out, rank, dqkv, dpart, dtable


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("N,H,d", CHAIN)
def test_chain_pad_entries_bit_identical_to_the_mask_tensor(N, H, d, dtype):
    """dhz_ps_attn_fwd_dt_pad / dhz_ps_attn_bwd_dt_pad (N = 64) and dhz_ps_attn_fwd_w_pad / dhz_ps_attn_bwd_w_pad (N = 16): (shift term +
    padding term) is exact and is added where the mask is added, so output, ranks, dqkv and the bias-table gradient are the same bits"""
    ref = _run_chain(N, H, d, dtype, pad=False)
    got = _run_chain(N, H, d, dtype, pad=True)
    for name, a, b in zip(("out", "rank", "dqkv", "dbias_part", "dtable"), got, ref):
        assert not torch.isnan(a.float()).any(), name
        same = torch.equal(a, b)
        print(f"{name}: equal {same}" + ("" if same else f", max diff {(a.float() - b.float()).abs().max().item():.3e}"))
        assert same, name
    if N == 64:            # the window-parametrised entry at win = 8 runs the same kernel
        c = _chain_inputs(N, H, d)
        C, B_ = H * d, c["B_"]
        qkv = torch.cat([_tok(c["q"]), _tok(c["k"]), _tok(c["v"])], 1).to(DEV).to(dtype).contiguous()
        bias = torch.zeros(H, N, N, device=DEV)
        out = torch.empty((B_ * N, C), device=DEV, dtype=dtype)
        rank = torch.empty((B_, H, N), device=DEV, dtype=torch.uint8)
        es, base = qkv.element_size(), qkv.data_ptr()
        idx, sm, words = c["idx"].to(torch.uint8).to(DEV), c["sm"].to(DEV), _words_tensor(WORDS).to(DEV)
        outs = []
        for entry, tail in (("dhz_ps_attn_fwd_dt_pad", ()), ("dhz_ps_attn_fwd_w_pad", (8,))):
            _L().call(entry, base, base + es * C, base + 2 * es * C, 3 * C, _p(idx), _p(bias), _p(sm), _p(words), _p(out), C, _p(rank), B_, H, 4, d,
                      *tail, 1 if dtype == BF else 0, _s())
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("N,H,d", CHAIN)
def test_chain_pad_entries_vs_float64(N, H, d):
    """the same inputs against the float64 oracle with the materialised mask; tolerances and the tie rule of the selection are those of
    tests/test_gpu_kernels.py::test_ps_attention_oracle"""
    c = _chain_inputs(N, H, d)
    win, u, B_, C = c["win"], c["u"], c["B_"], H * d
    q64, k64, v64 = (c[n].double().requires_grad_() for n in ("q", "k", "v"))
    t64 = c["table"].double().requires_grad_()
    bias = t64[O.relative_position_index(win).reshape(-1)].reshape(N, N, H).permute(2, 0, 1)
    ctx, top, Mq, _, _ = O.prob_attention(q64, k64, v64, c["idx"], bias, c["full"].double(), return_aux=True)
    (ctx * c["gout"].double()).sum().backward()
    out, rank, dqkv, _, dtable = _run_chain(N, H, d, torch.float32, pad=True)
    r = rank.cpu().numpy()
    bad = 0
    for b in range(B_):
        for h in range(H):
            if sorted(np.nonzero(r[b, h] < u)[0].tolist()) != sorted(top[b, h].tolist()):
                m = Mq[b, h].detach().sort(descending=True)[0]
                assert (m[u - 1] - m[u]).abs() < 1e-5 * m.abs().max(), "selection differs without a near-tie"
                bad += 1
    assert bad <= max(1, B_ * H // 200)
    oerr = (out.cpu().double() - _tok(ctx.detach())).abs().max().item()
    gref = torch.cat([_tok(t.grad) for t in (q64, k64, v64)], 1)
    gerr = (dqkv.cpu().double() - gref).abs().max().item()
    terr = (dtable.cpu().double() - t64.grad).abs().max().item()
    print(f"selection mismatches {bad}; max err: out {oerr:.3e} dqkv {gerr:.3e} dtable {terr:.3e}")
    if bad == 0:
        assert torch.allclose(out.cpu().double(), _tok(ctx.detach()), atol=2e-5, rtol=1e-4), oerr
        assert torch.allclose(dqkv.cpu().double(), gref, atol=1e-4, rtol=1e-3), gerr
        assert torch.allclose(dtable.cpu().double(), t64.grad, atol=2e-4 * B_ ** 0.5, rtol=2e-3), terr


# ----------------------------------------------------------------------------- 4. fused forward
def _block(C, heads, res, shift, win=8, seed=0):
    import My_model_1 as M1
    torch.manual_seed(100 + C + res + shift + seed)
    blk = M1.LeWinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=heads, win_size=win, shift_size=shift,
                                   token_mlp='leff', drop_path=0.).to(DEV)
    with torch.no_grad():
        for p in blk.parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn_like(p))
        blk.attn.relative_position_bias_table.mul_(15.0)
    return blk


@pytest.mark.parametrize("six_term", [True, False], ids=["six", "fp32pipe"])
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("C,heads,res", [(32, 1, 16), (64, 2, 16), (128, 4, 32)])
def test_fused_forward_with_padding_words(C, heads, res, shift, six_term):
    """dhz_fused_window_attn_fwd_pad (inference instances of the fused forward, six-term and fp32-pipe projections) against the kernel
    chain given the same words, under the tolerance of tests/test_gpu_fused.py; with all words 0 it is the kernel without padding words,
    bit for bit."""
    from dehaze_hip import fused
    B, nW = 2, (res // 8) ** 2
    words = (WORDS * ((B * nW + len(WORDS) - 1) // len(WORDS)))[:B * nW]
    blk = _block(C, heads, res, shift).eval()
    x = torch.randn(B, res * res, C, device=DEV)
    idx = torch.randint(64, (64, 25)).to(torch.uint8).to(DEV)
    dummy = torch.zeros(B, 1, res, res, device=DEV)            # the block takes the staged words, not this image
    calls = []
    real = _L().call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    def run(w, enabled):
        blk._staged_idx = idx
        blk._staged_pad = None if w is None else _words_tensor(w).to(DEV)
        fused.ENABLED = enabled
        try:
            return blk(x) if w is None else blk(x, dummy)
        finally:
            fused.ENABLED = True

    old = (fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C, fused.ATTN_FUSED_PAD_P6_C)
    # every width in either arithmetic (C = 32 six-term is built but not dispatched), the same with and without words
    fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C, fused.ATTN_FUSED_PAD_P6_C = six_term, (32, 64, 128), (32, 64, 128)
    _L().call = spy
    try:
        with torch.no_grad():
            yf = run(words, True)
            fused_calls = list(calls)
            yc = run(words, False)
            y0 = run([0] * (B * nW), True)
            yn = run(None, True)
    finally:
        _L().call = real
        fused.ATTN_FUSED_P6, fused.ATTN_FUSED_P6_C, fused.ATTN_FUSED_PAD_P6_C = old
    assert "dhz_fused_window_attn_fwd_pad" in fused_calls and "dhz_ps_attn_fwd_w_pad" not in fused_calls
    assert "dhz_ps_attn_fwd_w_pad" in calls
    err = (yf - yc).abs().max().item()
    print(f"fused vs chain max err {err:.3e}; padding changes the output by {(yf - yn).abs().max().item():.3e}")
    assert torch.allclose(yf, yc, atol=2e-5, rtol=1e-4), err
    assert (yf - yn).abs().max().item() > 1e-3, "the words do not reach the kernel"
    assert torch.equal(y0, yn)


# ----------------------------------------------------------------------------- 5. model, batch 2
def _canvas(h, w, seed):
    import test_in_any_resolution as TA
    g = torch.Generator().manual_seed(seed)
    return TA.expand2square(torch.rand(1, 3, h, w, generator=g), factor=128)


_CHILD = """
import sys, torch
sys.path[:0] = [%r, %r]
import My_model_1 as M1
from dehaze_hip import ops
assert ops.PAD_BITS is False
dev = torch.device("cuda:0")
torch.manual_seed(4321)
model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev).eval()
x, m = torch.load(sys.argv[1])
torch.manual_seed(11)
with torch.no_grad():
    y = model(x.to(dev), m.to(dev)).cpu()
assert all(b._staged_pad is None for st in model.stages() for b in st.blocks)
torch.save(y, sys.argv[2])
"""


def test_model_batch_two_vs_oracle_at_batch_one(tmp_path):
    """two images of different valid size in ONE masked forward: each equals the oracle's forward of that image alone (the tensor route
    and the reference cannot run this batch: [B nW, N, N] + [nW, N, N] does not broadcast for B > 1).  Tolerance of
    tests/test_gpu_data_eval.py::test_any_resolution_mask_path_vs_oracle.  The tensor route (DHZ_PAD_BITS=0, its own process: the switch is
    read at import) agrees at batch 1."""
    import My_model_1 as M1
    torch.manual_seed(4321)
    model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(DEV).eval()
    P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    (s0, m0), (s1, m1) = _canvas(100, 70, 21), _canvas(60, 120, 22)
    x, pad = torch.cat([s0, s1]), 1 - torch.cat([m0, m1])
    assert x.shape == (2, 3, 128, 128) and float(m0.sum()) == 100 * 70 and float(m1.sum()) == 60 * 120
    torch.manual_seed(11)
    with torch.no_grad():
        y = model(x.to(DEV), pad.to(DEV)).cpu()
    for i, (s, m) in enumerate(((s0, m0), (s1, m1))):
        torch.manual_seed(11)
        with torch.no_grad():
            yo = O.uformer_forward(P, s, img_size=128, mask=1 - m)
        err = (y[i:i + 1] - yo).abs().max().item()
        print(f"image {i}: max err vs oracle {err:.3e}")
        assert torch.allclose(y[i:i + 1], yo, atol=2e-4, rtol=1e-3), (i, err)
    # the tensor route at batch 1, in a child process
    torch.manual_seed(11)
    with torch.no_grad():
        y1 = model(s0.to(DEV), (1 - m0).to(DEV)).cpu()
    torch.save((s0, 1 - m0), tmp_path / "in.pt")
    env = dict(os.environ, DHZ_PAD_BITS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % (PKG, ROOT), str(tmp_path / "in.pt"), str(tmp_path / "out.pt")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    yt = torch.load(tmp_path / "out.pt")
    err = (y1 - yt).abs().max().item()
    print(f"pad words vs tensor route (batch 1): max diff {err:.3e}")
    assert torch.allclose(y1, yt, atol=2e-4, rtol=1e-3), err


# ----------------------------------------------------------------------------- 6. no mask tensor
def test_masked_forward_allocates_no_mask_tensor():
    """512 x 512 canvas: the masked forward's peak memory is the unmasked forward's plus the words (one stage-0 mask tensor alone would be
    4096 windows x 16 KiB = 64 MiB)"""
    import My_model_1 as M1
    torch.manual_seed(5)
    model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(DEV).eval()
    x = torch.rand(1, 3, 512, 512, device=DEV)
    pad = torch.ones(1, 1, 512, 512, device=DEV)
    pad[:, :, 60:450, 100:500] = 0
    peaks = {}
    with torch.no_grad():
        for name, args in (("warm", (x,)), ("warm_masked", (x, pad)), ("plain", (x,)), ("masked", (x, pad))):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            if name == "masked":
                model._stage_pad_bits(x, pad)
                staged = {b._staged_pad.data_ptr(): b._staged_pad for st in model.stages() for b in st.blocks}
                nbytes = sum(t.numel() * 8 for t in staged.values())
                assert len(staged) == 5 and nbytes < 64 * 1024, (len(staged), nbytes)
                del staged
            y = model(*args)
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
            del y
    print({k: f"{v / 2 ** 20:.2f} MiB" for k, v in peaks.items()})
    assert peaks["masked"] - peaks["plain"] < (1 << 20), peaks


# ----------------------------------------------------------------------------- 7. autograd
@pytest.mark.parametrize("win,res,shift,B", [(8, 16, 0, 2), (8, 16, 4, 1), (4, 8, 0, 2), (4, 8, 2, 1)])
def test_block_under_autograd_equals_the_tensor_route(win, res, shift, B):
    """one 8 x 8 and one 4 x 4 block under grad with the words of test 2 (an image-space mask at the block's resolution that carries them):
    outputs, input and parameter gradients with the padding words equal those of the tensor route (ops.PAD_BITS False, what DHZ_PAD_BITS=0
    sets: the switch is read once at import into that attribute, which both routes consult at call time, so flipping it here is the same
    comparison without a second process), in the deterministic mode's fixed order of summation.  The tensor route adds [B nW, N, N] to the [nW, N, N] shift mask: the
    shifted blocks run one image (four of the words), the unshifted ones two (all eight)."""
    from dehaze_hip import ops
    C, N = 32, win * win
    words = WORDS if B == 2 else [WORDS[2], WORDS[3], WORDS[5], WORDS[6]]
    blk = _block(C, 1, res, shift, win=win, seed=7).train()
    mask = _mask_image(words, B, res, res, win).to(DEV)
    assert torch.equal(ops.pad_window_bits(mask, res, res, win).cpu(), _words_tensor([w & ((1 << N) - 1) for w in words]))
    x = torch.randn(B, res * res, C, device=DEV)
    gout = torch.randn(B, res * res, C, device=DEV)
    idx = torch.randint(N, (N, O.n_top(N))).to(torch.uint8).to(DEV)
    calls = []
    real = _L().call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    def run(pad_bits):
        old, was = ops.PAD_BITS, ops.DETERMINISTIC
        ops.PAD_BITS = pad_bits
        ops.set_deterministic(True)
        del calls[:]
        _L().call = spy
        try:
            for p in blk.parameters():
                p.grad = None
            xx = x.clone().requires_grad_()
            blk._staged_idx = idx
            y = blk(xx, mask)
            (y * gout).sum().backward()
            torch.cuda.synchronize()
            return y.detach(), xx.grad.clone(), {n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None}, list(calls)
        finally:
            _L().call = real
            ops.PAD_BITS = old
            ops.set_deterministic(was)

    yt, dxt, gt, ct = run(False)
    yp, dxp, gp, cp = run(True)
    fwd, bwd = "dhz_ps_attn_fwd_w_pad", "dhz_ps_attn_bwd_w_pad"                       # (ops calls the `_w` entries at either window side)
    assert fwd in cp and bwd in cp and "dhz_pad_window_bits" in cp and "dhz_fused_window_attn_fwd_pad" not in cp
    assert not [n for n in ct if n.endswith("_pad") or n == "dhz_pad_window_bits"]
    assert set(gt) == set(gp) and "attn.relative_position_bias_table" in gp
    bad = []
    for name, a, b in [("y", yp, yt), ("dx", dxp, dxt)] + [(n, gp[n], gt[n]) for n in sorted(gt)]:
        if not torch.equal(a, b):
            bad.append((name, (a - b).abs().max().item(), b.abs().max().item()))
    print("differing tensors (name, max diff, max ref):", bad)
    assert not bad, bad


# ----------------------------------------------------------------------------- 8. the batched driver
def test_batched_eval_driver_synthetic():
    """eval_any_resolution.py: three synthetic images of one size at --batch_size 2 = one forward of two images and one of one"""
    import eval_any_resolution as EA
    from dehaze_hip import ops
    shapes = []
    real = ops.pad_window_bits

    def spy(mask, H, W, win=8):
        shapes.append((mask.shape[0], H))
        return real(mask, H, W, win)

    ops.pad_window_bits = spy
    try:
        torch.manual_seed(6)
        p1, s1, p2, s2 = EA.main(["--synthetic", "3", "--height", "90", "--width", "140", "--batch_size", "2"])
    finally:
        ops.pad_window_bits = real
    assert np.isfinite([p1, s1, p2, s2]).all() and abs(p1 - p2) < 1e-3
    assert [b for b, H in shapes if H == 256] == [2, 1] and len(shapes) == 10, shapes


def test_mask_of_another_ratio_keeps_the_tensor_route():
    """a block called on its own with a mask that is no whole multiple of its map (24 x 24 for a 16 x 16 map), or with two channels, is
    resampled by F.interpolate as before: no padding words, the same bits as with the switch off"""
    from dehaze_hip import ops
    blk = _block(32, 1, 16, 0).eval()
    x = torch.randn(1, 256, 32, device=DEV)
    idx = torch.randint(64, (64, 25)).to(torch.uint8).to(DEV)
    mask = torch.zeros(1, 1, 24, 24, device=DEV)
    mask[:, :, :9, :] = 1
    calls = []
    real = _L().call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)

    def run(on):
        old = ops.PAD_BITS
        ops.PAD_BITS = on
        try:
            blk._staged_idx = idx
            with torch.no_grad():
                return blk(x, mask)
        finally:
            ops.PAD_BITS = old

    assert not ops.pad_bits_cover(mask, 16, 16) and ops.pad_bits_cover(mask, 12, 12) and not ops.pad_bits_cover(mask.expand(1, 2, 24, 24), 12, 12)
    _L().call = spy
    try:
        y1 = run(True)
    finally:
        _L().call = real
    assert not [n for n in calls if n.endswith("_pad") or n == "dhz_pad_window_bits"], calls
    assert torch.equal(y1, run(False))
