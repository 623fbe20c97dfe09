"""-m gpu: the deterministic mode (dhz_set_deterministic, dehaze_hip.ops.set_deterministic).  With it on, an accumulating entry gives
the same bits from call to call and under a smaller persistent grid (the cut into work items is a function of the shape), still meets the fp64
reference at the tolerance of its default-mode test, and still ADDS to its target.  A whole training step repeats bit for bit.

Tolerances are the ones of the entries' own tests: tests/test_gpu_split.py (BOUND[6] of sum |dy||x| + 1e-6; bias sums rtol 1e-5, atol
1e-3 sqrt(T)), tests/test_gpu_linear.py (2e-5 sqrt(T) for dhz_linear_wgrad / _multi, 1e-3 for the row-scaled shape of its C-ABI test),
tests/test_gpu_model.py::test_training_steps_vs_oracle (called as it is: the issue asks for that very comparison); the other entries name
their source in their docstrings.  The flag is process-global: every test clears it on the way out."""
import contextlib
import ctypes
import re
import warnings

import pytest
import torch
import torch.nn.functional as F

from _grid import reserved_grid

pytestmark = pytest.mark.gpu

BOUND6 = 2.0 ** -21            # tests/test_gpu_split.py


@contextlib.contextmanager
def deterministic(workspace_bytes=None):
    from dehaze_hip import _lib, ops
    try:
        ops.set_deterministic(True, workspace_bytes)
        assert _lib.load().dhz_get_deterministic() == 1
        ops._stream()             # the workspace is with the library from here on: the entries' own tests launch through the raw C-ABI
        yield
    finally:
        ops.set_deterministic(False)
        assert _lib.load().dhz_get_deterministic() == 0


def _stream():
    from dehaze_hip import ops
    return ops._stream()          # (hands the workspace to the library on the first call after the switch)


def _wgrad_case(entry, T, nmat, nper, K, scaled, seed):
    """inputs, a launcher onto given targets, and the fp64 reference of one token-Linear weight gradient through the C-ABI"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    N = nmat * nper
    dy = torch.randn(T, N, generator=g).to(dev)
    x = torch.randn(T, K, generator=g).to(dev)
    rps = 512 if T % 512 == 0 else 256
    rs = (0.5 + torch.rand(T // rps, generator=g)).to(dev) if scaled else None

    def launch(dws, dbs):
        pw = (ctypes.c_void_p * nmat)(*[t.data_ptr() for t in dws])
        pb = (ctypes.c_void_p * nmat)(*[t.data_ptr() for t in dbs])
        pw, pb = ctypes.cast(pw, ctypes.c_void_p), ctypes.cast(pb, ctypes.c_void_p)
        lead = (dy.data_ptr(), N, x.data_ptr(), K, T)
        if entry == "split":
            _lib.call("dhz_linear_wgrad_split", *lead, nmat, nper, K, pw, pb, rs.data_ptr() if scaled else None, rps if scaled else 0, 6, _stream())
        elif entry == "multi":
            _lib.call("dhz_linear_wgrad_multi", *lead, nmat, nper, K, pw, pb, _stream())
        elif entry == "rs":
            _lib.call("dhz_linear_wgrad_rs", *lead, nper, K, dws[0].data_ptr(), dbs[0].data_ptr(), rs.data_ptr(), rps, _stream())
        else:
            _lib.call("dhz_linear_wgrad", *lead, nper, K, dws[0].data_ptr(), dbs[0].data_ptr(), _stream())

    d64 = dy.double() * (rs.double().repeat_interleave(rps)[:, None] if scaled else 1.0)
    ref_w, ref_b = d64.t() @ x.double(), d64.sum(0)
    mag = d64.abs().t() @ x.double().abs()
    return launch, ref_w, ref_b, mag


def _run(launch, nmat, nper, K, fill):
    dev = torch.device("cuda:0")
    dws = [torch.full((nper, K), fill, device=dev) for _ in range(nmat)]
    dbs = [torch.full((nper,), -fill, device=dev) for _ in range(nmat)]
    launch(dws, dbs)
    torch.cuda.synchronize()
    return torch.cat(dws, 0), torch.cat(dbs, 0)


def _check_vs_fp64(entry, T, got_w, got_b, ref_w, ref_b, mag, fill):
    ew, eb = (got_w.double() - fill - ref_w).abs(), (got_b.double() + fill - ref_b).abs()
    # a non-zero target adds one rounding of (target + gradient) to the error: half an ulp of the sum
    slack_w = (ref_w.abs() + abs(fill)) * 2.0 ** -24 if fill else 0.0
    slack_b = (ref_b.abs() + abs(fill)) * 2.0 ** -24 if fill else 0.0
    print(f"{entry} T={T}: max dw err {ew.max().item():.3e} (rel. to sum|dy||x|: {(ew / mag).max().item():.3e}), max db err {eb.max().item():.3e}")
    if entry == "split":
        assert (ew <= BOUND6 * mag + 1e-6 + slack_w).all(), (ew / mag).max().item()
        assert (eb <= 1e-5 * ref_b.abs() + 1e-3 * T ** 0.5 + slack_b).all(), eb.max().item()
    elif entry == "rs":
        assert (ew <= 1e-3 + slack_w).all() and (eb <= 1e-3 + slack_b).all(), (ew.max().item(), eb.max().item())
    else:
        assert (ew <= 2e-5 * T ** 0.5 + slack_w).all() and (eb <= 2e-5 * T ** 0.5 + slack_b).all(), (ew.max().item(), eb.max().item())


# (entry, T, nmat, nper, K, scaled): the step's own shapes (T, K, N) = (131072, 128, 384), (524288, 32, 96), (32768, 256, 768),
# (2048, 512, 1536) as the packed Q / K / V launches they are; an embed_dim = 16 shape (csrc/linear_wgrad.hip's narrow kernel); row-scaled
# forms of both kernels; a one-matrix split shape
CASES = [("split", 131072, 3, 128, 128, False), ("multi", 524288, 3, 32, 32, False), ("split", 32768, 3, 256, 256, False),
         ("split", 2048, 3, 512, 512, False), ("plain", 65536, 1, 16, 16, False), ("split", 65536, 1, 256, 64, True),
         ("rs", 1024, 1, 96, 64, True), ("split", 4736, 1, 128, 128, False), ("plain", 32768, 1, 128, 32, False)]


@pytest.mark.parametrize("entry,T,nmat,nper,K,scaled", CASES)
def test_token_linear_wgrad_is_reproducible_and_right(entry, T, nmat, nper, K, scaled):
    launch, ref_w, ref_b, mag = _wgrad_case(entry, T, nmat, nper, K, scaled, seed=T + nper + K)
    with deterministic():
        w0, b0 = _run(launch, nmat, nper, K, 0.0)
        w1, b1 = _run(launch, nmat, nper, K, 0.0)
        assert torch.equal(w0, w1) and torch.equal(b0, b1), "two calls differ"
        for ncu in (8, 9):
            with reserved_grid(ncu):
                w2, b2 = _run(launch, nmat, nper, K, 0.0)
            assert torch.equal(w0, w2) and torch.equal(b0, b2), f"grids sized for {ncu} CUs change the bits"
        _check_vs_fp64(entry, T, w0, b0, ref_w, ref_b, mag, 0.0)
        # the accumulate contract: onto a non-zero target, twice
        w3, b3 = _run(launch, nmat, nper, K, 0.75)
        w4, b4 = _run(launch, nmat, nper, K, 0.75)
        assert torch.equal(w3, w4) and torch.equal(b3, b4), "two calls onto a non-zero target differ"
        _check_vs_fp64(entry, T, w3, b3, ref_w, ref_b, mag, 0.75)
    # (d) switched off: the default route, at its tolerance
    w5, b5 = _run(launch, nmat, nper, K, 0.0)
    _check_vs_fp64(entry, T, w5, b5, ref_w, ref_b, mag, 0.0)


def test_loss_sums_are_reproducible_and_right():
    """dhz_charbonnier_fwd and dhz_l1_pair_fwd (the contrast sums): per-workgroup partials, summed in workgroup order"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    n = 2 * 3 * 256 * 256 + 1024
    a, p, q = (torch.rand(n, generator=g).to(dev) for _ in range(3))

    def run(fill):
        cs = torch.full((1,), fill, device=dev)
        ls = torch.full((2,), fill, device=dev)
        _lib.call("dhz_charbonnier_fwd", a.data_ptr(), p.data_ptr(), None, cs.data_ptr(), n, 1e-3, 1, _stream())
        _lib.call("dhz_l1_pair_fwd", a.data_ptr(), p.data_ptr(), q.data_ptr(), ls.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        return torch.cat([cs, ls])

    ref = torch.stack([(((a.double() - p.double()) ** 2 + 1e-6).sqrt()).sum(), (a.double() - p.double()).abs().sum(),
                       (a.double() - q.double()).abs().sum()])
    with deterministic():
        r0, r1 = run(0.0), run(0.0)
        assert torch.equal(r0, r1)
        with reserved_grid(8):
            assert torch.equal(r0, run(0.0))
        r2, r3 = run(1000.0), run(1000.0)
        assert torch.equal(r2, r3)
    rd = run(0.0)
    for got, fill in ((r0, 0.0), (r2, 1000.0), (rd, 0.0)):
        err = ((got.double() - fill - ref).abs() / n).max().item()
        print(f"loss sums: error of the means {err:.3e}")
        # tests/test_gpu_kernels.py: the mean within 1e-6; onto a non-zero target, plus one rounding of (target + sum)
        assert err < 1e-6 + (ref.max().item() + fill) * 2.0 ** -24 / n * (fill != 0.0), err


def _step_run(steps, ncu):
    """`steps` training steps of a freshly built model from fixed seeds; returns (losses, parameters, last flat gradient)"""
    import My_CR
    import My_model_1 as M1
    from dehaze_hip.train import FlatAdamW, synthetic_batch, train_step
    from losses import CharbonnierLoss
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(4321)
        cr = My_CR.ContrastLoss().to(dev)
    opt = FlatAdamW(model)
    gt, hazy = synthetic_batch(2, 128, seed=5)
    gt, hazy = gt.to(dev), hazy.to(dev)
    model.train()
    losses = []
    with reserved_grid(ncu):
        for step in range(steps):
            torch.manual_seed(1000 + step)
            loss, _, _ = train_step(model, CharbonnierLoss(), cr, opt, None, hazy, gt)
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
    return torch.stack(losses), opt._flat["p"].clone(), opt._flat["g"].clone()


def test_whole_step_repeats_bit_for_bit():
    """Uformer E = 32, 128 x 128, batch 2 (DropPath on), Charbonnier + CR + FlatAdamW, 10 steps: twice on the whole device, once on grids sized
    for 8 CUs"""
    with deterministic():
        runs = [_step_run(10, None), _step_run(10, None), _step_run(10, 8)]
    l0, p0, g0 = runs[0]
    assert torch.isfinite(l0).all()
    for tag, (l, p, g) in zip(("second run", "8 CUs"), runs[1:]):
        assert torch.equal(l0, l), (tag, (l0 - l).abs().max().item())
        assert torch.equal(g0, g), (tag, (g0 - g).abs().max().item())
        assert torch.equal(p0, p), (tag, (p0 - p).abs().max().item())


def test_deterministic_steps_vs_oracle():
    """the mode computes what the default path computes: tests/test_gpu_model.py's three AdamW steps against the CPU oracle, as they are"""
    import test_gpu_model
    with deterministic():
        test_gpu_model.test_training_steps_vs_oracle(torch.device("cuda:0"))


def test_refusals_are_argument_checks():
    from dehaze_hip import _lib, ops
    dev = torch.device("cuda:0")
    T, N, K = 4096, 128, 128
    dy, x = torch.randn(T, N, device=dev), torch.randn(T, K, device=dev)
    dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
    lib = _lib.load()
    with deterministic():
        # bf16 storage: outside the mode, in Python and in the library
        w = torch.nn.Parameter(torch.zeros(N, K, device=dev))
        with pytest.raises(NotImplementedError, match="deterministic"):
            ops.linear_wgrad(dy.to(torch.bfloat16), 0, x.to(torch.bfloat16), [(w, None)])
        pw = ctypes.cast((ctypes.c_void_p * 1)(dw.data_ptr()), ctypes.c_void_p)
        assert lib.dhz_linear_wgrad_bf16(dy.data_ptr(), N, x.data_ptr(), K, T, 1, N, K, pw, None, _stream()) == -22
        assert b"deterministic" in lib.dhz_last_error()
    with deterministic(workspace_bytes=4096):
        # an undersized workspace: an error that names the bytes needed (slabs x (N K + N) floats), nothing launched
        rc = lib.dhz_linear_wgrad(dy.data_ptr(), N, x.data_ptr(), K, T, N, K, dw.data_ptr(), db.data_ptr(), _stream())
        msg = lib.dhz_last_error().decode()
        assert rc == -22, rc
        m = re.search(r"workspace of (\d+) bytes \((\d+) items x (\d+) floats\)", msg)
        assert m, msg
        assert int(m.group(3)) == N * K + N and int(m.group(1)) == 4 * int(m.group(2)) * int(m.group(3)) and int(m.group(2)) > 1, msg
        torch.cuda.synchronize()
        assert not dw.any() and not db.any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The other converted entries, each through the raw C-ABI.  A case gives: launch(targets) -> overwritten outputs, the targets' shapes, the
# fp64 references and the (atol, rtol) of the entry's own default-mode test (|got - ref| <= atol + rtol |ref|, as torch.allclose).
def _check_accumulating_entry(name, launch, shapes, refs, tols):
    dev = torch.device("cuda:0")

    def run(fill):
        targets = [torch.full(s, fill, device=dev) for s in shapes]
        extra = launch(targets) or []
        torch.cuda.synchronize()
        return targets + list(extra)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    def check(got, fill, tag):
        for k, (ref, (atol, rtol)) in enumerate(zip(refs, tols)):
            err = (got[k].double().cpu() - fill - ref).abs()
            # a non-zero target adds one rounding of (target + gradient): half an ulp of the sum
            slack = (ref.abs() + abs(fill)) * 2.0 ** -24 if fill else 0.0
            print(f"{name} {tag} target {k}: max err {err.max().item():.3e} (max |ref| {ref.abs().max().item():.3e})")
            assert (err <= atol + rtol * ref.abs() + slack).all(), (name, tag, k, err.max().item())

    with deterministic():
        r0, r1 = run(0.0), run(0.0)
        assert same(r0, r1), f"{name}: two calls differ"
        for ncu in (8, 9):
            with reserved_grid(ncu):
                r2 = run(0.0)
            assert same(r0, r2), f"{name}: grids sized for {ncu} CUs change the bits"
        check(r0, 0.0, "mode on")
        r3, r4 = run(0.5), run(0.5)
        assert same(r3, r4), f"{name}: two calls onto a non-zero target differ"
        check(r3, 0.5, "mode on, onto 0.5")
    check(run(0.0), 0.0, "mode off")


def _s():
    return torch.cuda.current_stream().cuda_stream


# (2, 64, 64, 32, 64): 16 token slabs; (2, 32, 32, 64, 128): more tiles, fewer tokens; (4, 128, 128, 32, 64): the E = 32 model's first
# down-sampling at batch 4
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 64, 64, 32, 64), (2, 32, 32, 64, 128), (4, 128, 128, 32, 64)])
def test_conv4s2_wgrad(B, H, W, Cin, Cout):
    """tolerances: tests/test_gpu_conv.py::test_conv4s2_c_abi"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B + H + W + Cin)
    x = torch.randn(B, H * W, Cin, generator=g)
    gy = torch.randn(B, Cout, H // 2, W // 2, generator=g)
    w64 = torch.zeros(Cout, Cin, 4, 4, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().view(B, H, W, Cin).permute(0, 3, 1, 2), w64, b64, stride=2, padding=1).backward(gy.double())
    dwref = w64.grad.permute(0, 2, 3, 1).reshape(Cout, 16 * Cin)
    xd, dy = x.to(dev), gy.permute(0, 2, 3, 1).reshape(B, -1, Cout).contiguous().to(dev)
    T = B * (H // 2) * (W // 2)

    def launch(t):
        _lib.call("dhz_conv4s2_wgrad", dy.data_ptr(), xd.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), B, H, W, Cin, Cout, _s())

    tol_w = 3e-6 * T ** 0.5 * max(1.0, dwref.abs().max().item() / T ** 0.5) + 1e-4
    _check_accumulating_entry("conv4s2_wgrad", launch, [(Cout, 16 * Cin), (Cout,)], [dwref, b64.grad],
                              [(tol_w, 0.0), (3e-5 * T ** 0.5 + 1e-4, 0.0)])


# ragged tiles; more 8 x 16 tiles (640) than workgroups of the persistent grid; two channel chunks per tile
@pytest.mark.parametrize("B,H,W,C", [(3, 9, 21, 64), (5, 128, 128, 64), (2, 24, 40, 128)])
def test_thin_conv3x3_wgrad(B, H, W, C):
    """tolerances: tests/test_gpu_kernels.py::test_thin_conv3x3_vs_torch"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.randn(B, H * W, C, generator=g)
    gy = torch.randn(B, 3, H, W, generator=g)
    w64 = torch.zeros(3, C, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().view(B, H, W, C).permute(0, 3, 1, 2), w64, b64, padding=1).backward(gy.double())
    xd, dy = x.to(dev), gy.to(dev)

    def launch(t):
        _lib.call("dhz_thin_conv3x3_wgrad", dy.data_ptr(), xd.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), B, H, W, C, _s())

    scale = max(1.0, (B * H * W / 1000.0) ** 0.5)
    _check_accumulating_entry("thin_conv3x3_wgrad", launch, [(3, C, 3, 3), (3,)], [w64.grad, b64.grad], [(2e-4 * scale, 1e-4)] * 2)


# maps that are no multiple of the 16 x 16 tile; both widths; the training map
@pytest.mark.parametrize("B,H,W,E", [(2, 32, 32, 32), (1, 48, 40, 64), (2, 128, 128, 32)])
def test_input_proj_bwd(B, H, W, E):
    """tolerances: tests/test_gpu_conv.py::test_input_proj_vs_torch.  The LeakyReLU mask is the sign of the forward output the entry is
    given, so the reference uses the same one."""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B + H + E)
    img = torch.rand(B, 3, H, W, generator=g)
    w = torch.randn(E, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(E, generator=g) * 0.1
    gout = torch.randn(B, H * W, E, generator=g)
    imgd, dy = img.to(dev), gout.to(dev)
    y = torch.empty(B, H * W, E, device=dev)
    _lib.call("dhz_input_proj_fwd", imgd.data_ptr(), w.to(dev).data_ptr(), b.to(dev).data_ptr(), y.data_ptr(), B, H, W, E, 0.01, _s())
    slope = torch.where(y.cpu() > 0, 1.0, 0.01).double()
    w64 = torch.zeros(E, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    b64 = torch.zeros(E, dtype=torch.float64, requires_grad=True)
    dpre = (gout.double() * slope).view(B, H, W, E).permute(0, 3, 1, 2)
    F.conv2d(img.double(), w64, b64, padding=1).backward(dpre)
    T = B * H * W

    def launch(t):
        _lib.call("dhz_input_proj_bwd", dy.data_ptr(), y.data_ptr(), imgd.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), B, H, W, E, 0.01, _s())

    tol_w = 3e-6 * T ** 0.5 * max(1.0, w64.grad.abs().max().item() / T ** 0.5) + 1e-4
    _check_accumulating_entry("input_proj_bwd", launch, [(E, 3, 3, 3), (E,)], [w64.grad, b64.grad],
                              [(tol_w, 0.0), (3e-5 * T ** 0.5 + 1e-4, 0.0)])


# every channel-width path of the kernel (32 ... 512), shifted and not, plain LayerNorm (partition 0), and a map of 8192 tokens
@pytest.mark.parametrize("C,res,shift,partition", [(32, 16, 4, 1), (64, 32, 4, 1), (128, 16, 0, 0), (512, 8, 0, 1), (32, 64, 0, 1)])
def test_ln_partition_bwd(C, res, shift, partition):
    """tolerances: tests/test_gpu_kernels.py::test_ln_partition"""
    from dehaze_hip import _lib
    from oracle import uformer_oracle as O
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(C + res + shift)
    B = 2
    x = torch.randn(B, res * res, C, generator=g) * 2 + 0.5
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    go = torch.randn(B * res * res, C, generator=g)
    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.layer_norm(x64, (C,), g64, b64, 1e-5).view(B, res, res, C)
    if partition:
        if shift:
            y = torch.roll(y, (-shift, -shift), (1, 2))
        y = O.window_partition(y, 8)
    (y.reshape(-1, C) * go.double()).sum().backward()
    xd, gd, bd, dxw = x.to(dev), gamma.to(dev), beta.to(dev), go.to(dev)
    xw = torch.empty(B * res * res, C, device=dev)
    stats = torch.empty(B * res * res, 2, device=dev)
    _lib.call("dhz_ln_partition_fwd", xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), xw.data_ptr(), stats.data_ptr(), B, res, res, C, shift,
              partition, _s())

    def launch(t):
        dx = torch.empty(B, res * res, C, device=dev)
        _lib.call("dhz_ln_partition_bwd", dxw.data_ptr(), xd.data_ptr(), gd.data_ptr(), stats.data_ptr(), None, dx.data_ptr(),
                  t[0].data_ptr(), t[1].data_ptr(), B, res, res, C, shift, partition, _s())
        return [dx]

    _check_accumulating_entry("ln_partition_bwd", launch, [(C,), (C,)], [g64.grad, b64.grad], [(2e-4, 1e-3)] * 2)


# (Ch, res, per-image factors): the LeFF widths of the model (4 C), a map that is no multiple of 16, the 8-lane width, and the DropPath form
@pytest.mark.parametrize("Ch,res,scaled", [(128, 16, False), (64, 24, False), (96, 16, False), (256, 32, False), (128, 64, False),
                                           (64, 16, True), (128, 32, True)])
def test_leff_dwconv_bwd(Ch, res, scaled):
    """tolerances: tests/test_gpu_kernels.py::test_leff_dwconv; the scaled form (dhz_leff_dwconv_bwd_scaled_dt, a factor per image on dz)
    against the same reference on the pre-scaled gradient"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(Ch + res)
    B = 4 if scaled else 2
    u = torch.randn(B, res * res, Ch, generator=g)
    w = 0.3 * torch.randn(Ch, 1, 3, 3, generator=g)
    b = 0.1 * torch.randn(Ch, generator=g)
    go = torch.randn(B, res * res, Ch, generator=g)
    sc = torch.tensor([0.0, 1.25, 1.0, 1.111])
    u64, w64, b64 = u.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    m = F.gelu(u64).transpose(1, 2).reshape(B, Ch, res, res)
    z = F.gelu(F.conv2d(m, w64, b64, padding=1, groups=Ch)).flatten(2).transpose(1, 2)
    (z * (go.double() * sc.double().view(B, 1, 1) if scaled else go.double())).sum().backward()
    ud, wd, dz, scd = u.to(dev), w.to(dev), go.to(dev), sc.to(dev)
    tp, zd = torch.empty_like(ud), torch.empty_like(ud)
    _lib.call("dhz_leff_dwconv_fwd", ud.data_ptr(), wd.data_ptr(), b.to(dev).data_ptr(), tp.data_ptr(), zd.data_ptr(), B, res, res, Ch, _s())

    def launch(t):
        du = torch.empty_like(ud)
        lead = (dz.data_ptr(), ud.data_ptr(), tp.data_ptr(), wd.data_ptr(), du.data_ptr(), t[0].data_ptr(), t[1].data_ptr())
        if scaled:
            _lib.call("dhz_leff_dwconv_bwd_scaled_dt", *lead, scd.data_ptr(), B, res, res, Ch, 0, _s())
        else:
            _lib.call("dhz_leff_dwconv_bwd", *lead, B, res, res, Ch, _s())
        return [du]

    _check_accumulating_entry("leff_dwconv_bwd" + ("_scaled" if scaled else ""), launch, [(Ch * 9,), (Ch,)],
                              [w64.grad.reshape(Ch * 9), b64.grad], [(3e-4, 1e-3)] * 2)


def _table_ref(part, H):
    from oracle import uformer_oracle as O
    ridx = O.relative_position_index(8).reshape(-1).long()
    p64 = part.double().cpu()
    ref = torch.zeros(225, H, dtype=torch.float64)
    for h in range(H):
        ref[:, h].index_add_(0, ridx, p64[h::H].sum(0).reshape(-1))
    return ref


# (windows, heads, head_dim): the part counts are the ones dhz_ps_attn_bwd hands over for these shapes
@pytest.mark.parametrize("B_,H,d", [(512, 1, 32), (128, 4, 32), (32, 16, 32)])
def test_bias_table_grad(B_, H, d):
    """dhz_bias_table_grad (accumulate = 1) and dhz_bias_table_grad_multi on the same partial tiles.  Tolerance: the table-gradient line of
    tests/test_gpu_kernels.py::test_ps_attention_oracle at its one-window value (atol 2e-4, rtol 2e-3)"""
    from dehaze_hip import _lib
    dev = torch.device("cuda:0")
    parts = _lib.load().dhz_ps_attn_bwd_parts_d(B_, H, d)
    assert parts > H and parts % H == 0, parts
    g = torch.Generator().manual_seed(B_ + H)
    part = torch.randn(parts, 64, 64, generator=g).to(dev)
    part2 = torch.randn(2 * H, 64, 64, generator=g).to(dev)
    ref, ref2 = _table_ref(part, H), _table_ref(part2, H)

    def single(t):
        _lib.call("dhz_bias_table_grad", part.data_ptr(), parts, t[0].data_ptr(), H, 1, _s())

    def multi(t):
        pp = (ctypes.c_void_p * 2)(part.data_ptr(), part2.data_ptr())
        pt = (ctypes.c_void_p * 2)(t[0].data_ptr(), t[1].data_ptr())
        np_, nh = (ctypes.c_int * 2)(parts, 2 * H), (ctypes.c_int * 2)(H, H)
        _lib.call("dhz_bias_table_grad_multi", ctypes.cast(pp, ctypes.c_void_p), ctypes.cast(np_, ctypes.c_void_p),
                  ctypes.cast(pt, ctypes.c_void_p), ctypes.cast(nh, ctypes.c_void_p), 2, _s())

    _check_accumulating_entry("bias_table_grad", single, [(225, H)], [ref], [(2e-4, 2e-3)])
    _check_accumulating_entry("bias_table_grad_multi", multi, [(225, H)] * 2, [ref, ref2], [(2e-4, 2e-3)] * 2)
    # accumulate = 0 overwrites whatever the target held
    with deterministic():
        dt = torch.full((225, H), 7.0, device=dev)
        _lib.call("dhz_bias_table_grad", part.data_ptr(), parts, dt.data_ptr(), H, 0, _s())
        torch.cuda.synchronize()
        assert ((dt.double().cpu() - ref).abs() <= 2e-4 + 2e-3 * ref.abs()).all()
