"""-m gpu: SSIM / PSNR scored on the device in float64 (dhz_ssim_pair, dhz_ssim_pair_workspace_bytes; dehaze_hip/metrics.py, the drop-in
metrics.py, FFA_main.py --metrics, eval_any_resolution.py --gpu_metrics).

Oracles.  FFA form: a float64 torch-CPU evaluation of FFA_model/metrics.py's formula written out below (F.conv2d in double with the
fp32-built 2-D window), and the reference's own values in tests/golden/ffa_metrics.npz.  Uniform form: utils/metrics.py on host copies.

Bound.  |device - oracle| <= 1e-9 absolute for every per-plane SSIM mean and every reported SSIM; squared-error sums within 1e-12
relative, so PSNR within 1e-9 dB.  Double unit round-off is 1.1e-16, each moment is a sum of K^2 <= 121 terms <= 1, the variances lose
nothing relative to that by cancellation, the smallest denominator factor is C2 = 9e-4: about 1e-10 per pixel, 1e-9 leaves one decade.
The squared-error oracle forms its terms as the kernel must (fp32 subtraction, fp32 square) and adds them in double.  Against the
reference's fp32 `psnr` (numpy's float32 mean: a few fp32 roundings, 6e-8 relative each, 4.3 dB per unit of relative error) the bound is
1e-5 dB.
"""
import glob
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
DEV = "cuda:0"
TOL, RTOL_SQ = 1e-9, 1e-12

FFA_SHAPES = [(1, 3, 5, 9), (1, 1, 11, 11), (2, 3, 33, 47), (1, 3, 64, 64), (1, 3, 130, 70)]
UNI_SHAPES = [(1, 3, 7, 7), (1, 3, 8, 13), (2, 3, 33, 47), (1, 3, 64, 64), (1, 3, 130, 70)]
CONTENTS = ("noise", "smooth", "near_constant", "identical", "range")


def make_pair(kind, shape, seed=0):
    """(pred, gt) fp32 CPU tensors"""
    g = torch.Generator().manual_seed(1000 + seed)
    B, C, H, W = shape
    if kind == "noise":
        gt = torch.rand(shape, generator=g)
        return gt + 0.1 * torch.randn(shape, generator=g), gt
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
        ph = torch.arange(float(B * C)).view(B, C, 1, 1)
        gt = (0.5 + 0.45 * torch.sin(0.21 * yy + ph) * torch.sin(0.13 * xx + 0.5 * ph)).float()
        return (0.9 * gt + 0.05 + 0.01 * torch.randn(shape, generator=g)).float(), gt
    if kind == "near_constant":
        return 0.7 + 0.002 * torch.randn(shape, generator=g), torch.full(shape, 0.7)
    if kind == "identical":
        gt = torch.rand(shape, generator=g)
        return gt.clone(), gt
    if kind == "range":
        gt = -0.2 + 1.5 * torch.rand(shape, generator=g)
        return (gt + 0.2 * torch.randn(shape, generator=g)).clamp(-0.2, 1.3), gt
    if kind == "negative":                       # a target with negative values: the uniform PSNR's data_range = 2
        gt = torch.rand(shape, generator=g) - 0.5
        return (gt + 0.05 * torch.randn(shape, generator=g)).clamp(-1, 1), gt
    raise KeyError(kind)


def sq_oracle(a, b):
    """[B, C] squared-error sums: fp32 subtraction and fp32 square, added in double"""
    d = a - b
    assert d.dtype == torch.float32
    return (d * d).double().sum(dim=(2, 3))


def ffa_oracle(a, b, clamp=True, dtype=torch.float64):
    """FFA_model/metrics.py:31-58 in `dtype`: (per-plane map means [B, C], squared-error sums [B, C])"""
    from dehaze_hip.metrics import window_table
    if clamp:
        a, b = a.clamp(0, 1), b.clamp(0, 1)
    C = a.shape[1]
    w = window_table(11).to(dtype).expand(C, 1, 11, 11).contiguous()
    x, y = a.to(dtype), b.to(dtype)
    conv = lambda t: F.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return m.double().mean(dim=(2, 3)), sq_oracle(a, b)


def uniform_oracle(pred, gt):
    """utils/metrics.py on host copies, as FFA_main.evaluate calls it: per image (ssim, psnr) and the per-plane SSIM means [B, C]"""
    from utils.metrics import _ssim_plane, peak_signal_noise_ratio, structural_similarity
    out, planes = [], []
    for p, t in zip(pred, gt):
        a, b = t.permute(1, 2, 0).numpy(), p.permute(1, 2, 0).numpy()
        with np.errstate(divide="ignore"):
            out.append((structural_similarity(a, b, multichannel=True), float(peak_signal_noise_ratio(a, b))))
        planes.append([_ssim_plane(a[..., c], b[..., c], 7, 2.0) for c in range(a.shape[-1])])
    return out, torch.tensor(planes, dtype=torch.float64)


def ffa_sums(pred, gt, clamp=True):
    from dehaze_hip import metrics as DM
    return DM.pair_sums(pred, gt, 11, False, 0.01 ** 2, 0.03 ** 2, 1.0, clamp, DM._table("gauss", pred.device))


def uniform_sums(pred, gt):
    from dehaze_hip import metrics as DM
    return DM.pair_sums(gt, pred, 7, True, 0.02 ** 2, 0.06 ** 2, 49 / 48.0, False, DM._table("ones", pred.device), 1.0 / 49)


def check_sq(dev_e, ref_e):
    err = (dev_e.cpu() - ref_e).abs()
    assert bool((err <= RTOL_SQ * ref_e).all()), (dev_e.cpu(), ref_e)


@pytest.mark.parametrize("shape", FFA_SHAPES + ["slice"], ids=str)
def test_ffa_form_against_float64(shape):
    """zero-padded K = 11 on every content, clamp on; per-plane means, the wrappers' values, the identical pair's exact values, and in
    the near-constant case that an fp32 evaluation is NOT within the bound (the case separates an fp32 kernel from a float64 one)"""
    import metrics as M
    from dehaze_hip import metrics as DM
    sliced = shape == "slice"
    shp = (2, 3, 33, 35) if sliced else shape
    for i, kind in enumerate(CONTENTS):
        pred, gt = make_pair(kind, shp, i)
        dp, dg = pred.to(DEV), gt.to(DEV)
        if sliced:                                   # image 1 of a stacked batch: starts 13 860 bytes into the allocation
            pred, gt, dp, dg = pred[1:2], gt[1:2], dp[1:2], dg[1:2]
            assert dp.data_ptr() % 16 != 0 and dp.data_ptr() - dp._base.data_ptr() == 13860
        B, C, H, W = pred.shape
        ref_s, ref_e = ffa_oracle(pred, gt)
        s, e = ffa_sums(dp, dg)
        assert s.dtype == e.dtype == torch.float64 and s.shape == e.shape == (B, C)
        err = ((s / (H * W)).cpu() - ref_s).abs().max().item()
        print(f"ffa {tuple(pred.shape)} {kind}: per-plane ssim err {err:.3e}")
        assert err <= TOL, (kind, err)
        check_sq(e, ref_e)
        whole = M.ssim(dp, dg)
        assert whole.is_cuda and whole.dtype == torch.float64 and abs(whole.item() - ref_s.mean().item()) <= TOL
        per = M.ssim(dp, dg, size_average=False)
        assert per.shape == (B,) and (per.cpu() - ref_s.mean(1)).abs().max().item() <= TOL
        mse = ref_e.sum().item() / pred.numel()
        p = M.psnr(dp, dg)
        if kind == "identical":
            assert p == 100 and bool((e == 0).all())
            assert (s / (H * W) - 1).abs().max().item() <= 1e-15 and abs(whole.item() - 1) <= 1e-15
        else:
            assert abs(p - 20 * math.log10(1 / math.sqrt(mse))) <= TOL
        if kind == "near_constant" and (H, W) == (33, 47):
            f32 = DM.ssim_gauss(pred, gt).item()                      # the reference's ATen fp32 evaluation, on the CPU
            print(f"near-constant: fp32 evaluation is {abs(f32 - ref_s.mean().item()):.3e} from float64")
            assert abs(f32 - ref_s.mean().item()) > 1e-6


@pytest.mark.parametrize("shape", UNI_SHAPES, ids=str)
def test_uniform_form_against_utils_metrics(shape):
    """valid K = 7 against utils/metrics.py on the host copies"""
    from dehaze_hip import metrics as DM
    B, C, H, W = shape
    for i, kind in enumerate(("noise", "smooth", "near_constant", "identical", "negative")):
        pred, gt = make_pair(kind, shape, 10 + i)
        if kind != "negative":
            pred = pred.clamp(0, 1)                  # evaluate() scores the clamped prediction
        dp, dg = pred.to(DEV), gt.to(DEV)
        ref, ref_planes = uniform_oracle(pred, gt)
        s, e = uniform_sums(dp, dg)
        err = ((s / ((H - 6) * (W - 6))).cpu() - ref_planes).abs().max().item()
        print(f"uniform {shape} {kind}: per-plane ssim err {err:.3e}")
        assert err <= TOL, (kind, err)
        check_sq(e, sq_oracle(gt, pred))
        sc = DM.Scores()
        sc.add_uniform(dp, dg)
        ss, pp = sc.read()
        for b in range(B):
            assert abs(ss[b] - ref[b][0]) <= TOL
            if kind == "identical":
                assert pp[b] == float("inf") and abs(ss[b] - 1) <= 1e-15
            else:
                assert abs(pp[b] - ref[b][1]) <= TOL, (kind, pp[b], ref[b][1])
        if kind == "negative":
            assert float(gt.min()) < 0                # data_range 2: 6.02 dB above the data_range 1 value
            mse = (sq_oracle(gt, pred).sum(1) / (C * H * W))
            assert abs(pp[0] - 10 * math.log10(4 / mse[0].item())) <= TOL
        assert abs(DM.ssim_uniform(dp, dg) - np.mean([r[0] for r in ref])) <= TOL
        if kind != "identical":
            assert abs(DM.psnr_uniform(dp, dg) - np.mean([r[1] for r in ref])) <= TOL


def test_valid_form_refuses_planes_smaller_than_the_window():
    from dehaze_hip import _lib, metrics as DM
    lib = _lib.load()
    x = torch.rand(1, 3, 6, 40, device=DEV)
    out = torch.zeros(2, 3, dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    need = lib.dhz_ssim_pair_workspace_bytes(1, 3, 6, 40)
    assert 0 < need <= ws.numel() * 8
    rc = lib.dhz_ssim_pair(out[0].data_ptr(), out[1].data_ptr(), x.data_ptr(), 720, 240, x.data_ptr(), 720, 240, 1, 3, 6, 40, 7,
                           DM._table("ones", x.device).data_ptr(), 1 / 49.0, 1, 4e-4, 36e-4, 49 / 48.0, 0, ws.data_ptr(), need, None)
    assert rc == -22 and b"valid rule" in lib.dhz_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not ws.any()
    with pytest.raises(ValueError):
        uniform_sums(x, x)
    with pytest.raises(ValueError):
        DM.ssim_uniform(x, x)
    assert abs(DM.ssim_gauss(x, x).item() - 1) <= 1e-15          # the zero-padded form takes it


def test_raw_entry_writes_nothing_outside_its_outputs_and_workspace():
    """the C entry with NaN floats behind the inputs' ends, the outputs and the workspace: every guard stays NaN, the values are the
    wrapper's"""
    from dehaze_hip import _lib, metrics as DM
    lib = _lib.load()
    B, C, H, W = 2, 3, 70, 45
    pred, gt = make_pair("noise", (B, C, H, W), 77)
    n = B * C * H * W
    bufs = []
    for t in (pred, gt):
        buf = torch.full((n + 64,), float("nan"), device=DEV)
        buf[:n] = t.reshape(-1).to(DEV)
        bufs.append(buf)
    need = lib.dhz_ssim_pair_workspace_bytes(B, C, H, W)
    assert need == B * C * 2 * 2 * 16
    ws = torch.full((need // 8 + 16,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((2, B * C + 8), float("nan"), dtype=torch.float64, device=DEV)
    for K, valid, kind, wscale, c1, c2, cov in ((11, 0, "gauss", 1.0, 1e-4, 9e-4, 1.0), (7, 1, "ones", 1 / 49.0, 4e-4, 36e-4, 49 / 48.0)):
        rc = lib.dhz_ssim_pair(out[0].data_ptr(), out[1].data_ptr(), bufs[0].data_ptr(), C * H * W, H * W, bufs[1].data_ptr(), C * H * W, H * W,
                               B, C, H, W, K, DM._table(kind, torch.device(DEV)).data_ptr(), wscale, valid, c1, c2, cov, 0, ws.data_ptr(), need,
                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.dhz_last_error()
        torch.cuda.synchronize()
        assert bool(out[:, B * C:].isnan().all()) and bool(ws[need // 8:].isnan().all()) and not bool(ws[:need // 8].isnan().any())
        s, e = DM.pair_sums(pred.to(DEV), gt.to(DEV), K, valid, c1, c2, cov, False, DM._table(kind, torch.device(DEV)), wscale)
        assert torch.equal(out[0, :B * C].view(B, C), s) and torch.equal(out[1, :B * C].view(B, C), e)
    assert all(bool(b[n:].isnan().all()) for b in bufs)


def test_golden_pairs_of_the_reference(golden):
    """the reference's own float64 evaluation (tests/golden/ffa_metrics.npz) to 1e-9; its fp32 psnr to 1e-5 dB (module docstring)"""
    import metrics as M
    g = golden("ffa_metrics")
    for name in ("noise", "smooth", "range"):
        pred, gt = torch.from_numpy(g[name + "_pred"]).to(DEV), torch.from_numpy(g[name + "_gt"]).to(DEV)
        assert abs(M.ssim(pred, gt).item() - float(g[name + "_ssim_f64"])) <= TOL
        assert np.abs(M.ssim(pred, gt, size_average=False).cpu().numpy() - g[name + "_ssim_per_image_f64"]).max() <= TOL
        assert abs(M.psnr(pred, gt) - float(g[name + "_psnr_f32"])) <= 1e-5


def test_out_of_range_pair_with_the_clamp_on_and_off():
    for shape in ((1, 3, 5, 9), (2, 3, 33, 47)):
        pred, gt = make_pair("range", shape, 5)
        assert float(gt.min()) < 0 and float(pred.max()) > 1
        H, W = shape[2:]
        res = {}
        for clamp in (True, False):
            ref_s, ref_e = ffa_oracle(pred, gt, clamp)
            s, e = ffa_sums(pred.to(DEV), gt.to(DEV), clamp)
            assert ((s / (H * W)).cpu() - ref_s).abs().max().item() <= TOL
            check_sq(e, ref_e)
            res[clamp] = s
        assert (res[True] - res[False]).abs().max().item() > 1e-3 * H * W


def test_bits_are_reproducible():
    """two runs, two dhz_set_reserved_cus levels, the deterministic mode on: bit-equal doubles"""
    from dehaze_hip import _lib, ops
    pred, gt = make_pair("noise", (2, 3, 130, 70), 9)
    dp, dg = pred.to(DEV), gt.to(DEV)
    runs = [ffa_sums(dp, dg) + uniform_sums(dp, dg) for _ in range(2)]
    for level in (64, 100):
        try:
            _lib.call("dhz_set_reserved_cus", level)
            runs.append(ffa_sums(dp, dg) + uniform_sums(dp, dg))
        finally:
            _lib.call("dhz_set_reserved_cus", 0)
    try:
        ops.set_deterministic(True, workspace_bytes=1 << 20)
        runs.append(ffa_sums(dp, dg) + uniform_sums(dp, dg))
    finally:
        ops.set_deterministic(False)
    for other in runs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other))


def test_scores_reads_back_once(monkeypatch):
    """five images of two sizes: one read-back, the per-image calls' values"""
    from dehaze_hip import metrics as DM
    pairs = [make_pair("noise", (1, 3, 33, 47) if i % 2 else (1, 3, 20, 70), 20 + i) for i in range(5)]
    pairs = [(p.clamp(0, 1).to(DEV), g.to(DEV)) for p, g in pairs]
    want_u = [(DM.ssim_uniform(p, g), DM.psnr_uniform(p, g)) for p, g in pairs]
    want_f = [(DM.ssim_gauss(p, g).item(), DM.psnr_ffa(p, g)) for p, g in pairs]
    copies = []
    real_cpu, real_item, real_tolist = torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (copies.append("cpu") if t.is_cuda else None, real_cpu(t, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda t: (copies.append("item") if t.is_cuda else None, real_item(t))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: (copies.append("tolist") if t.is_cuda else None, real_tolist(t))[1])
    su, sf = DM.Scores(), DM.Scores()
    for p, g in pairs:
        su.add_uniform(p, g)
        sf.add_ffa(p, g)
    assert copies == [] and len(su) == len(sf) == 5
    (us, up), (fs, fp) = su.read(), sf.read()
    assert copies == ["cpu", "cpu"] and su.readbacks == sf.readbacks == 1
    monkeypatch.undo()
    for i in range(5):
        assert us[i] == want_u[i][0] and abs(up[i] - want_u[i][1]) <= 1e-12
        assert fs[i] == want_f[i][0] and abs(fp[i] - want_f[i][1]) <= 1e-12


def test_evaluate_in_process():
    """FFA(3, 2) on 2 synthetic 35 x 50 pairs: `device` equals `host` to 1e-9; `ffa` equals the drop-in's float64 CPU evaluation of the same
    predictions to 1e-9"""
    import FFA_main
    import metrics as M
    from dehaze_hip.ffa import FFA
    from dehaze_hip.train import synthetic_batch
    torch.manual_seed(11)
    net = FFA(gps=3, blocks=2).to(DEV)
    vt, vi = synthetic_batch(2, (35, 50), seed=4321, device=DEV)
    host = FFA_main.evaluate(net, vt, vi)
    assert FFA_main.evaluate(net, vt, vi, "host") == host
    dev = FFA_main.evaluate(net, vt, vi, "device")
    print("evaluate host", host, "device", dev)
    assert abs(dev[0] - host[0]) <= TOL and abs(dev[1] - host[1]) <= TOL
    ffa = FFA_main.evaluate(net, vt, vi, "ffa")
    net.eval()
    with torch.no_grad():
        preds = [net(x[None]).cpu().double() for x in vi]
    net.train()
    want_s = np.mean([M.ssim(p, t[None].cpu().double()).item() for p, t in zip(preds, vt)])
    want_p = np.mean([M.psnr(p.float(), t[None].cpu()) for p, t in zip(preds, vt)])       # fp32 terms, as the kernel forms them
    print("evaluate ffa", ffa, "float64 CPU", (want_s, want_p))
    assert abs(ffa[0] - want_s) <= TOL and abs(ffa[1] - want_p) <= 1e-5
    sq = [sq_oracle(p.float().clamp(0, 1), t[None].cpu().clamp(0, 1)).sum().item() / p.numel() for p, t in zip(preds, vt)]
    assert abs(ffa[1] - np.mean([20 * math.log10(1 / math.sqrt(m)) for m in sq])) <= TOL
    with pytest.raises(ValueError):
        FFA_main.evaluate(net, vt, vi, "fp32")


def _ffa_main(tmp_path, mode):
    mdir = str(tmp_path / mode) + os.sep
    cmd = [sys.executable, "FFA_main.py", "--blocks", "2", "--bs", "2", "--crop_size", "64", "--synthetic", "4", "--val_synthetic", "2",
           "--steps", "2", "--eval_step", "1", "--deterministic", "--model_dir", mdir, "--metrics", mode]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(mdir, "My_NH_ffa_3_2_*_psnr: *_ssim: *.pk")))
    assert len(names) == 2, os.listdir(mdir)
    ck = torch.load(os.path.join(mdir, names[-1]), map_location="cpu")
    assert set(ck) == {"step", "max_psnr", "max_ssim", "ssims", "psnrs", "losses", "model"} and ck["step"] == 2
    lines = re.findall(r"step :(\d+) \|ssim:([0-9.]+)\| psnr:([0-9.]+)", r.stdout)
    return names, ck, lines


def test_ffa_main_device_metrics_match_host(tmp_path):
    """--metrics device / host from one seed (--deterministic: the two runs train the same weights): stored ssims / psnrs agree to 1e-9, the
    printed lines are equal, and the checkpoints carry the same names - the pattern and step literally, the two numbers a name spells out
    in full (str of a double) to the same 1e-9, which is as identical as two summation orders can be"""
    nh, ckh, lh = _ffa_main(tmp_path, "host")
    nd, ckd, ld = _ffa_main(tmp_path, "device")
    assert len(ckh["ssims"]) == len(ckd["ssims"]) == 2 and ckh["losses"] == ckd["losses"]
    for k in ("ssims", "psnrs"):
        assert np.abs(np.asarray(ckh[k]) - np.asarray(ckd[k])).max() <= TOL, (ckh[k], ckd[k])
    assert abs(ckh["max_ssim"] - ckd["max_ssim"]) <= TOL and abs(ckh["max_psnr"] - ckd["max_psnr"]) <= TOL
    assert lh == ld and len(lh) == 2
    pat = re.compile(r"^(My_NH_ffa_3_2_\d+_psnr: )([-0-9.e]+)(_ssim: )([-0-9.e]+)(\.pk)$")
    for a, b in zip(nh, nd):
        ma, mb = pat.match(a), pat.match(b)
        assert ma and mb and ma.group(1, 3, 5) == mb.group(1, 3, 5)
        assert abs(float(ma.group(2)) - float(mb.group(2))) <= TOL and abs(float(ma.group(4)) - float(mb.group(4))) <= TOL


def test_ffa_main_ffa_metrics(tmp_path):
    _, ck, lines = _ffa_main(tmp_path, "ffa")
    assert len(ck["ssims"]) == len(ck["psnrs"]) == 2 and len(lines) == 2
    assert all(math.isfinite(v) and 0 < v <= 1 for v in ck["ssims"]) and all(math.isfinite(v) and 0 < v <= 100 for v in ck["psnrs"])


def test_eval_any_resolution_gpu_metrics():
    """the four printed numbers: the first pair within 1e-6 of the default route's print (six decimals), the second pair within 2e-4 (the
    default route's utils.SSIM is the fp32 evaluation, at most 7.7e-5 from float64; PSNR2 within 1e-4 dB)"""
    code = "import torch; torch.manual_seed(6); import eval_any_resolution as E; E.main(%r)"
    args = ["--synthetic", "2", "--height", "96", "--width", "120"]
    outs = []
    for extra in ([], ["--gpu_metrics"]):
        r = subprocess.run([sys.executable, "-c", code % (args + extra)], cwd=PKG, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        m1 = re.search(r"PSNR: ([-0-9.]+), SSIM: ([-0-9.]+)", r.stdout)
        m2 = re.search(r"PSNR2: ([-0-9.]+), SSIM2: ([-0-9.]+)", r.stdout)
        assert m1 and m2, r.stdout[-2000:]
        outs.append([float(v) for v in m1.groups() + m2.groups()])
    print("default", outs[0], "gpu_metrics", outs[1])
    assert all(math.isfinite(v) for v in outs[1])
    assert round(abs(outs[0][0] - outs[1][0]), 9) <= 1e-6 and round(abs(outs[0][1] - outs[1][1]), 9) <= 1e-6
    assert abs(outs[0][2] - outs[1][2]) <= 1e-4 and abs(outs[0][3] - outs[1][3]) <= 2e-4
