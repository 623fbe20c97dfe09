"""FFA-Net on maps of any size: the `_any` attention entries (csrc/ffa_attn.hip), the model's ragged dispatch (dehaze_hip/ffa.py) and
FFA_test.py.

Kernels against float64: the restatement of the K13 formulas in tests/test_gpu_ffa.py, its bounds unchanged (elementwise 2e-5 forward /
5e-5 backward, rtol 1e-4; sums 2e-5 sqrt(T) + 1e-4), G = 1 with and without `res` and G = 3, at
  1 x 5 x 7     35 pixels: every workgroup is a tail
  2 x 17 x 19   323 pixels: a pooling chunk that is no multiple of 256; 3 backward workgroups, the last with 67 pixels
  3 x 33 x 16   528 pixels, three images
  2 x 42 x 52   2184 pixels: 3 pooling chunks; 18 backward workgroups = two level-1 segments, the second of 2 slots; the last workgroup
                holds 8 pixels
Every output has 64 NaN floats behind it that must stay NaN; every input map has 64 NaN floats behind it in its allocation that must
never reach a result.  The level-1 dca sums are read from the workspace offset the header documents, with chunks = ceil(H W / 128).

The model at 2 x 3 x 38 x 52 against the reference fixture tests/golden/ffa_any.npz (gen_golden_ffa_any.py) with the bounds of
test_ffa_forward_and_gradients_against_the_reference_fixture and no library warning; which entries a forward + backward names; the
DHZ_FFA_ANY switch; three train_step calls against float64 AdamW; FFA_test.py in a child process."""
import math
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import test_gpu_ffa as F

pytestmark = pytest.mark.gpu

ROOT = F.ROOT
PKG = F.PKG
GOLD = os.path.join(ROOT, "tests", "golden", "ffa_any.npz")
SHAPES = [(1, 5, 7), (2, 17, 19), (3, 33, 16), (2, 42, 52)]
REGULAR = (2, 16, 32)
# (G, residual) x shape -> a seed at which every float64 ReLU pre-activation (hid, h) stays GUARD away from zero (F.find_seed on the CPU; asserted)
SEEDS = {
    (1, True): {(1, 5, 7): 1, (2, 17, 19): 1, (3, 33, 16): 1, (2, 42, 52): 1, REGULAR: 1},
    (1, False): {(1, 5, 7): 1, (2, 17, 19): 1, (3, 33, 16): 1, (2, 42, 52): 3, REGULAR: 1},
    (3, False): {(1, 5, 7): 1, (2, 17, 19): 1, (3, 33, 16): 1, (2, 42, 52): 1, REGULAR: 1},
}
# shape -> (backward-a workgroups per image, level-1 segments per image) as the docstring counts them; held against the workspace query
TAILS = {(1, 5, 7): (1, 1), (2, 17, 19): (3, 1), (3, 33, 16): (5, 1), (2, 42, 52): (18, 2)}
ANY_LAUNCHES = ("dhz_ffa_ca_fwd_any", "dhz_ffa_gate_pa_fwd_any", "dhz_ffa_gate_pa_bwd_a_any", "dhz_ffa_ca_bwd_any", "dhz_ffa_gate_pa_bwd_b_any")


def tailed(t):
    """an input on the device with 64 NaN floats behind it in the same allocation"""
    buf = torch.full((t.numel() + 64,), float("nan"), device="cuda")
    buf[:t.numel()] = t.reshape(-1).cuda()
    return buf[:t.numel()].view(t.shape)


def run_chain(c, sfx="_any"):
    """the five attention entries (with `sfx`) in order on the device; returns the canaried outputs by name"""
    from dehaze_hip import _lib
    lib = _lib.load()
    G, B, H, W, hc = c["G"], c["B"], c["H"], c["W"], c["hc"]
    n = 64 * G
    s = torch.cuda.current_stream().cuda_stream
    maps = [tailed(F.to_blocked(x)) for x in c["maps"]]
    mp = [x.data_ptr() for x in maps] + [None] * (3 - G)
    P = {k: F.exact(c[k]) for k in ("Wa", "ba", "Wb", "bb", "Wp1", "bp1", "wp2", "bp2")}
    res = tailed(F.to_blocked(c["res"])) if c["res"] is not None else None
    dout = tailed(F.to_blocked(c["dout"]))
    need = lib.dhz_ffa_workspace_bytes_any(B, H, W, G) if sfx else lib.dhz_ffa_workspace_bytes(B, H, W, G)
    assert need > 0
    ws = F.Canary(need // 4)
    o = {k: F.Canary(*shape) for k, shape in dict(mean=(B, n), hid=(B, hc), ca=(B, n), out=(B, 8, H, W, 8), dt=(B, 8, H, W, 8), dWa=(hc, n),
                                                  dba=(hc,), dWb=(n, hc), dbb=(n,), dmean=(B, n), dWp1=(8, 64), dbp1=(8,), dwp2=(8,),
                                                  dbp2=(1,)).items()}
    dm = [F.Canary(B, 8, H, W, 8) for _ in range(G)]
    p = lambda k: o[k].t.data_ptr()  # noqa: E731
    _lib.call("dhz_ffa_ca_fwd" + sfx, *mp, P["Wa"].data_ptr(), P["ba"].data_ptr(), P["Wb"].data_ptr(), P["bb"].data_ptr(), p("mean"),
              p("hid"), p("ca"), ws.t.data_ptr(), need, B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_fwd" + sfx, *mp, p("ca"), P["Wp1"].data_ptr(), P["bp1"].data_ptr(), P["wp2"].data_ptr(), P["bp2"].data_ptr(),
              res.data_ptr() if res is not None else None, p("out"), B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_bwd_a" + sfx, *mp, p("ca"), P["Wp1"].data_ptr(), P["bp1"].data_ptr(), P["wp2"].data_ptr(), P["bp2"].data_ptr(),
              dout.data_ptr(), p("dt"), ws.t.data_ptr(), need, B, H, W, G, s)
    _lib.call("dhz_ffa_ca_bwd" + sfx, ws.t.data_ptr(), need, P["Wa"].data_ptr(), P["Wb"].data_ptr(), p("mean"), p("hid"), p("ca"), p("dWa"),
              p("dba"), p("dWb"), p("dbb"), p("dmean"), p("dWp1"), p("dbp1"), p("dwp2"), p("dbp2"), B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_bwd_b" + sfx, p("dt"), p("ca"), p("dmean"), *([x.t.data_ptr() for x in dm] + [None] * (3 - G)), B, H, W, G, s)
    torch.cuda.synchronize()
    assert torch.isnan(ws.buf[-64:]).all(), "written behind the workspace"
    got = {k: v.get() for k, v in o.items()}              # get(): the 64 floats behind stay NaN, and no NaN inside
    got["dm"] = [x.get() for x in dm]
    # the level-1 sums behind the partials (include/dehaze_hip.h, K13): float offset B chunks (64 G + 532), chunks = ceil(H W / 128)
    chunks, slot = (H * W + 127) // 128, n + 532
    nseg = (chunks + 15) // 16
    segs = ws.buf[B * chunks * slot: B * (chunks + nseg) * slot].view(B, nseg, slot)[:, :, :n].cpu().double()
    assert not torch.isnan(segs).any()
    got["dca"] = segs.sum(1)
    return got


def same_bits(a, b):
    for k, v in a.items():
        if k == "dm":
            assert all(torch.equal(x, y) for x, y in zip(v, b[k])), k
        else:
            assert torch.equal(v, b[k]), k


CASES = [(G, has_res, shape) for (G, has_res) in ((1, True), (1, False), (3, False)) for shape in SHAPES]


@pytest.mark.parametrize("G,has_res,shape", CASES, ids=[f"G{G}-res{int(r)}-{'x'.join(map(str, s))}" for G, r, s in CASES])
def test_any_attention_entries_against_float64(G, has_res, shape):
    from dehaze_hip import _lib
    B, H, W = shape
    c = F.make_case(G, has_res, B, H, W, SEEDS[(G, has_res)][shape])
    r, guard = F.reference(c)
    assert guard >= F.GUARD, f"a ReLU pre-activation within {guard:.2e} of zero: choose another seed (find_seed)"
    chunks, nseg = TAILS[shape]                             # the library cuts the map into the workgroups and segments counted above
    assert _lib.load().dhz_ffa_workspace_bytes_any(B, H, W, G) == 4 * B * ((chunks + nseg) * (64 * G + 532) + 2 * 64 * G * c["hc"] + 64 * G
                                                                            + c["hc"] + 532)
    got = run_chain(c)
    HW = H * W
    img, par = 2e-5 * math.sqrt(HW) + 1e-4, 2e-5 * math.sqrt(B * HW) + 1e-4
    F.close(got["mean"] * HW, r["sum"], img, 0, "mean * HW")
    F.close(got["hid"], r["hid"], 2e-5, 1e-4, "hid")
    F.close(got["ca"], r["ca"], 2e-5, 1e-4, "ca")
    F.close(F.from_blocked(got["out"]), r["out"], 2e-5, 1e-4, "out")
    F.close(F.from_blocked(got["dt"]), r["dt"], 5e-5, 1e-4, "dt")
    F.close(got["dca"], r["dca"], img, 0, "dca")
    for k in ("dWp1", "dbp1", "dwp2", "dbp2", "dWa", "dba", "dWb", "dbb"):
        F.close(got[k], r[k], par, 0, k)
    F.close(got["dmean"], r["dmean"], img, 0, "dmean")
    for g in range(G):
        F.close(F.from_blocked(got["dm"][g]), r["dm"][g], 5e-5, 1e-4, f"dm_{g}")
    if B > 1:
        assert (r["ca"][0] - r["ca"][1]).abs().max() > 1e-2
    # the same bits on a second run and with 100 CUs reserved
    same_bits(got, run_chain(c))
    try:
        _lib.call("dhz_set_reserved_cus", 100)
        d = run_chain(c)
    finally:
        _lib.call("dhz_set_reserved_cus", 0)
    same_bits(got, d)


@pytest.mark.parametrize("G,has_res", [(1, True), (1, False), (3, False)])
def test_any_entries_equal_the_old_entries_on_a_regular_shape(G, has_res):
    from dehaze_hip import _lib
    lib = _lib.load()
    B, H, W = REGULAR
    assert lib.dhz_ffa_workspace_bytes_any(B, H, W, G) == lib.dhz_ffa_workspace_bytes(B, H, W, G) > 0
    c = F.make_case(G, has_res, B, H, W, SEEDS[(G, has_res)][REGULAR])
    same_bits(run_chain(c, ""), run_chain(c, "_any"))


@pytest.mark.parametrize("n", [1, 3, 8, 1027, 3 * 413 * 550])
def test_add_any_against_float64(n):
    """dhz_ffa_add_any: any n (3 x 413 x 550 = 681450 is the image of the issue's second eval shape: n % 4 == 2); NaN behind inputs and output"""
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(n)
    a, x = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e3
    s = torch.cuda.current_stream().cuda_stream
    y = F.Canary(n)
    da, dx = tailed(a), tailed(x)
    _lib.call("dhz_ffa_add_any", da.data_ptr(), dx.data_ptr(), y.t.data_ptr(), n, s)
    got = y.get()
    F.close(got, a.double() + x.double(), 2e-5, 1e-4, "y")
    assert torch.equal(got.float(), a + x)                              # one rounding per element, as aten::add
    if n % 4 == 0:
        y2 = F.Canary(n)
        _lib.call("dhz_ffa_add", da.data_ptr(), dx.data_ptr(), y2.t.data_ptr(), n, s)
        assert torch.equal(y2.get(), got)


def test_ffa_on_an_image_whose_float_count_is_no_multiple_of_four(monkeypatch):
    """1 x 3 x 33 x 35 = 3465 floats: the `+ x1` of FFA:110 runs dhz_ffa_add_any; results against the library route of the same module"""
    net = F.seeded_ffa(seed=5).cuda()
    x = torch.rand(1, 3, 33, 35, generator=torch.Generator().manual_seed(3)).cuda()
    gout = torch.randn(1, 3, 33, 35, generator=torch.Generator().manual_seed(4)).cuda()
    names = _spy(monkeypatch)
    msgs, (y, y2, yt), grads = _library_route(net, x, gout)
    assert not msgs, msgs
    assert "dhz_ffa_add_any" in names and "dhz_ffa_gate_pa_fwd_any" in names
    assert torch.allclose(y, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y2, yt, atol=2e-4, rtol=1e-3)
    for (n, _), ga, gb in zip(net.named_parameters(), *grads):
        scale = gb.abs().max().item()
        assert (ga - gb).abs().max().item() < 5e-3 * scale + 1e-6, (n, (ga - gb).abs().max().item(), scale)


def test_ffa_on_a_batch_slice_that_is_not_16_byte_aligned():
    """image 1 of a 2 x 3 x 33 x 35 batch starts 13860 bytes into the allocation (FFA_main.evaluate walks a stacked batch this way)"""
    net = F.seeded_ffa(seed=5).cuda()
    x = torch.rand(2, 3, 33, 35, generator=torch.Generator().manual_seed(3)).cuda()
    assert x[1:2].data_ptr() % 16 != 0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y1, y = net(x[1:2]), net(x)
            yt = net._forward_torch(x[1:2])
    assert not [w for w in rec if "library" in str(w.message)], [str(w.message) for w in rec]
    assert torch.allclose(y1, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y1, y[1:2], atol=2e-4, rtol=1e-3)
    xs = x[1:2].detach().requires_grad_()                   # a misaligned leaf through the backward too
    net(xs).square().sum().backward()
    assert torch.isfinite(xs.grad).all()


def _write_png(path, chw):
    from PIL import Image
    Image.fromarray((chw.permute(1, 2, 0).numpy() * 255).round().astype(np.uint8), "RGB").save(path)


def test_ffa_test_command_line_on_folders(tmp_path):
    """--test_imgs / --gt_dir on real files: PNG and JPEG hazy images of two ragged sizes, PNG clear images named the SOTS way (1400_1 -> 1400)"""
    from PIL import Image
    from dehaze_hip.train import synthetic_batch
    net = F.seeded_ffa(seed=11, scaled=False)
    pk = str(tmp_path / "w.pk")
    torch.save({'model': {'module.' + k: v for k, v in net.state_dict().items()}}, pk)
    hazy_dir, gt_dir, out = tmp_path / "hazy", tmp_path / "gt", tmp_path / "pred"
    hazy_dir.mkdir()
    gt_dir.mkdir()
    for name, gname, (H, W) in (("1400_1.png", "1400.png", (46, 62)), ("1401_3.jpg", "1401.png", (33, 35))):
        gt, hazy = synthetic_batch(1, (H, W), seed=H, device="cpu")
        _write_png(str(gt_dir / gname), gt[0])
        if name.endswith(".png"):
            _write_png(str(hazy_dir / name), hazy[0])
        else:
            Image.fromarray((hazy[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8), "RGB").save(str(hazy_dir / name), quality=95)
    (hazy_dir / "notes.txt").write_text("not an image")
    r = subprocess.run([sys.executable, "FFA_test.py", "--test_imgs", str(hazy_dir), "--gt_dir", str(gt_dir), "--blocks", "2", "--weights", pk,
                        "--out_dir", str(out)], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "library" not in r.stderr, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["1400_1_FFA.png", "1401_3_FFA.png"]
    for f, size in (("1400_1_FFA.png", (62, 46)), ("1401_3_FFA.png", (35, 33))):
        with Image.open(out / f) as im:
            assert im.size == size and im.mode == "RGB"
    m = re.search(r"PSNR: ([-0-9.naif]+), SSIM: ([-0-9.naif]+) over 2 image", r.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))), r.stdout[-2000:]
    # a hazy file without a clear image is an error that names it
    _write_png(str(hazy_dir / "1500_1.png"), torch.rand(3, 33, 35))
    r = subprocess.run([sys.executable, "FFA_test.py", "--test_imgs", str(hazy_dir), "--gt_dir", str(gt_dir), "--blocks", "2", "--weights", pk,
                        "--out_dir", str(out)], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "1500_1.png" in r.stderr, r.stderr[-2000:]


# ---- the module on a ragged map
def test_ffa_ragged_forward_and_gradients_against_the_reference_fixture():
    g = np.load(GOLD)
    assert tuple(g["x"].shape) == (2, 3, 38, 52)
    gout = torch.from_numpy(g["gout"]).cuda()
    yr = torch.from_numpy(g["y"])
    for into_image in (False, True):
        net = F.seeded_ffa().cuda()
        x = torch.from_numpy(g["x"]).cuda()
        if into_image:
            x.requires_grad_()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            y = net(x)
            (y * gout).sum().backward()
        assert not [w for w in rec if "library" in str(w.message)], [str(w.message) for w in rec]
        print("FFA 38 x 52 forward: max error", (y.detach().cpu() - yr).abs().max().item())
        assert torch.allclose(y.detach().cpu(), yr, atol=2e-4, rtol=1e-3), (y.detach().cpu() - yr).abs().max()
        named = list(net.named_parameters())
        assert [n for n, _ in named] == list(g["names"])
        gn = np.array([float(p.grad.double().norm()) for _, p in named])
        rel = np.abs(gn - g["grad_norm"]) / (g["grad_norm"] + 1e-8)
        print("FFA 38 x 52 gradient norms: worst relative error", rel.max(), named[int(rel.argmax())][0])
        assert rel.max() < 5e-3, (rel.max(), named[int(rel.argmax())][0])
        pg = torch.Generator().manual_seed(F.POS_SEED)
        worst = 0.0
        for i, (n, p) in enumerate(named):
            pos = torch.randint(p.numel(), (F.NPOS,), generator=pg)
            got = p.grad.reshape(-1).cpu()[pos].double().numpy()
            ref = g["grad_samples"][i]
            worst = max(worst, np.abs(got - ref).max() / (np.abs(ref).max() + 1e-8))
        print("FFA 38 x 52 sampled gradient entries: worst error relative to the parameter's largest sample", worst)
        assert worst < 5e-3, worst
        if into_image:
            dx, dxr = x.grad.cpu().double().numpy(), g["dx"].astype(np.float64)
            assert abs(np.linalg.norm(dx) - np.linalg.norm(dxr)) / np.linalg.norm(dxr) < 5e-3
            e = np.abs(dx - dxr).max() / np.abs(dxr).max()
            print("FFA 38 x 52 image gradient: worst error relative to its largest entry", e)
            assert e < 5e-3, e


def _spy(monkeypatch):
    from dehaze_hip import _lib
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return names


def _fwd_bwd(net, H, W):
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H * W)).cuda()
    net.zero_grad(set_to_none=True)
    net(x).square().sum().backward()
    torch.cuda.synchronize()


def test_dispatch_names_any_entries_on_ragged_maps_only(monkeypatch):
    net = F.seeded_ffa(seed=5).cuda()
    names = _spy(monkeypatch)
    _fwd_bwd(net, 32, 48)
    assert names and not [n for n in names if n.endswith("_any")], sorted(set(names))
    assert {"dhz_winograd_conv3x3", "dhz_conv3x3_wgrad", "dhz_ffa_ca_fwd", "dhz_ffa_gate_pa_bwd_a"} <= set(names)
    del names[:]
    _fwd_bwd(net, 38, 52)
    assert {"dhz_winograd_conv3x3_any", "dhz_conv3x3_wgrad_any", *ANY_LAUNCHES} <= set(names), sorted(set(names))
    assert not {"dhz_winograd_conv3x3", "dhz_winograd43_conv3x3", "dhz_conv3x3_wgrad", "dhz_ffa_ca_fwd", "dhz_ffa_gate_pa_fwd",
                "dhz_ffa_gate_pa_bwd_a", "dhz_ffa_ca_bwd", "dhz_ffa_gate_pa_bwd_b"} & set(names), sorted(set(names))


def _library_route(net, x, gout):
    """forward twice + gradients through net(x); the library warnings raised; the same through _forward_torch"""
    from dehaze_hip import ops
    ops._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y, y2 = net(x), net(x)
    msgs = [str(w.message) for w in rec if "library" in str(w.message)]
    with torch.no_grad():
        yt = net._forward_torch(x)
    grads = []
    for fwd in (net, net._forward_torch):
        net.zero_grad(set_to_none=True)
        (fwd(x) * gout).sum().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    return msgs, (y, y2, yt), grads


def test_switch_off_restores_the_library_route(monkeypatch):
    from dehaze_hip import ffa
    net = F.seeded_ffa(seed=5).cuda()
    x = torch.rand(2, 3, 38, 52, generator=torch.Generator().manual_seed(3)).cuda()
    gout = torch.randn(2, 3, 38, 52, generator=torch.Generator().manual_seed(4)).cuda()
    monkeypatch.setattr(ffa, "ANY", False)
    names = _spy(monkeypatch)
    msgs, (y, y2, yt), grads = _library_route(net, x, gout)
    assert len(msgs) == 1 and "FFA" in msgs[0], msgs
    assert not [n for n in names if n.startswith("dhz_ffa") or n.startswith("dhz_winograd")], sorted(set(names))
    assert torch.allclose(y, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y2, yt, atol=2e-4, rtol=1e-3)
    for (n, _), ga, gb in zip(net.named_parameters(), *grads):
        scale = gb.abs().max().item()
        assert (ga - gb).abs().max().item() < 5e-3 * scale + 1e-6, (n, (ga - gb).abs().max().item(), scale)
    # and with the switch on the kernels agree with that route at the same bounds
    monkeypatch.setattr(ffa, "ANY", True)
    msgs, (y, y2, yt), grads = _library_route(net, x, gout)
    assert not msgs, msgs
    assert torch.allclose(y, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y2, yt, atol=2e-4, rtol=1e-3)
    for (n, _), ga, gb in zip(net.named_parameters(), *grads):
        scale = gb.abs().max().item()
        assert (ga - gb).abs().max().item() < 5e-3 * scale + 1e-6, (n, (ga - gb).abs().max().item(), scale)


def test_a_ragged_map_below_the_floor_still_falls_back(monkeypatch):
    from dehaze_hip import ffa, ops
    assert ffa.ANY and not ffa.blocked_shape_ok(24, 40)
    net = F.seeded_ffa(seed=5).cuda()
    x = torch.rand(1, 3, 24, 40, generator=torch.Generator().manual_seed(3)).cuda()
    names = _spy(monkeypatch)
    ops._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            net(x)
    assert len([w for w in rec if "library" in str(w.message)]) == 1
    assert not [n for n in names if n.endswith("_any")], sorted(set(names))


SHAPE = (2, 3, 38, 52)


def _three_steps(deterministic=False):
    from dehaze_hip import ops
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(*SHAPE, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    try:
        if deterministic:
            ops.set_deterministic(True)
        net = F.seeded_ffa(seed=1234, scaled=False).cuda()
        opt = FlatAdamW(net, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
        crit = CharbonnierLoss()
        net.train()
        losses = []
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for _ in range(3):
                loss, _, _ = train_step(net, crit, None, opt, None, hazy.cuda(), gt.cuda(), w_cr=0.0)
                losses.append(loss.item())
        assert not [w for w in rec if "library" in str(w.message)], [str(w.message) for w in rec]
        return losses, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, (hazy, gt)
    finally:
        if deterministic:
            ops.set_deterministic(False)


def test_ffa_ragged_three_train_steps_against_float64_adamw():
    losses, sd, (hazy, gt) = _three_steps()
    ref = F.seeded_ffa(seed=1234, scaled=False).double()
    opt = torch.optim.AdamW(ref.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    for step in range(3):
        opt.zero_grad()
        d = ref._forward_torch(hazy.double()).clamp(0, 1) - gt.double()
        loss = torch.sqrt(d * d + 1e-3 ** 2).mean()                    # CharbonnierLoss, eps 1e-3 (losses.py)
        loss.backward()
        opt.step()
        print("FFA 38 x 52 step", step, losses[step], loss.item())
        assert abs(losses[step] - loss.item()) < 5e-5, (step, losses[step], loss.item())
    worst = max((sd[k].double() - v.detach()).abs().max().item() for k, v in ref.state_dict().items())
    print("FFA 38 x 52 parameters after three steps: worst error", worst)
    assert worst < 5e-4, worst


def test_ffa_ragged_deterministic_steps_are_bit_equal():
    la, sa, _ = _three_steps(deterministic=True)
    lb, sb, _ = _three_steps(deterministic=True)
    assert la == lb
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_ffa_test_command_line(tmp_path):
    from PIL import Image
    net = F.seeded_ffa(seed=11, scaled=False)
    pk = str(tmp_path / "its_train_ffa_3_2.pk")
    torch.save({'step': 1, 'max_psnr': 0.0, 'max_ssim': 0.0, 'ssims': [], 'psnrs': [], 'losses': [],
                'model': {'module.' + k: v for k, v in net.state_dict().items()}}, pk)
    out = tmp_path / "pred"
    r = subprocess.run([sys.executable, "FFA_test.py", "--synthetic", "2", "--height", "46", "--width", "62", "--blocks", "2", "--weights", pk,
                        "--out_dir", str(out)], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "library" not in r.stderr, r.stderr[-2000:]
    pngs = sorted(os.listdir(out))
    assert pngs == ["synthetic_000_FFA.png", "synthetic_001_FFA.png"], pngs
    for f in pngs:
        with Image.open(out / f) as im:
            assert im.size == (62, 46) and im.mode == "RGB"
    m = re.search(r"PSNR: ([-0-9.naif]+), SSIM: ([-0-9.naif]+)", r.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))), r.stdout[-2000:]
