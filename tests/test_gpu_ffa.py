"""FFA-Net on the kernels (csrc/ffa_attn.hip, dehaze_hip/ffa.py).

Kernels against float64: every dhz_ffa_* entry against a restatement of the formulas of include/dehaze_hip.h (K13) in float64 torch on the
CPU, for G = 1 (with and without the residual) and G = 3, at one chunk (1 x 16 x 16), non-square maps both ways with per-image gates
that differ (2 x 16 x 32, 3 x 32 x 16) and a map of several reduction chunks and workgroups that is no power of two (2 x 48 x 80: 3840
pixels = 4 pooling chunks, the last one short; 30 backward workgroups per image = two level-1 segments, the second one short).
Bounds are the project's: elementwise outputs atol 2e-5 (forward) / 5e-5 (backward), rtol 1e-4 (tests/test_gpu_winograd.py); summed
outputs 2e-5 sqrt(T) + 1e-4 with T the number of summed positions (tests/test_gpu_linear.py): T = H W for per-image sums (mean H W, dca),
T = B H W for the parameter gradients.  Every output map has 64 NaN floats behind it that must stay NaN; every input map ends with its
allocation.  Each reducing entry runs twice and once more under dhz_set_reserved_cus(100): the same bits.

The model: forward, gradient norms and sampled gradient entries against the reference fixture tests/golden/ffa_blocks2.npz, three
train_step calls against float64 AdamW, two deterministic runs bit-equal, the fallback for sides that are no multiples of 16, and
My_train.py --arch FFA.  Bounds: those of tests/test_gpu_unet.py."""
import glob
import math
import os
import random
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
GOLD = os.path.join(ROOT, "tests", "golden", "ffa_blocks2.npz")
SHAPES = [(1, 16, 16), (2, 16, 32), (3, 32, 16), (2, 48, 80)]
# (G, residual) x shape -> a seed at which every float64 ReLU pre-activation (hid, h) stays 1e-5 away from zero (found on the CPU; asserted)
GUARD = 1e-5


def to_blocked(x):
    """[B, 64, H, W] -> [B, 8, H, W, 8]"""
    B, C, H, W = x.shape
    return x.view(B, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_blocked(x):
    B, _, H, W, _ = x.shape
    return x.permute(0, 1, 4, 2, 3).reshape(B, 64, H, W)


def make_case(G, has_res, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    hc = 8 if G == 1 else 4
    n = 64 * G
    c = dict(G=G, B=B, H=H, W=W, hc=hc)
    c["maps"] = [torch.randn(B, 64, H, W, generator=g) for _ in range(G)]
    c["res"] = torch.randn(B, 64, H, W, generator=g) if has_res else None
    c["dout"] = torch.randn(B, 64, H, W, generator=g)
    c["Wa"] = torch.randn(hc, n, generator=g) * 2 / math.sqrt(n)
    c["ba"] = torch.randn(hc, generator=g) * 0.5
    c["Wb"] = torch.randn(n, hc, generator=g) * 2 / math.sqrt(hc)
    c["bb"] = torch.randn(n, generator=g) * 0.5
    c["Wp1"] = torch.randn(8, 64, generator=g) * 2 / math.sqrt(64)
    c["bp1"] = torch.randn(8, generator=g) * 0.5
    c["wp2"] = torch.randn(8, generator=g) * 2 / math.sqrt(8)
    c["bp2"] = torch.randn(1, generator=g) * 0.5
    return c


def reference(c):
    """the formulas of the header in float64; returns a dict of everything the entries write, and the smallest |ReLU pre-activation|"""
    d = {k: (v.double() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    G, B, H, W = c["G"], c["B"], c["H"], c["W"]
    HW = H * W
    m = [x.double() for x in c["maps"]]
    Wa, ba, Wb, bb, Wp1, bp1, wp2, bp2 = (d[k] for k in ("Wa", "ba", "Wb", "bb", "Wp1", "bp1", "wp2", "bp2"))
    r = {}
    r["sum"] = torch.cat([x.sum((2, 3)) for x in m], 1)                               # mean * HW, [B, 64 G]
    mean = r["sum"] / HW
    hid_pre = mean @ Wa.T + ba
    hid = hid_pre.clamp(min=0)
    ca = torch.sigmoid(hid @ Wb.T + bb)
    cag = ca.view(B, G, 64)
    t = sum(cag[:, g, :, None, None] * m[g] for g in range(G))
    h_pre = torch.einsum("ic,bchw->bihw", Wp1, t) + bp1[None, :, None, None]
    h = h_pre.clamp(min=0)
    pg = torch.sigmoid(torch.einsum("i,bihw->bhw", wp2, h) + bp2)
    out = t * pg[:, None]
    if c["res"] is not None:
        out = out + d["res"]
    r.update(mean=mean, hid=hid, ca=ca, out=out)
    dout = d["dout"]
    dpg = (dout * t).sum(1)
    dz = dpg * pg * (1 - pg)
    dh = dz[:, None] * wp2[None, :, None, None] * (h_pre > 0)
    dt = dout * pg[:, None] + torch.einsum("ic,bihw->bchw", Wp1, dh)
    r["dt"] = dt
    r["dwp2"] = (dz[:, None] * h).sum((0, 2, 3))
    r["dbp2"] = dz.sum().reshape(1)
    r["dWp1"] = torch.einsum("bihw,bchw->ic", dh, t)
    r["dbp1"] = dh.sum((0, 2, 3))
    dca = torch.cat([(dt * m[g]).sum((2, 3)) for g in range(G)], 1)
    r["dca"] = dca
    dzb = dca * ca * (1 - ca)
    r["dWb"] = dzb.T @ hid
    r["dbb"] = dzb.sum(0)
    dhid = (dzb @ Wb) * (hid_pre > 0)
    r["dWa"] = dhid.T @ mean
    r["dba"] = dhid.sum(0)
    dmean = dhid @ Wa
    r["dmean"] = dmean
    dmg = dmean.view(B, G, 64)
    r["dm"] = [cag[:, g, :, None, None] * dt + dmg[:, g, :, None, None] / HW for g in range(G)]
    return r, min(hid_pre.abs().min().item(), h_pre.abs().min().item())


def find_seed(G, has_res, B, H, W):
    """the first seed from 1 whose float64 pre-activations keep the guard (run on the CPU to fill SEEDS)"""
    for seed in range(1, 200):
        if reference(make_case(G, has_res, B, H, W, seed))[1] >= GUARD:
            return seed
    raise AssertionError("no seed found")


SEEDS = {
    (1, False): {(1, 16, 16): 1, (2, 16, 32): 1, (3, 32, 16): 1, (2, 48, 80): 1},
    (1, True): {(1, 16, 16): 1, (2, 16, 32): 1, (3, 32, 16): 1, (2, 48, 80): 4},
    (3, False): {(1, 16, 16): 1, (2, 16, 32): 1, (3, 32, 16): 1, (2, 48, 80): 1},
}


def exact(t):
    """an input on the device that ends with its allocation"""
    d = torch.empty(t.shape, device="cuda", dtype=torch.float32)
    d.copy_(t)
    return d


class Canary:
    """an output tensor with 64 NaN floats behind it"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 64,), float("nan"), device="cuda")
        self.t = self.buf[:n].view(*shape)

    def get(self):
        torch.cuda.synchronize()
        assert torch.isnan(self.buf[-64:]).all(), "written behind the output"
        assert not torch.isnan(self.t).any(), "output not fully written"
        return self.t.cpu().double()


def close(got, want, atol, rtol, what):
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    worst = (err - bound).max().item()
    print(f"{what}: max error {err.max().item():.3e} (atol {atol:.2e}, rtol {rtol:.0e}, scale {want.abs().max().item():.3e})")
    assert worst <= 0, (what, err.max().item(), atol)


def run_chain(c):
    """all five attention entries in order on the device; returns the canaried outputs by name"""
    from dehaze_hip import _lib
    lib = _lib.load()
    G, B, H, W, hc = c["G"], c["B"], c["H"], c["W"], c["hc"]
    n = 64 * G
    s = torch.cuda.current_stream().cuda_stream
    maps = [exact(to_blocked(x)) for x in c["maps"]]
    mp = [x.data_ptr() for x in maps] + [None] * (3 - G)
    P = {k: exact(c[k]) for k in ("Wa", "ba", "Wb", "bb", "Wp1", "bp1", "wp2", "bp2")}
    res = exact(to_blocked(c["res"])) if c["res"] is not None else None
    dout = exact(to_blocked(c["dout"]))
    need = lib.dhz_ffa_workspace_bytes(B, H, W, G)
    assert need > 0
    ws = Canary(need // 4)
    o = {k: Canary(*shape) for k, shape in dict(mean=(B, n), hid=(B, hc), ca=(B, n), out=(B, 8, H, W, 8), dt=(B, 8, H, W, 8), dWa=(hc, n),
                                                dba=(hc,), dWb=(n, hc), dbb=(n,), dmean=(B, n), dWp1=(8, 64), dbp1=(8,), dwp2=(8,),
                                                dbp2=(1,)).items()}
    dm = [Canary(B, 8, H, W, 8) for _ in range(G)]
    p = lambda k: o[k].t.data_ptr()  # noqa: E731
    _lib.call("dhz_ffa_ca_fwd", *mp, P["Wa"].data_ptr(), P["ba"].data_ptr(), P["Wb"].data_ptr(), P["bb"].data_ptr(), p("mean"), p("hid"),
              p("ca"), ws.t.data_ptr(), need, B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_fwd", *mp, p("ca"), P["Wp1"].data_ptr(), P["bp1"].data_ptr(), P["wp2"].data_ptr(), P["bp2"].data_ptr(),
              res.data_ptr() if res is not None else None, p("out"), B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_bwd_a", *mp, p("ca"), P["Wp1"].data_ptr(), P["bp1"].data_ptr(), P["wp2"].data_ptr(), P["bp2"].data_ptr(),
              dout.data_ptr(), p("dt"), ws.t.data_ptr(), need, B, H, W, G, s)
    _lib.call("dhz_ffa_ca_bwd", ws.t.data_ptr(), need, P["Wa"].data_ptr(), P["Wb"].data_ptr(), p("mean"), p("hid"), p("ca"), p("dWa"),
              p("dba"), p("dWb"), p("dbb"), p("dmean"), p("dWp1"), p("dbp1"), p("dwp2"), p("dbp2"), B, H, W, G, s)
    _lib.call("dhz_ffa_gate_pa_bwd_b", p("dt"), p("ca"), p("dmean"), *([x.t.data_ptr() for x in dm] + [None] * (3 - G)), B, H, W, G, s)
    torch.cuda.synchronize()
    assert torch.isnan(ws.buf[-64:]).all(), "written behind the workspace"
    got = {k: v.get() for k, v in o.items()}
    got["dm"] = [x.get() for x in dm]
    # dca is no output of its own: dhz_ffa_ca_bwd leaves its level-1 sums in the workspace (include/dehaze_hip.h, K13)
    chunks, slot = H * W // 128, n + 532
    nseg = (chunks + 15) // 16
    segs = ws.buf[B * chunks * slot: B * (chunks + nseg) * slot].view(B, nseg, slot)[:, :, :n].cpu().double()
    assert not torch.isnan(segs).any()
    got["dca"] = segs.sum(1)
    return got


CASES = [(G, has_res, shape) for (G, has_res) in ((1, True), (1, False), (3, False)) for shape in SHAPES]


@pytest.mark.parametrize("G,has_res,shape", CASES, ids=[f"G{G}-res{int(r)}-{'x'.join(map(str, s))}" for G, r, s in CASES])
def test_attention_entries_against_float64(G, has_res, shape):
    B, H, W = shape
    c = make_case(G, has_res, B, H, W, SEEDS[(G, has_res)][shape])
    r, guard = reference(c)
    assert guard >= GUARD, f"a ReLU pre-activation within {guard:.2e} of zero: choose another seed (find_seed)"
    got = run_chain(c)
    HW = H * W
    img, par = 2e-5 * math.sqrt(HW) + 1e-4, 2e-5 * math.sqrt(B * HW) + 1e-4
    close(got["mean"] * HW, r["sum"], img, 0, "mean * HW")
    close(got["hid"], r["hid"], 2e-5, 1e-4, "hid")
    close(got["ca"], r["ca"], 2e-5, 1e-4, "ca")
    close(from_blocked(got["out"]), r["out"], 2e-5, 1e-4, "out")
    close(from_blocked(got["dt"]), r["dt"], 5e-5, 1e-4, "dt")
    close(got["dca"], r["dca"], img, 0, "dca")
    for k in ("dWp1", "dbp1", "dwp2", "dbp2", "dWa", "dba", "dWb", "dbb"):
        close(got[k], r[k], par, 0, k)
    close(got["dmean"], r["dmean"], img, 0, "dmean")
    for g in range(G):
        close(from_blocked(got["dm"][g]), r["dm"][g], 5e-5, 1e-4, f"dm_{g}")
    # per-image gates differ: a kernel that reused image 0's gates would pass none of the above
    if B > 1:
        assert (r["ca"][0] - r["ca"][1]).abs().max() > 1e-2


@pytest.mark.parametrize("G,shape", [(1, (2, 48, 80)), (3, (2, 48, 80)), (1, (3, 32, 16))])
def test_attention_entries_are_bit_reproducible(G, shape):
    from dehaze_hip import _lib
    B, H, W = shape
    c = make_case(G, False, B, H, W, 5)
    a = run_chain(c)
    b = run_chain(c)
    try:
        _lib.call("dhz_set_reserved_cus", 100)
        d = run_chain(c)
    finally:
        _lib.call("dhz_set_reserved_cus", 0)
    for other in (b, d):
        for k, v in a.items():
            if k == "dm":
                assert all(torch.equal(x, y) for x, y in zip(v, other[k]))
            else:
                assert torch.equal(v, other[k]), k


@pytest.mark.parametrize("n", [8, 2 * 64 * 16 * 32, 3 * 64 * 32 * 16 + 4])
def test_elementwise_helpers_against_float64(n):
    from dehaze_hip import _lib
    g = torch.Generator().manual_seed(n)
    a1 = torch.randn(n, generator=g).clamp(min=0)                       # a post-ReLU activation: zeros and positives
    planted = torch.tensor([0.0, -0.0, 1e-40, 3e-8])                    # zero, minus zero, a positive denormal, a small positive
    a1[:4] = planted
    a1[-4:] = planted.flip(0)
    x = torch.randn(n, generator=g) * 1e3                               # large next to a small a1: (a1 + x) - x would lose the sign
    dr, dout = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s = torch.cuda.current_stream().cuda_stream
    res, dpre1, sm = Canary(n), Canary(n), Canary(n)
    da1, dx, ddr, ddout = exact(a1), exact(x), exact(dr), exact(dout)
    _lib.call("dhz_ffa_add", da1.data_ptr(), dx.data_ptr(), res.t.data_ptr(), n, s)
    _lib.call("dhz_ffa_relu_bwd_add", da1.data_ptr(), ddr.data_ptr(), ddout.data_ptr(), dpre1.t.data_ptr(), sm.t.data_ptr(), n, s)
    close(res.get(), a1.double() + x.double(), 2e-5, 1e-4, "res")
    close(dpre1.get(), torch.where(a1 > 0, dr, torch.zeros(())).double(), 5e-5, 1e-4, "dpre1")
    close(sm.get(), dout.double() + dr.double(), 5e-5, 1e-4, "s")
    assert torch.equal(dpre1.get()[:4], torch.where(planted > 0, dr[:4], torch.zeros(())).double())      # the mask is the sign of a1 itself


# ---- the module on the kernels
MODEL_SEED, POS_SEED, NPOS, GATE_SCALE = 41, 43, 32, 4.0


def seeded_ffa(seed=MODEL_SEED, scaled=True, blocks=2):
    from dehaze_hip.ffa import FFA
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    net = FFA(gps=3, blocks=blocks)
    if scaled:                                                          # as tests/golden/gen_golden_ffa.py::scale_gates
        with torch.no_grad():
            for n, p in net.named_parameters():
                if {"ca", "pa"} & set(n.split(".")):
                    p.mul_(GATE_SCALE)
    return net


def test_ffa_forward_and_gradients_against_the_reference_fixture():
    g = np.load(GOLD)
    net = seeded_ffa().cuda()
    x, gout = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["gout"]).cuda()
    assert tuple(x.shape) == (2, 3, 32, 48)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        y = net(x)
        (y * gout).sum().backward()
    assert not [w for w in rec if "library" in str(w.message)], [str(w.message) for w in rec]
    yr = torch.from_numpy(g["y"])
    print("FFA forward: max error", (y.detach().cpu() - yr).abs().max().item())
    assert torch.allclose(y.detach().cpu(), yr, atol=2e-4, rtol=1e-3), (y.detach().cpu() - yr).abs().max()
    named = list(net.named_parameters())
    gn = np.array([float(p.grad.double().norm()) for _, p in named])
    rel = np.abs(gn - g["grad_norm"]) / (g["grad_norm"] + 1e-8)
    print("FFA gradient norms: worst relative error", rel.max(), named[int(rel.argmax())][0])
    assert rel.max() < 5e-3, (rel.max(), named[int(rel.argmax())][0])
    pg = torch.Generator().manual_seed(POS_SEED)
    worst = 0.0
    for i, (n, p) in enumerate(named):
        pos = torch.randint(p.numel(), (NPOS,), generator=pg)
        got = p.grad.reshape(-1).cpu()[pos].double().numpy()
        ref = g["grad_samples"][i]
        worst = max(worst, np.abs(got - ref).max() / (np.abs(ref).max() + 1e-8))
    print("FFA sampled gradient entries: worst error relative to the parameter's largest sample", worst)
    assert worst < 5e-3, worst


def _three_steps(deterministic=False):
    from dehaze_hip import ops
    from dehaze_hip.train import FlatAdamW, train_step
    from losses import CharbonnierLoss
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(2, 3, 32, 32, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(2, 1, 1, 1, generator=g)).clamp(0, 1)
    try:
        if deterministic:
            ops.set_deterministic(True)
        net = seeded_ffa(seed=1234, scaled=False).cuda()
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


def test_ffa_three_train_steps_against_float64_adamw():
    losses, sd, (hazy, gt) = _three_steps()
    ref = seeded_ffa(seed=1234, scaled=False).double()
    opt = torch.optim.AdamW(ref.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.02)
    for step in range(3):
        opt.zero_grad()
        d = ref._forward_torch(hazy.double()).clamp(0, 1) - gt.double()
        loss = torch.sqrt(d * d + 1e-3 ** 2).mean()                    # CharbonnierLoss, eps 1e-3 (losses.py)
        loss.backward()
        opt.step()
        print("FFA step", step, losses[step], loss.item())
        assert abs(losses[step] - loss.item()) < 5e-5, (step, losses[step], loss.item())
    worst = max((sd[k].double() - v.detach()).abs().max().item() for k, v in ref.state_dict().items())
    print("FFA parameters after three steps: worst error", worst)
    assert worst < 5e-4, worst


def test_ffa_deterministic_steps_are_bit_equal():
    la, sa, _ = _three_steps(deterministic=True)
    lb, sb, _ = _three_steps(deterministic=True)
    assert la == lb
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


def test_ffa_other_sizes_fall_back_with_one_warning_and_equal_torch():
    from dehaze_hip import ops
    net = seeded_ffa(seed=5).cuda()
    x = torch.rand(2, 3, 24, 40, generator=torch.Generator().manual_seed(3)).cuda()
    ops._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            y = net(x)
            y2 = net(x)
    msgs = [str(w.message) for w in rec if "library" in str(w.message)]
    assert len(msgs) == 1 and "FFA" in msgs[0], msgs
    with torch.no_grad():
        yt = net._forward_torch(x)
    assert torch.allclose(y, yt, atol=2e-4, rtol=1e-3) and torch.allclose(y2, yt, atol=2e-4, rtol=1e-3)
    gout = torch.randn(2, 3, 24, 40, generator=torch.Generator().manual_seed(4)).cuda()
    grads = []
    for fwd in (net, net._forward_torch):
        net.zero_grad(set_to_none=True)
        (fwd(x) * gout).sum().backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    for (n, _), ga, gb in zip(net.named_parameters(), *grads):
        scale = gb.abs().max().item()
        assert (ga - gb).abs().max().item() < 5e-3 * scale + 1e-6, (n, (ga - gb).abs().max().item(), scale)


def test_my_train_command_line_ffa():
    r = subprocess.run([sys.executable, "My_train.py", "--arch", "FFA", "--ffa_blocks", "2", "--train_ps", "64", "--batch_size", "2",
                        "--synthetic", "4", "--nepoch", "1", "--w_loss_vgg7", "0", "--env", "_ffa_cli_test"], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # every loss the run printed: the progress lines (loss:, Charbonnier:) and the epoch line (Loss:)
    vals = [float(v) for v in re.findall(r"(?:loss|Loss|Charbonnier):\s*([-+]?(?:nan|inf|[0-9.]+(?:e[-+]?[0-9]+)?))", r.stdout)]
    assert len(vals) >= 3, r.stdout[-2000:]
    assert all(math.isfinite(v) and v > 0 for v in vals), vals
    # whole-image evaluation of that 2-block checkpoint: test_long_GPU.py has no --ffa_blocks, the depth comes from DHZ_FFA_BLOCKS
    ckpts = sorted(glob.glob(os.path.join(PKG, "log", "FFA_ffa_cli_test", "models", "epoch_model_*.pth")), key=os.path.getmtime)
    assert ckpts, "My_train.py wrote no epoch checkpoint"
    env = dict(os.environ, DHZ_FFA_BLOCKS="2")
    e = subprocess.run([sys.executable, "test_long_GPU.py", "--arch", "FFA", "--weights", ckpts[-1], "--synthetic", "2", "--height", "96",
                        "--width", "120", "--train_ps", "64", "--save_images", "False"], cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=300)
    assert e.returncode == 0, e.stdout[-2000:] + e.stderr[-2000:]
    m = re.search(r"PSNR: ([-0-9.naif]+), SSIM: ([-0-9.naif]+)", e.stdout)
    assert m and math.isfinite(float(m.group(1))) and math.isfinite(float(m.group(2))), e.stdout[-2000:]
