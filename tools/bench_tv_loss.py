#!/usr/bin/env python3
"""The total-variation losses (dhz_tv_loss_fwd / _bwd, dehaze_hip/tv_loss.py): the kernels against the ATen formula they replace
(tv_loss.KERNELS = False, what DHZ_TV_LOSS=0 sets), in one process, the two routes alternated.

  1. the loss alone: TVTerm(form)(x) + backward for both forms at 32 x 3 x 128 x 128, 4 x 3 x 240 x 240 and 1 x 3 x 460 x 620, ms per call
     by device events over --iters calls after a warm-up, --rounds rounds; and the C entries alone (forward: two launches; backward: one)
  2. the steps: ffa_train_step (FFA(3, --blocks), L1, 4 x 3 x 240 x 240) and train_step (Uformer E = 32, Charbonnier, w_cr = 0,
     32 x 3 x 128 x 128) with the term off, on the kernels and on the ATen formula: ms per step, wall time over --steps steps that end in a
     device synchronise
  3. the achieved errors of both routes against the float64 reference on the cases of tests/golden/tv_loss.npz
  4. with --parent DIR (a built checkout of the parent commit): `bench.py --gpus 1 --steps 30 --warmup 10` there and here, alternated, each
     in a fresh child process; the result lines as printed
No threshold: the numbers are the result.  Writes profiles/tv_loss.txt.

usage:  python tools/bench_tv_loss.py [--blocks 19] [--iters 50] [--steps 10] [--rounds 5] [--parent DIR] [--passes 2] [--out profiles/tv_loss.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
for p in (PKG, ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(32, 3, 128, 128), (4, 3, 240, 240), (1, 3, 460, 620)]
NAMES = ("one_site", "row", "col", "odd", "two_bands", "clamped", "flat")
FORM = {"beta": 0, "sq": 1}
COEFF = {"beta": 5.0, "sq": 1.0}
ATEN = "ATen formula (DHZ_TV_LOSS=0)"


def events(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def row(name, ts, fmt="9.3f"):
    s = sorted(ts)
    return f"    {name:44s} " + "  ".join(format(t, fmt) for t in ts) + f"   median {s[len(s) // 2]:.3f}  min {s[0]:.3f}  max {s[-1]:.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=19)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: part 4")
    ap.add_argument("--passes", type=int, default=2, help="part 4: bench.py runs per arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tv_loss.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tv_loss.py measures on the GPU"
    import My_model_1 as M1
    from dehaze_hip import _lib, ffa, tv_loss as TV
    from dehaze_hip.train import FlatAdamW, ffa_train_step, synthetic_batch, train_step
    from losses import CharbonnierLoss
    lib = _lib.load()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    def route(kernels, fn):
        def run():
            TV.KERNELS = kernels
            try:
                return fn()
            finally:
                TV.KERNELS = True
        return run

    say(f"tools/bench_tv_loss.py on {torch.cuda.get_device_name(0)}, library {lib.dhz_build_id().decode()}")
    say(f"1. the loss alone, forward + backward, ms per call (device events over {a.iters} calls after 5 warm-up calls; {a.rounds} rounds, the "
        "rows of a shape alternated)")
    for shape in SHAPES:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(H)
        x = torch.rand(shape, generator=g).to(dev).requires_grad_(True)
        need = lib.dhz_tv_loss_workspace_bytes(B, C, H, W)
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        loss, gl, dx = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty(shape, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        xd = x.detach()
        for form in ("beta", "sq"):
            term = TV.TVTerm(form)

            def both():
                x.grad = None
                term(x).backward()

            def c_fwd():
                _lib.call("dhz_tv_loss_fwd", loss.data_ptr(), xd.data_ptr(), B, C, H, W, FORM[form], 0.5, COEFF[form], ws.data_ptr(), need, st)

            def c_bwd():
                _lib.call("dhz_tv_loss_bwd", dx.data_ptr(), gl.data_ptr(), xd.data_ptr(), B, C, H, W, FORM[form], 0.5, COEFF[form], st)

            rows = [("TVTerm, kernels", route(True, both)), ("TVTerm, " + ATEN, route(False, both)),
                    ("dhz_tv_loss_fwd alone", c_fwd), ("dhz_tv_loss_bwd alone", c_bwd)]
            times = {n: [] for n, _ in rows}
            for _ in range(a.rounds):
                for n, fn in rows:
                    times[n].append(events(fn, a.iters))
            la = route(True, lambda: term(xd).item())()
            lb = route(False, lambda: term(xd).item())()
            say(f"  {B} x {C} x {H} x {W}, form {form}   (loss: kernels {la:.9f}, ATen {lb:.9f}; workspace {need} bytes)")
            for n, _ in rows:
                say(row(n, times[n]))
            med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
            say(f"    ATen / kernels = {med['TVTerm, ' + ATEN] / med['TVTerm, kernels']:.2f}")
        del ws, dx, x, xd

    say(f"2. the steps, ms per step (wall time over {a.steps} steps ending in a synchronise, after 2 warm-up steps; {a.rounds} rounds, the "
        "rows alternated)")

    def step_rows(title, step):
        rows = [("term off (tv_term=None)", lambda: step(None, None))]
        for form in ("beta", "sq"):
            term = TV.TVTerm(form)
            rows += [(f"{form} on, kernels", route(True, lambda term=term: step(term, 0.1))),
                     (f"{form} on, {ATEN}", route(False, lambda term=term: step(term, 0.1)))]
        times = {n: [] for n, _ in rows}
        for _ in range(a.rounds):
            for n, fn in rows:
                times[n].append(wall(fn, a.steps))
        say(f"  {title}")
        for n, _ in rows:
            say(row(n, times[n]))
        med = {n: sorted(t)[len(t) // 2] for n, t in times.items()}
        off = med["term off (tv_term=None)"]
        for form in ("beta", "sq"):
            say(f"    the {form} term costs {med[form + ' on, kernels'] - off:+.3f} ms per step on the kernels, "
                f"{med[form + ' on, ' + ATEN] - off:+.3f} ms on the ATen formula (medians)")

    torch.manual_seed(0)
    net = ffa.FFA(3, a.blocks).to(dev)
    opt = FlatAdamW(net, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    net.train()
    ty, tx = synthetic_batch(4, 240, seed=1234, device=dev)
    step_rows(f"ffa_train_step, FFA(3, {a.blocks}), L1 [+ 0.1 TVTerm(form)], 4 x 3 x 240 x 240",
              lambda term, w: ffa_train_step(net, None, opt, None, tx, ty) if term is None
              else ffa_train_step(net, None, opt, None, tx, ty, tv_term=term, w_tv=w))
    del net, opt

    torch.manual_seed(0)
    model = M1.Uformer(img_size=128, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff').to(dev)
    opt = FlatAdamW(model)
    model.train()
    ty, tx = synthetic_batch(32, 128, seed=1234, device=dev)
    char = CharbonnierLoss()
    step_rows("train_step, Uformer E = 32, Charbonnier [+ 0.1 TVTerm(form)], no contrastive loss, 32 x 3 x 128 x 128",
              lambda term, w: train_step(model, char, None, opt, None, tx, ty, 1.0, 0) if term is None
              else train_step(model, char, None, opt, None, tx, ty, 1.0, 0, tv_term=term, w_tv=w))
    del model, opt

    say("3. achieved errors against the float64 reference (tests/golden/tv_loss.npz): |value - float64 value| and max |grad - float64 grad| "
        "as a share of max |grad|;")
    say("   reference = the reference function's own fp32 evaluation on the CPU (over its finite pixels on clamped / flat under beta)")
    gold = np.load(os.path.join(ROOT, "tests", "golden", "tv_loss.npz"))
    say(f"    {'case':16s} {'kernels: value':>15s} {'grad':>10s}   {'ATen on device: value':>22s} {'grad':>10s}   {'reference: value':>17s} {'grad':>10s}")
    for name in NAMES:
        for form in ("beta", "sq"):
            key = f"{name}_{form}"
            g64 = torch.from_numpy(gold[key + "_grad"]).double()
            gmax = g64.abs().max().item()
            v64 = float(gold[key + "_f64"])
            term = TV.TVTerm(form)
            res = []
            for kernels in (True, False):
                p = torch.from_numpy(gold[name + "_x"]).to(dev).requires_grad_(True)
                loss = route(kernels, lambda: term(p))()
                loss.backward()
                res += [abs(loss.double().item() - v64), (p.grad.double().cpu() - g64).abs().max().item() / gmax]
            say(f"    {key:16s} {res[0]:15.2e} {res[1]:10.2e}   {res[2]:22.2e} {res[3]:10.2e}   "
                f"{abs(float(gold[key + '_f32']) - v64):17.2e} {float(gold[key + '_grad_err_f32']) / gmax:10.2e}")

    if a.parent:
        torch.cuda.synchronize()
        say(f"4. python bench.py --gpus 1 --steps 30 --warmup 10, the parent commit's build and this tree's alternated, {a.passes} passes each, "
            "a fresh process per run")
        for i in range(a.passes):
            for label, where in (("parent", os.path.abspath(a.parent)), ("this tree", ROOT)):
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "30", "--warmup", "10"], cwd=where, capture_output=True,
                                   text=True, timeout=900)
                out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                say(f"{label}, run {i + 1}:")
                say(out[-1] if r.returncode == 0 and out else f"  FAILED rc={r.returncode}: {r.stderr[-500:]}")
                if r.returncode != 0:
                    write()
                    raise SystemExit("bench_tv_loss.py: bench.py failed; nothing more is started")
    write()


if __name__ == "__main__":
    main()
