"""dhz_winograd_conv3x3 vs MIOpen (torch conv2d) on the VGG19 layer shapes, batch 64 (forward) .
SLICES=1: the per-shape table of the channel-sliced launches instead (see slices_table).
ANY=1: the maps of 64 / 192 / 384-pixel patches on dhz_winograd_conv3x3_any against the library convolution (see any_table)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd"))
import torch, torch.nn.functional as F
from dehaze_hip import _lib
dev = torch.device("cuda:0"); s = torch.cuda.current_stream().cuda_stream
def timeit(f, n=10):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
def slices_table():
    """SLICES=1: the step's under-filled launches (128 x 128 patches: 32 differentiated, 64 reference images), each as the plain launch it
    replaces against the sliced launch PLUS its epilogue kernel, for both kernels and every slice count the entries take.  ROUNDS rounds with
    the variants alternating inside a round; a variant's figure is the median of its rounds, its spread max - min over the rounds.  A shape
    is dispatched only where the sliced launch wins by more than the spread (profiles/r08_wino_slices.txt)."""
    rounds = int(os.environ.get("ROUNDS", 3))
    shapes = [("conv5_1 no-grad  B64", 64, 8, 512, 512, False), ("conv5_1 forward  B32", 32, 8, 512, 512, False),
              ("conv5_1 dgrad    B32", 32, 8, 512, 512, True), ("conv4_1 dgrad    B32", 32, 16, 512, 256, True),
              ("conv4_1 forward  B32", 32, 16, 256, 512, False), ("conv4_2-4 forward B32", 32, 16, 512, 512, False),
              ("conv4_2-4 dgrad  B32", 32, 16, 512, 512, True), ("conv3_1 dgrad    B32", 32, 32, 256, 128, True)]
    print(f"{'launch':22s} {'variant':10s} {'median us':>10s} {'spread us':>10s}   (rounds: {rounds})")
    for name, B, H, C, K, bwd in shapes:
        w = torch.randn(K, C, 3, 3, device=dev) * 0.05
        bias = torch.randn(K, device=dev)
        xb = torch.randn(B, C // 8, H, H, 8, device=dev)
        yb = torch.empty(B, K // 8, H, H, 8, device=dev)
        ws = torch.empty(4, B, K // 8, H, H, 8, device=dev)
        mask = torch.randn(B, K // 8, H, H, 8, device=dev) if bwd else None
        ep = (None, 0, mask.data_ptr(), None) if bwd else (bias.data_ptr(), 1, None, None)
        ups = {}
        for pre, npos in (("dhz_winograd_prepack", 16), ("dhz_winograd43_prepack", 36)):
            ups[npos] = torch.empty(npos * K * C, device=dev)
            _lib.call(pre, w.data_ptr(), ups[npos].data_ptr(), K, C, 0, s)
        variants = {"f22": lambda: _lib.call("dhz_winograd_conv3x3", xb.data_ptr(), ups[16].data_ptr(), *ep, yb.data_ptr(), B, H, H, C, K, s)}
        for S in (2, 4):
            variants[f"f22 S={S}"] = lambda S=S: _lib.call("dhz_winograd_conv3x3_slices", xb.data_ptr(), ups[16].data_ptr(), *ep, yb.data_ptr(),
                                                           ws.data_ptr(), S, B, H, H, C, K, s)
        if H >= 16:
            variants["f43"] = lambda: _lib.call("dhz_winograd43_conv3x3", xb.data_ptr(), ups[36].data_ptr(), *ep, yb.data_ptr(), B, H, H, C, K, s)
            for S in (2, 4):
                if (C // 8) % S == 0 and C // 8 // S <= 32:
                    variants[f"f43 S={S}"] = lambda S=S: _lib.call("dhz_winograd43_conv3x3_slices", xb.data_ptr(), ups[36].data_ptr(), *ep,
                                                                   yb.data_ptr(), ws.data_ptr(), S, B, H, H, C, K, s)
        t = {v: [] for v in variants}
        for _ in range(rounds):
            for v, f in variants.items():
                t[v].append(timeit(f, 20))
        for v, ts in t.items():
            print(f"{name:22s} {v:10s} {sorted(ts)[len(ts) // 2]:10.1f} {max(ts) - min(ts):10.1f}")


def any_table():
    """ANY=1: the layers whose maps only dhz_winograd_conv3x3_any takes (and the 8 x 8 layers of 64-pixel patches beside them), each as the
    library convolution the feature stack ran for it before (NCHW conv2d + ReLU; aten convolution_backward's input gradient + the ReLU mask)
    against the any-size launch, plain and in 2 / 4 channel slices (launch + epilogue kernel).  `rule` is what dhz_winograd_slices_any
    answers for the shape.  ROUNDS rounds, variants alternating inside a round; median and max - min over the rounds
    (profiles/wino_any_maps.txt)."""
    rounds = int(os.environ.get("ROUNDS", 3))
    lib = _lib.load()
    # (patch, batch): B differentiated images, 2 B no-gradient ones
    shapes = []
    for patch, B, layers in ((64, 32, (("conv4_1", 8, 256, 512), ("conv4_2-4", 8, 512, 512), ("conv5_1", 4, 512, 512))),
                             (192, 8, (("conv4_1", 24, 256, 512), ("conv4_2-4", 24, 512, 512), ("conv5_1", 12, 512, 512))),
                             (384, 2, (("conv5_1", 24, 512, 512),))):
        for lname, H, C, K in layers:
            shapes += [(f"{patch:3d}px {lname:9s} no-grad B{2 * B}", 2 * B, H, C, K, False), (f"{patch:3d}px {lname:9s} forward B{B}", B, H, C, K, False),
                       (f"{patch:3d}px {lname:9s} dgrad   B{B}", B, H, K, C, True)]
    print(f"{'launch':32s} {'map':>7s} {'C->K':>9s} {'blocks':>6s} {'rule':>4s} {'variant':9s} {'median us':>10s} {'spread us':>10s}   (rounds: {rounds})")
    for name, B, H, C, K, bwd in shapes:
        # C, K: the kernel's input / output channels (backward-data: those of the forward layer swapped)
        w = torch.randn(C, K, 3, 3, device=dev) * 0.05 if bwd else torch.randn(K, C, 3, 3, device=dev) * 0.05
        bias = torch.randn(K, device=dev)
        x = torch.randn(B, C, H, H, device=dev)
        act = torch.relu(torch.randn(B, K, H, H, device=dev))
        xb = torch.randn(B, C // 8, H, H, 8, device=dev)
        yb = torch.empty(B, K // 8, H, H, 8, device=dev)
        ws = torch.empty(4, B, K // 8, H, H, 8, device=dev)
        mask = torch.relu(torch.randn(B, K // 8, H, H, 8, device=dev)) if bwd else None
        ep = (None, 0, mask.data_ptr(), None) if bwd else (bias.data_ptr(), 1, None, None)
        up = torch.empty(16 * K * C, device=dev)
        _lib.call("dhz_winograd_prepack", w.data_ptr(), up.data_ptr(), K, C, int(bwd), s)
        if bwd:
            def library():
                g = torch.ops.aten.convolution_backward(x, act, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0]
                return torch.ops.aten.threshold_backward(g, act, 0)
        else:
            def library():
                return F.relu(F.conv2d(x, w, bias, padding=1))
        variants = {"library": library,
                    "any": lambda: _lib.call("dhz_winograd_conv3x3_any", xb.data_ptr(), up.data_ptr(), *ep, yb.data_ptr(), B, H, H, C, K, s)}
        for S in (2, 4):
            variants[f"any S={S}"] = lambda S=S: _lib.call("dhz_winograd_conv3x3_any_slices", xb.data_ptr(), up.data_ptr(), *ep, yb.data_ptr(),
                                                           ws.data_ptr(), S, B, H, H, C, K, s)
        t = {v: [] for v in variants}
        for _ in range(rounds):
            for v, f in variants.items():
                t[v].append(timeit(f, 20))
        for v, ts in t.items():
            print(f"{name:32s} {H:3d}x{H:<3d} {C:4d}>{K:<4d} {lib.dhz_winograd_any_blocks(B, H, H):6d} {lib.dhz_winograd_slices_any(B, H, H, C, K):4d} "
                  f"{v:9s} {sorted(ts)[len(ts) // 2]:10.1f} {max(ts) - min(ts):10.1f}")


if os.environ.get("SLICES"):
    slices_table()
    sys.exit(0)
if os.environ.get("ANY"):
    any_table()
    sys.exit(0)
B = int(os.environ.get("B", 64))
F43 = os.environ.get("F43")          # F43=1: the F(4x4,3x3) kernel (dhz_winograd43_*) instead of F(2x2,3x3)
PRE, ENT, NPOS = ("dhz_winograd43_prepack", "dhz_winograd43_conv3x3", 36) if F43 else ("dhz_winograd_prepack", "dhz_winograd_conv3x3", 16)
for C, K, H in [(64, 64, 128), (64, 128, 64), (128, 128, 64), (128, 256, 32), (256, 256, 32), (256, 512, 16), (512, 512, 16)]:
    x = torch.randn(B, C, H, H, device=dev); w = torch.randn(K, C, 3, 3, device=dev) * 0.05; b = torch.randn(K, device=dev)
    xb = torch.empty(B, C // 8, H, H, 8, device=dev); yb = torch.empty(B, K // 8, H, H, 8, device=dev)
    up = torch.empty(NPOS * K * C, device=dev)
    _lib.call(PRE, w.data_ptr(), up.data_ptr(), K, C, 0, s)
    t_m = timeit(lambda: _lib.call(ENT, xb.data_ptr(), up.data_ptr(), b.data_ptr(), 1, None, None, yb.data_ptr(), B, H, H, C, K, s))
    t_l = timeit(lambda: F.relu(F.conv2d(x, w, b, padding=1))) if not os.environ.get("NO_LIB") else float("nan")
    fl = 2.0 * B * H * H * C * K * 9
    print(f"C {C:4d} K {K:4d} H {H:4d}: wino-mfma {t_m:8.1f} us ({fl/t_m/1e6:6.1f} TF-equiv)   miopen+relu {t_l:8.1f} us ({fl/t_l/1e6:6.1f} TF-equiv)   x{t_l/t_m:.2f}")
