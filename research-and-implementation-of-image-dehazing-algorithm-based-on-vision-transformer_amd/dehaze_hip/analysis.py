"""Fourier and variance analysis of feature maps: the reference's fourier_analysis.ipynb and featuremap_variance.ipynb (the "how do
ViTs work" evidence: MSA is a low-pass filter, Conv / MLP amplify high frequencies) on the HIP kernel dhz_fourier_diag
(csrc/fourier.hip; include/dehaze_hip.h K17).

The notebooks move every latent to the CPU, run fft2 on [B, C, n, n], take log(|F| + 1e-6), average over batch and channels and keep
only the half diagonal of the shifted spectrum.  The diagonal needs no 2-D transform: with g[s] the sum of f[y][x] over
(y + x) mod n = s,  F[k][k] = sum_s g[s] exp(-2 pi i k s / n) - one read of the latent in the layout the model holds it in.

  * `diag_log_amplitude(x, layout, per_map)` - per map A[b, c, k] = log(|F[k][k]| + 1e-6), k < n / 2, and V[b, c] = the unbiased
    variance over the n^2 positions; by default their sums over the B C maps (the caller divides by the map count).
  * `tap_plan(model)`, `taps(model)` - the latents of a Uformer forward in forward order, each reduced where it is tapped.
  * `write_csv` / `read_csv` - the two tables My_fourier_analysis.py writes.

Routing: fp32 or bf16 device tensors take the kernel (float64 arithmetic, no atomics, the same bits from call to call).  DHZ_FOURIER=0 (or
analysis.KERNELS = False) evaluates the same quantities with the notebook's ATen formula in the input's precision: the A/B arm, and the
route of CPU tensors (fp32, bf16 or fp64 there).  Opt-in: nothing on the default paths imports this module.
"""
import contextlib
import csv
import functools
import math
import os

import torch

from . import _lib

KERNELS = os.environ.get("DHZ_FOURIER", "1") != "0"        # A/B switch: off = the notebook's ATen formula everywhere
LAYOUTS = {"tokens": 0, "nchw": 1}
SUM_PARTS = 16                                              # the kernel's sum over maps: partial j = maps j, j + 16, ..., then j ascending


def _geometry(x, layout):
    """(B, C, n) of a latent, or ValueError naming the shape"""
    if layout not in LAYOUTS:
        raise ValueError(f"diag_log_amplitude: layout={layout!r} ('tokens' [B, n*n, C] or 'nchw' [B, C, n, n])")
    if not torch.is_tensor(x):
        raise ValueError(f"diag_log_amplitude: a tensor is needed, got {type(x).__name__}")
    shape = tuple(x.shape)
    if layout == "tokens":
        if x.dim() != 3:
            raise ValueError(f"diag_log_amplitude: tokens are [B, n*n, C], got shape {shape}")
        B, L, C = shape
        n = math.isqrt(L)
        if n * n != L:
            raise ValueError(f"diag_log_amplitude: {L} tokens are no square map (shape {shape})")
    else:
        if x.dim() != 4 or shape[2] != shape[3]:
            raise ValueError(f"diag_log_amplitude: NCHW latents are [B, C, n, n] with square maps, got shape {shape}")
        B, C, n, _ = shape
    if n % 2 or n < 2:
        raise ValueError(f"diag_log_amplitude: side n={n} must be even and >= 2 (shape {shape})")
    if B < 1 or C < 1:
        raise ValueError(f"diag_log_amplitude: empty latent (shape {shape})")
    return B, C, n


def diag_log_amplitude_aten(x, layout="tokens", per_map=False):
    """The notebook's formula: fft2 -> log(abs + 1e-6) -> shift by n / 2 -> .diag()[n/2:], and latent.var(dim=[-1, -2]), per map, in the
    precision of x (bf16 computes in fp32); the results are returned as float64.  Sums are torch's over (B, C)."""
    B, C, n = _geometry(x, layout)
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise ValueError(f"diag_log_amplitude: dtype {x.dtype} of shape {tuple(x.shape)} (fp32, bf16 or fp64)")
    lat = x.reshape(B, n, n, C).permute(0, 3, 1, 2) if layout == "tokens" else x
    if lat.dtype == torch.bfloat16:
        lat = lat.float()
    amp = torch.log(torch.fft.fft2(lat).abs() + 1e-6)
    amp = torch.roll(amp, shifts=(n // 2, n // 2), dims=(-2, -1))
    A = torch.diagonal(amp, dim1=-2, dim2=-1)[..., n // 2:].double()
    V = lat.var(dim=[-1, -2]).double()
    return (A, V) if per_map else (A.sum(dim=(0, 1)), V.sum())


def _kernel(x, layout, per_map):
    B, C, n = _geometry(x, layout)
    x = x.contiguous()
    lib = _lib.load()
    code = LAYOUTS[layout]
    nbytes = lib.dhz_fourier_diag_workspace_bytes(B, C, n, code)
    if nbytes == 0:
        raise ValueError(f"diag_log_amplitude: shape {tuple(x.shape)} is outside the kernel's range (even n <= 2048; B, C <= 65535)")
    f64 = dict(dtype=torch.float64, device=x.device)
    ws = torch.empty(nbytes // 8, **f64)
    A, V = torch.empty((B, C, n // 2), **f64), torch.empty((B, C), **f64)
    sumA, sumV = torch.empty(n // 2, **f64), torch.empty((), **f64)
    with torch.cuda.device(x.device):
        _lib.call("dhz_fourier_diag", A.data_ptr(), V.data_ptr(), sumA.data_ptr(), sumV.data_ptr(), x.data_ptr(), B, C, n, code,
                  0 if x.dtype == torch.float32 else 1, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    return (A, V) if per_map else (sumA, sumV)


def diag_log_amplitude(x, layout="tokens", per_map=False):
    """x: tokens [B, n*n, C] or NCHW [B, C, n, n], n even.  Returns float64 tensors on x's device: (sum over maps of A [n/2], sum over maps
    of V, a scalar), or with per_map (A [B, C, n/2], V [B, C]).  A non-square token count, an odd side or an unsupported dtype raises
    ValueError naming the shape."""
    if KERNELS and torch.is_tensor(x) and x.is_cuda:
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"diag_log_amplitude: dtype {x.dtype} of shape {tuple(x.shape)} (the kernel reads fp32 or bf16)")
        return _kernel(x, layout, per_map)
    return diag_log_amplitude_aten(x, layout, per_map)


def fixed_order_sum(v):
    """The kernel's sum over maps of per-map values v [B, C, ...] (float64), restated: partial j = maps j, j + 16, ... in ascending
    order, then the 16 partials in ascending order.  Bit-identical to the sums diag_log_amplitude returns on the kernel route."""
    v = v.reshape((v.shape[0] * v.shape[1],) + tuple(v.shape[2:]))
    parts = []
    for j in range(SUM_PARTS):
        acc = torch.zeros_like(v[0])
        for m in range(j, v.shape[0], SUM_PARTS):
            acc = acc + v[m]
        parts.append(acc)
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


# ----------------------------------------------------------------------------- taps

KINDS = ("proj", "msa", "mlp", "pool", "up")


def tap_plan(model):
    """[(name, kind, side, channels)] of the latents a Uformer forward passes, in forward order, from the module tree alone (no forward):
    the output of input_proj (proj); per LeWin block the tensor after the attention residual (msa) and after the LeFF / Mlp residual
    (mlp); every dowsample_i output (pool); every upsample_i output after the skip concat (up).  The 3-channel output is no tap."""
    from .model import Uformer
    if not isinstance(model, Uformer):
        raise TypeError(f"taps: a My_model_1.Uformer or My_model.Uformer is needed, got {type(model).__name__}")
    plan = [("input_proj", "proj", model.reso, model.embed_dim)]

    def blocks(stage):
        for i, blk in enumerate(getattr(model, stage).blocks):
            for kind in ("msa", "mlp"):
                plan.append((f"{stage}.blocks.{i}.{kind}", kind, blk.input_resolution[0], blk.dim))

    for s in range(4):
        blocks(f"encoderlayer_{s}")
        plan.append((f"dowsample_{s}", "pool", model.reso // 2 ** (s + 1), getattr(model, f"dowsample_{s}").out_channel))
    blocks("conv")
    for s in range(4):
        dec = getattr(model, f"decoderlayer_{s}")
        plan.append((f"upsample_{s}", "up", dec.input_resolution[0], dec.dim))
        blocks(f"decoderlayer_{s}")
    return plan


class Collector:
    """Receives the tapped latents of one or more forwards and reduces each where it is tapped (diag_log_amplitude on the token layout),
    so that no latent outlives its tap.  Per tap it keeps float64 device accumulators - the sum of A over maps and the sum of V - across
    batches; results() reads them back once."""

    def __init__(self, plan):
        self.plan = list(plan)
        self.order = []                               # tap indices in the order they arrived, all forwards
        self._sumA = [None] * len(self.plan)
        self._sumV = [None] * len(self.plan)
        self._maps = [0] * len(self.plan)
        self._shape = [None] * len(self.plan)

    def add(self, i, x):
        x = x.detach()
        sumA, sumV = diag_log_amplitude(x, "tokens")
        B, L, C = x.shape
        if self._shape[i] is None:
            self._shape[i], self._sumA[i], self._sumV[i] = (math.isqrt(L), C), sumA, sumV        # fresh tensors of this call
        elif self._shape[i] != (math.isqrt(L), C):
            raise ValueError(f"taps: {self.plan[i][0]} changed from side, channels {self._shape[i]} to {(math.isqrt(L), C)} between forwards")
        else:
            self._sumA[i] += sumA
            self._sumV[i] += sumV
        self._maps[i] += B * C
        self.order.append(i)

    def results(self):
        """One row per tap that fired, in plan order: dict(index, name, kind, n, channels, maps, curve = mean A [n/2] as a list,
        delta = curve - curve[0], variance = mean V).  One device-to-host copy."""
        live = [i for i in range(len(self.plan)) if self._maps[i]]
        if not live:
            return []
        flat = torch.cat([self._sumA[i] for i in live] + [torch.stack([self._sumV[i] for i in live])]).cpu().tolist()
        rows, at = [], 0
        var = flat[len(flat) - len(live):]
        for j, i in enumerate(live):
            n, C = self._shape[i]
            curve = [v / self._maps[i] for v in flat[at:at + n // 2]]
            at += n // 2
            rows.append(dict(index=i, name=self.plan[i][0], kind=self.plan[i][1], n=n, channels=C, maps=self._maps[i], curve=curve,
                             delta=[v - curve[0] for v in curve], variance=var[j] / self._maps[i]))
        return rows


@contextlib.contextmanager
def taps(model):
    """with taps(model) as collector: model(x) ...  While active, the forward of a My_model_1.Uformer / My_model.Uformer hands the
    collector the latents of tap_plan(model) in forward order.  The block-internal tensor (msa) exists only when a block runs its two
    branches as two calls: the block's `_tap` makes it do so for the tapped forwards only; the rest are forward hooks.  On exit the
    hooks and attributes are gone: a plain forward launches what it launched before."""
    plan = tap_plan(model)
    col = Collector(plan)
    index = {name: i for i, (name, _, _, _) in enumerate(plan)}
    handles, tapped = [], []

    def hook(i):
        return lambda module, args, out: col.add(i, out)

    try:
        for name, i in index.items():
            if name.endswith(".msa"):
                blk = model.get_submodule(name[:-4])
                blk._tap = functools.partial(col.add, i)
                tapped.append(blk)
            elif name.endswith(".mlp"):
                handles.append(model.get_submodule(name[:-4]).register_forward_hook(hook(i)))
            else:
                handles.append(model.get_submodule(name).register_forward_hook(hook(i)))
        yield col
    finally:
        for h in handles:
            h.remove()
        for blk in tapped:
            del blk._tap                              # back to the class attribute (None)


# ----------------------------------------------------------------------------- tables

def write_csv(prefix, rows):
    """PREFIX_fourier.csv: index, name, kind, side n, channels, maps, then delta[k] = mean A[k] - mean A[0], k < n / 2 (ragged rows; the last
    column is the notebook's high-frequency figure).  PREFIX_variance.csv: index, name, kind, mean variance.  No header lines.
    Returns the two paths."""
    fpath, vpath = prefix + "_fourier.csv", prefix + "_variance.csv"
    os.makedirs(os.path.dirname(os.path.abspath(fpath)), exist_ok=True)
    with open(fpath, "w", newline="") as f:
        w = csv.writer(f)
        for r in rows:
            w.writerow([r["index"], r["name"], r["kind"], r["n"], r["channels"], r["maps"]] + [repr(float(v)) for v in r["delta"]])
    with open(vpath, "w", newline="") as f:
        w = csv.writer(f)
        for r in rows:
            w.writerow([r["index"], r["name"], r["kind"], repr(float(r["variance"]))])
    return fpath, vpath


def read_csv(prefix):
    """the rows write_csv wrote: dict(index, name, kind, n, channels, maps, delta, variance)"""
    rows = []
    with open(prefix + "_fourier.csv", newline="") as f:
        for rec in csv.reader(f):
            rows.append(dict(index=int(rec[0]), name=rec[1], kind=rec[2], n=int(rec[3]), channels=int(rec[4]), maps=int(rec[5]),
                             delta=[float(v) for v in rec[6:]]))
    with open(prefix + "_variance.csv", newline="") as f:
        for r, rec in zip(rows, csv.reader(f)):
            if (int(rec[0]), rec[1], rec[2]) != (r["index"], r["name"], r["kind"]):
                raise ValueError(f"{prefix}_variance.csv: row {rec[:3]} does not match {prefix}_fourier.csv")
            r["variance"] = float(rec[3])
    return rows
