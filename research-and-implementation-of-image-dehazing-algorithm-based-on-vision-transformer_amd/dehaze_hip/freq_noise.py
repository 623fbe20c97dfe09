"""Frequency-band noise: the reference's FreqAttack._fourier_mask (how-do-vits-work-transformer/ops/adversarial.py:138-175, the "Convs are
vulnerable to high-frequency noise, MSAs to low-frequency noise" experiment) on the HIP kernel dhz_band_noise (csrc/freq_noise.hip;
include/dehaze_hip.h K18).

The reference transforms the perturbation with fft2, shifts, multiplies by the difference of two centred square masks of even widths
w1 >= w2, shifts back and takes the real part of ifft2.  A centred mask of width w keeps the frequencies -w/2 .. w/2 - 1 on each axis,
so the band filter is a pair of circulant products per width and needs no 2-D transform (the header has the identity).

  * `band_widths(f, s, n)` - the reference's two widths for a band centre f (radians) and half-width s.
  * `band_noise(x, delta, w1, w2, scale, take_sign, return_noise)` - x + scale * band(delta or its sign) on [B, C, n, n].

Routing: contiguous fp32 device tensors with n <= 512 take the kernel (float64 arithmetic, no atomics, the same bits from call to call).
DHZ_FREQ_NOISE=0 (or freq_noise.KERNELS = False) evaluates the reference's ATen formula in the input's precision: the A/B arm, and the
route of CPU tensors, other dtypes and larger sides.  Opt-in: nothing on the default paths imports this module.
"""
import math
import os

import torch

from . import _lib

KERNELS = os.environ.get("DHZ_FREQ_NOISE", "1") != "0"     # A/B switch: off = the reference's ATen formula everywhere
NMAX = 512                                                  # the kernel's largest side


def band_widths(f, s, n):
    """(w1, w2) = clip(int((f +- s) n / (2 pi)) * 2, 0, n): adversarial.py:148-149 with _center_mask's clamps; int truncates toward zero"""
    def width(c):
        return min(max(int((c * n) / (2 * math.pi)) * 2, 0), n)
    return width(f + s), width(f - s)


def _geometry(x, delta, w1, w2):
    if not (torch.is_tensor(x) and torch.is_tensor(delta)):
        raise ValueError("band_noise: x and delta are tensors")
    shape = tuple(x.shape)
    if x.dim() != 4 or shape[2] != shape[3]:
        raise ValueError(f"band_noise: x is [B, C, n, n] with square planes, got shape {shape}")
    B, C, n, _ = shape
    if n % 2 or n < 2:
        raise ValueError(f"band_noise: side n={n} must be even and >= 2 (shape {shape})")
    if B < 1 or C < 1:
        raise ValueError(f"band_noise: empty input (shape {shape})")
    if tuple(delta.shape) != shape or delta.dtype != x.dtype or delta.device != x.device:
        raise ValueError(f"band_noise: delta {tuple(delta.shape)} {delta.dtype} {delta.device} does not match x {shape} {x.dtype} {x.device}")
    for w in (w1, w2):
        if int(w) != w or w % 2 or not 0 <= w <= n:
            raise ValueError(f"band_noise: widths w1={w1} w2={w2} must be even integers in [0, n={n}]")
    if w2 > w1:
        raise ValueError(f"band_noise: w2={w2} exceeds w1={w1}")
    return B, C, n


def _center_mask(w, n, device):
    m = torch.zeros(n, n, device=device)
    lo = (n - w) // 2
    m[lo:lo + w, lo:lo + w] = 1.0
    return m


def band_noise_aten(x, delta, w1, w2, scale=1.0, take_sign=False, return_noise=False):
    """The reference's formula in the precision of x: fft2 -> roll by n / 2 -> times (mask(w1) - mask(w2)) -> roll -> ifft2 -> .real.  Its
    abs * exp(i angle) step is the identity on the kept coefficients and is not repeated."""
    B, C, n = _geometry(x, delta, w1, w2)
    d = delta.sign() if take_sign else delta
    if scale != 1.0:
        d = scale * d
    mask = _center_mask(int(w1), n, x.device) - _center_mask(int(w2), n, x.device)
    spec = torch.roll(torch.fft.fft2(d), shifts=(n // 2, n // 2), dims=(2, 3)) * mask
    noise = torch.fft.ifft2(torch.roll(spec, shifts=(n // 2, n // 2), dims=(2, 3))).real
    out = x + noise.to(x.dtype)
    return (out, noise) if return_noise else out


def _kernel(x, delta, w1, w2, scale, take_sign, return_noise):
    B, C, n = _geometry(x, delta, w1, w2)
    lib = _lib.load()
    M = B * C
    nbytes = lib.dhz_band_noise_workspace_bytes(M, n)
    if nbytes == 0:
        raise ValueError(f"band_noise: shape {tuple(x.shape)} is outside the kernel's range (even n <= {NMAX}; B C <= 65535; B C n n < 2^31)")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    out = torch.empty_like(x)
    noise = torch.empty(x.shape, dtype=torch.float64, device=x.device) if return_noise else None
    with torch.cuda.device(x.device):
        _lib.call("dhz_band_noise", out.data_ptr(), noise.data_ptr() if return_noise else None, x.data_ptr(), delta.data_ptr(), M, n,
                  int(w1), int(w2), float(scale), int(bool(take_sign)), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    return (out, noise) if return_noise else out


def band_noise(x, delta, w1, w2, scale=1.0, take_sign=False, return_noise=False):
    """x, delta: [B, C, n, n], n even, the same dtype and device.  Returns x_adv = x + scale * band(d), d = delta or sign(delta) with
    take_sign, restricted to the band of widths (w1, w2); with return_noise (x_adv, noise), the noise in float64 on the kernel route and
    in the input's precision on the ATen route.  A non-square or odd-sided input raises ValueError on both routes."""
    B, C, n = _geometry(x, delta, w1, w2)
    if KERNELS and x.is_cuda and x.dtype == torch.float32 and n <= NMAX:
        return _kernel(x.contiguous(), delta.contiguous(), w1, w2, scale, take_sign, return_noise)
    return band_noise_aten(x.contiguous(), delta.contiguous(), w1, w2, scale, take_sign, return_noise)
