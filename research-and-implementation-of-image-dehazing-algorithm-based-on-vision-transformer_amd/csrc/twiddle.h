// The float64 twiddle of the analysis kernels (csrc/fourier.hip, csrc/freq_noise.hip), stated once.
#pragma once
#include <hip/hip_runtime.h>

// (cos, sin)(2 pi j / n), 0 <= j < n, from an argument in [0, pi / 4]: quadrant q = floor(4 j / n) and remainder r = 4 j - q n in
// integers, the remainder folded to 2 r <= n by swapping sine and cosine, then the quadrant's rotation
__device__ __forceinline__ double2 dhz_twiddle(int j, int n) {
    const int q = (4 * j) / n;
    int r = 4 * j - q * n;
    const bool fold = 2 * r > n;
    if (fold) r = n - r;
    const double a = (double)r / (double)(2 * n);
    const double sa = sinpi(a), ca = cospi(a);
    const double s0 = fold ? ca : sa, c0 = fold ? sa : ca;
    const double c = q == 0 ? c0 : q == 1 ? -s0 : q == 2 ? -c0 : s0;
    const double s = q == 0 ? s0 : q == 1 ? c0 : q == 2 ? -s0 : -c0;
    return make_double2(c, s);
}
