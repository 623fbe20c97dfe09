// SSIM as a training loss: loss = 1 - mean(S) and its gradient with respect to the prediction (include/dehaze_hip.h, K15, has the formulas
// and contracts).  The forward is the windowed-moments pass of csrc/metrics.hip with K = 11 and the Gaussian table under both border rules;
// when a gradient is wanted it also stores, per map pixel, the three coefficient maps
//   a = dS/dExx = -S / B2,   b = dS/dExy = 2 A1 / (B1 B2),   m = dS/dmux = 2 muy A2 / (B1 B2) - 2 mux S / B1 - 2 mux a - muy b
// and the backward is one transposed correlation of those maps with the same window:
//   dx(q) = -g / N [ (w^T * m)(q) + 2 x(q) (w^T * a)(q) + y(q) (w^T * b)(q) ]
// Inputs are fp32; every product, window sum, map value and reduction is double (Exx - mux^2 cancels in fp32), so the loss is the float64
// evaluation of the formula rounded once to fp32 and dx the float64 gradient rounded once.
//
// Cuts (functions of the shapes alone), the ones of csrc/metrics.hip: a plane is cut into bands of TW = 32 columns x BH = 64 rows; one
// workgroup of 256 threads walks its band in 8 steps of TH = 8 rows, one pixel per thread per step, staging the (TH + 10) x (TW + 10) halo in
// LDS as doubles (8-byte reads by 32 consecutive lanes per row: conflict-free at any row stride).  The forward's workgroup adds its threads'
// S in a fixed tree and stores one double to the workspace; ssim_loss_finish_kernel (one workgroup) adds the partials - thread t the
// partials t, t + 256, ... in ascending order, then the same fixed tree - and writes 1 - sum / N as fp32.  No atomics: the same bits from run
// to run, under any dhz_set_reserved_cus, with the deterministic mode on or off.
#include "common.h"

namespace {

constexpr int K = 11;
constexpr int TW = 32;       // band width = pixels of a row per half wave
constexpr int TH = 8;        // rows per step (256 threads)
constexpr int BH = 64;       // rows per band
constexpr int STEPS = BH / TH;
constexpr int HW_ = TW + K - 1, HH_ = TH + K - 1;

struct LossArgs {
    const float* x;
    const float* y;
    int H, W, OH, OW;        // plane and map extents
    int off;                 // window origin of map pixel p is p - off: K / 2 under the zero-padded rule, 0 under the valid rule
    int clamp01;
    double C1, C2;
    int bands_x, bands_y;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of the 256 threads' values in a fixed tree (wave shuffles, then the four waves in order); the result is valid in thread 0
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void ssim_loss_fwd_kernel(LossArgs p, const float* __restrict__ window, double* __restrict__ part,
                                                            double* __restrict__ map_m, double* __restrict__ map_a,
                                                            double* __restrict__ map_b) {
    __shared__ double sx[HH_ * HW_];
    __shared__ double sy[HH_ * HW_];
    __shared__ double sw[K * K];
    __shared__ double red[4];
    const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid >> 5;
    const int plane = blockIdx.z;
    const int H = p.H, W = p.W, OH = p.OH, OW = p.OW, off = p.off;
    const float* __restrict__ px_ = p.x + (long)plane * H * W;
    const float* __restrict__ py_ = p.y + (long)plane * H * W;
    const long mbase = (long)plane * OH * OW;
    const int x0 = blockIdx.x * TW, yb = blockIdx.y * BH;
    for (int i = tid; i < K * K; i += 256) sw[i] = (double)window[i];

    double acc = 0.0;
#pragma unroll 1
    for (int st = 0; st < STEPS; ++st) {
        const int y0 = yb + st * TH;
        if (y0 >= OH) break;                                 // uniform over the workgroup: no map row is left in this band
        __syncthreads();                                     // the previous step's reads are done
        for (int i = tid; i < HH_ * HW_; i += 256) {
            const int r = i / HW_, c = i - r * HW_;
            const int gy = y0 - off + r, gx = x0 - off + c;
            float vx = 0.f, vy = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                vx = px_[(long)gy * W + gx];
                vy = py_[(long)gy * W + gx];
                if (p.clamp01) {
                    vx = fminf(fmaxf(vx, 0.f), 1.f);
                    vy = fminf(fmaxf(vy, 0.f), 1.f);
                }
            }
            sx[i] = (double)vx;
            sy[i] = (double)vy;
        }
        __syncthreads();
        const int qy = y0 + ly, qx = x0 + lx;
        if (qy < OH && qx < OW) {
            double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll 1
            for (int ky = 0; ky < K; ++ky) {
                const double* rx = sx + (ly + ky) * HW_ + lx;
                const double* ry = sy + (ly + ky) * HW_ + lx;
                const double* rw = sw + ky * K;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const double w = rw[kx], x = rx[kx], y = ry[kx];
                    mx = fma(w, x, mx);
                    my = fma(w, y, my);
                    mxx = fma(w, x * x, mxx);
                    myy = fma(w, y * y, myy);
                    mxy = fma(w, x * y, mxy);
                }
            }
            {   // every product rounded on its own, as in csrc/metrics.hip: with x == y numerator and denominator are the same doubles, S == 1
#pragma clang fp contract(off)
                const double mxmy = mx * my, mx2 = mx * mx, my2 = my * my;
                const double A1 = 2.0 * mxmy + p.C1, A2 = 2.0 * (mxy - mxmy) + p.C2;
                const double B1 = mx2 + my2 + p.C1, B2 = (mxx - mx2) + (myy - my2) + p.C2;
                const double S = (A1 * A2) / (B1 * B2);
                acc += S;
                if (map_m) {
                    const double a = -S / B2, b = 2.0 * A1 / (B1 * B2);
                    const long o = mbase + (long)qy * OW + qx;
                    map_a[o] = a;
                    map_b[o] = b;
                    map_m[o] = 2.0 * my * A2 / (B1 * B2) - 2.0 * mx * S / B1 - 2.0 * mx * a - my * b;
                }
            }
        }
    }
    const double s = block_sum_d(acc, red);
    if (tid == 0) part[((long)plane * p.bands_y + blockIdx.y) * p.bands_x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const double* __restrict__ part, long nparts, double inv_n,
                                                               float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) *loss = (float)(1.0 - s * inv_n);
}

// output pixel q of the plane gathers map pixels p = q + off - k, k = 0 .. K - 1 each way, with weight w[k]; the tile's map halo starts at
// q0 + off - (K - 1), so halo cell r holds p = q0 + off - (K - 1) + r and meets pixel l of the tile with k = l + K - 1 - r
__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(LossArgs p, const float* __restrict__ window, const float* __restrict__ gloss,
                                                            double neg_inv_n, const double* __restrict__ map_m,
                                                            const double* __restrict__ map_a, const double* __restrict__ map_b,
                                                            float* __restrict__ dx) {
    __shared__ double sm[HH_ * HW_];
    __shared__ double sa[HH_ * HW_];
    __shared__ double sb[HH_ * HW_];
    __shared__ double sw[K * K];
    const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid >> 5;
    const int plane = blockIdx.z;
    const int H = p.H, W = p.W, OH = p.OH, OW = p.OW;
    const long pbase = (long)plane * H * W, mbase = (long)plane * OH * OW;
    const int x0 = blockIdx.x * TW, yb = blockIdx.y * BH;
    for (int i = tid; i < K * K; i += 256) sw[i] = (double)window[K * K - 1 - i];        // flipped both ways: sw[r][c] = w[K-1-r][K-1-c]
    const double scale = (double)gloss[0] * neg_inv_n;

#pragma unroll 1
    for (int st = 0; st < STEPS; ++st) {
        const int y0 = yb + st * TH;
        if (y0 >= H) break;                                  // uniform over the workgroup
        __syncthreads();
        for (int i = tid; i < HH_ * HW_; i += 256) {
            const int r = i / HW_, c = i - r * HW_;
            const int gy = y0 + p.off - (K - 1) + r, gx = x0 + p.off - (K - 1) + c;
            double vm = 0.0, va = 0.0, vb = 0.0;
            if (gy >= 0 && gy < OH && gx >= 0 && gx < OW) {
                const long o = mbase + (long)gy * OW + gx;
                vm = map_m[o];
                va = map_a[o];
                vb = map_b[o];
            }
            sm[i] = vm;
            sa[i] = va;
            sb[i] = vb;
        }
        __syncthreads();
        const int qy = y0 + ly, qx = x0 + lx;
        if (qy < H && qx < W) {
            double am = 0.0, aa = 0.0, ab = 0.0;
#pragma unroll 1
            for (int r = 0; r < K; ++r) {
                const double* rm = sm + (ly + r) * HW_ + lx;
                const double* ra = sa + (ly + r) * HW_ + lx;
                const double* rb = sb + (ly + r) * HW_ + lx;
                const double* rw = sw + r * K;
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const double w = rw[c];
                    am = fma(w, rm[c], am);
                    aa = fma(w, ra[c], aa);
                    ab = fma(w, rb[c], ab);
                }
            }
            const long o = pbase + (long)qy * W + qx;
            float vx = p.x[o], vy = p.y[o];
            bool pass = true;
            if (p.clamp01) {
                pass = vx >= 0.f && vx <= 1.f;               // torch.clamp passes the gradient at the bounds themselves; a NaN passes none
                vx = fminf(fmaxf(vx, 0.f), 1.f);
                vy = fminf(fmaxf(vy, 0.f), 1.f);
            }
            const double g = scale * (am + 2.0 * (double)vx * aa + (double)vy * ab);
            dx[o] = pass ? (float)g : 0.f;
        }
    }
}

bool shape_ok(int B, int C, int H, int W, int valid) {
    if (!(B >= 1 && C >= 1 && H >= 1 && W >= 1 && (long)B * C <= 65535 && H <= 65535 * BH)) return false;           // grid limits
    if ((long)B * C * H * W >= (1l << 31)) return false;
    if (valid != 0 && valid != 1) return false;
    return !valid || (H >= K && W >= K);
}
long bands_of(int H, int W) { return (long)((H + BH - 1) / BH) * ((W + TW - 1) / TW); }
long map_pixels(int B, int C, int H, int W, int valid) { return (long)B * C * (valid ? H - K + 1 : H) * (valid ? W - K + 1 : W); }

struct Plan {
    LossArgs a;
    dim3 grid;
    long nparts, npix;
    double *part, *m, *ma, *mb;
};

int make_plan(const char* who, Plan& pl, const float* x, const float* y, const float* window, const void* scalar, const char* scalar_name,
              void* ws, size_t ws_bytes, int B, int C, int H, int W, int Kw, int valid, double C1, double C2, int clamp01) {
    DHZ_REQUIRE(x && y && window && scalar, "%s: null pointer (x, y, window or %s)", who, scalar_name);
    DHZ_REQUIRE(Kw == K, "%s: K=%d unsupported (11)", who, Kw);
    DHZ_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: bad sizes B=%d C=%d H=%d W=%d (each >= 1)", who, B, C, H, W);
    DHZ_REQUIRE(valid == 0 || valid == 1, "%s: border rule %d (0 zero-padded, 1 valid)", who, valid);
    DHZ_REQUIRE(!valid || (H >= K && W >= K), "%s: the valid rule needs H, W >= K (H=%d W=%d K=%d)", who, H, W, K);
    DHZ_REQUIRE(shape_ok(B, C, H, W, valid), "%s: sizes out of range B=%d C=%d H=%d W=%d (B C <= 65535, H <= 4194240, B C H W < 2^31)", who, B,
                C, H, W);
    const size_t need = dhz_ssim_loss_workspace_bytes(B, C, H, W, valid);
    DHZ_REQUIRE(ws != nullptr, "%s: workspace missing (%zu bytes needed)", who, need);
    DHZ_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu < %zu bytes)", who, ws_bytes, need);
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: the workspace must be 8-byte aligned", who);
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(window) & 3) == 0 && (reinterpret_cast<uintptr_t>(scalar) & 3) == 0,
                "%s: float pointers must be 4-byte aligned", who);
    LossArgs& a = pl.a;
    a = LossArgs{};
    a.x = x; a.y = y;
    a.H = H; a.W = W;
    a.OH = valid ? H - K + 1 : H;
    a.OW = valid ? W - K + 1 : W;
    a.off = valid ? 0 : K / 2;
    a.clamp01 = clamp01 != 0;
    a.C1 = C1; a.C2 = C2;
    a.bands_x = (W + TW - 1) / TW;
    a.bands_y = (H + BH - 1) / BH;
    pl.grid = dim3(a.bands_x, a.bands_y, B * C);
    pl.nparts = (long)B * C * bands_of(H, W);
    pl.npix = map_pixels(B, C, H, W, valid);
    pl.part = static_cast<double*>(ws);
    pl.m = pl.part + pl.nparts;
    pl.ma = pl.m + pl.npix;
    pl.mb = pl.ma + pl.npix;
    return DHZ_OK;
}

}  // namespace

// [partials: one double per (plane, band)] [m] [a] [b]: one double per map pixel each
extern "C" size_t dhz_ssim_loss_workspace_bytes(int B, int C, int H, int W, int valid) {
    if (!shape_ok(B, C, H, W, valid)) return 0;
    return ((size_t)B * C * bands_of(H, W) + 3 * (size_t)map_pixels(B, C, H, W, valid)) * sizeof(double);
}

extern "C" int dhz_ssim_loss_fwd(float* loss, const float* x, const float* y, int B, int C, int H, int W, int K_, const float* window,
                                 int valid, double C1, double C2, int clamp01, int need_grad, void* ws, size_t ws_bytes, void* stream) {
    Plan pl;
    const int rc = make_plan("dhz_ssim_loss_fwd", pl, x, y, window, loss, "loss", ws, ws_bytes, B, C, H, W, K_, valid, C1, C2, clamp01);
    if (rc != DHZ_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool grad = need_grad != 0;
    ssim_loss_fwd_kernel<<<pl.grid, 256, 0, s>>>(pl.a, window, pl.part, grad ? pl.m : nullptr, grad ? pl.ma : nullptr,
                                                 grad ? pl.mb : nullptr);
    DHZ_CHECK_LAUNCH("dhz_ssim_loss_fwd");
    ssim_loss_finish_kernel<<<1, 256, 0, s>>>(pl.part, pl.nparts, 1.0 / (double)pl.npix, loss);
    DHZ_CHECK_LAUNCH("dhz_ssim_loss_fwd (finish)");
    return DHZ_OK;
}

extern "C" int dhz_ssim_loss_bwd(float* dx, const float* gloss, const float* x, const float* y, int B, int C, int H, int W, int K_,
                                 const float* window, int valid, double C1, double C2, int clamp01, void* ws, size_t ws_bytes,
                                 void* stream) {
    DHZ_REQUIRE(dx != nullptr, "dhz_ssim_loss_bwd: null pointer (dx)");
    Plan pl;
    const int rc = make_plan("dhz_ssim_loss_bwd", pl, x, y, window, gloss, "gloss", ws, ws_bytes, B, C, H, W, K_, valid, C1, C2, clamp01);
    if (rc != DHZ_OK) return rc;
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(dx) & 3) == 0, "dhz_ssim_loss_bwd: float pointers must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ssim_loss_bwd_kernel<<<pl.grid, 256, 0, s>>>(pl.a, window, gloss, -1.0 / (double)pl.npix, pl.m, pl.ma, pl.mb, dx);
    DHZ_CHECK_LAUNCH("dhz_ssim_loss_bwd");
    return DHZ_OK;
}
