// Total-variation losses of losses.py (include/dehaze_hip.h, K16, has the formulas and contracts): the value and the gradient with respect
// to x of
//   form 0, "beta" (tv_loss, losses.py:8-18):  coeff sum_sites s^beta / (B C H W),  s = (x[i,j+1] - x[i,j])^2 + (x[i+1,j] - x[i,j])^2 on the
//                                              (H - 1) x (W - 1) sites of a plane;
//   form 1, "sq" (TVLoss, losses.py:25-33):    coeff 2 (sum_v / (C (H - 1) W) + sum_h / (C H (W - 1))) / B over the squared vertical and
//                                              horizontal first differences.
// Inputs are fp32; every difference, square, power and sum is double (a difference of two fp32 values is exact in double, so s == 0 iff
// both differences are zero), the loss is rounded once to fp32 and so is every dx.  Zero-site rule: a site with s == 0 contributes 0 to
// the gradient, where autograd of the formula gives inf * 0 = NaN for beta < 1.
//
// A streaming stencil: no LDS staging - a wave reads 64 consecutive floats of a row, the neighbour reads of the same step hit the same
// lines in the vector cache, so HBM sees every element once.  Cuts (functions of the shapes alone): a plane is cut into bands of TW = 64
// columns x BH = 64 rows; one workgroup of 256 threads walks its band in 16 steps of TH = 4 rows, one pixel per thread per step.  The
// forward's workgroup adds its threads' terms in a fixed tree and stores one double to the workspace; tv_loss_finish_kernel (one
// workgroup) adds the partials - thread t the partials t, t + 256, ... in ascending order, then the same tree - and writes the loss.  The
// backward is a gather: pixel (i, j) recomputes the sites it belongs to from x.  No atomics: the same bits from run to run, under any
// dhz_set_reserved_cus, with the deterministic mode on or off.
#include <cmath>

#include "common.h"

namespace {

constexpr int TW = 64;       // band width = one wave per row
constexpr int TH = 4;        // rows per step (256 threads)
constexpr int BH = 64;       // rows per band
constexpr int STEPS = BH / TH;

struct TvArgs {
    const float* x;
    int H, W;
    int form;                // 0 beta, 1 sq
    double beta;
    double cv, ch;           // sq: 1 / (C (H - 1) W) and 1 / (C H (W - 1)), the weights of a squared vertical / horizontal difference
    double scale;            // beta: coeff / (B C H W); sq: 2 coeff / B
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

// s^beta and d/ds s^beta for s > 0; beta = 0.5, the default, goes through the correctly rounded square root
__device__ __forceinline__ double pow_beta(double s, double beta) { return beta == 0.5 ? sqrt(s) : pow(s, beta); }
__device__ __forceinline__ double dpow_beta(double s, double beta) {
    if (s == 0.0) return 0.0;                                    // the zero-site rule
    return beta == 0.5 ? 0.5 / sqrt(s) : beta * pow(s, beta - 1.0);
}

__global__ __launch_bounds__(256) void tv_loss_fwd_kernel(TvArgs p, double* __restrict__ part) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid >> 6;
    const int plane = blockIdx.z;
    const int H = p.H, W = p.W;
    const float* __restrict__ px = p.x + (long)plane * H * W;
    const int j = blockIdx.x * TW + lx, yb = blockIdx.y * BH;

    double acc = 0.0;
    if (j < W) {
#pragma unroll 4
        for (int st = 0; st < STEPS; ++st) {
            const int i = yb + st * TH + ly;
            if (i >= H) break;
            const float* r = px + (long)i * W + j;
            const double c = (double)r[0];
            const bool right = j + 1 < W, down = i + 1 < H;
            const double dh = right ? (double)r[1] - c : 0.0;
            const double dv = down ? (double)r[W] - c : 0.0;
            if (p.form == 0) {
                if (right && down) {
                    const double s = dh * dh + dv * dv;
                    acc += pow_beta(s, p.beta);
                }
            } else {
                acc += p.cv * (dv * dv) + p.ch * (dh * dh);
            }
        }
    }
    const double s = block_sum_d(acc, red);
    if (tid == 0) part[((long)plane * p.bands_y + blockIdx.y) * p.bands_x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void tv_loss_finish_kernel(const double* __restrict__ part, long nparts, double scale,
                                                             float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum_d(s, red);
    if (threadIdx.x == 0) *loss = (float)(scale * s);
}

// beta: pixel (i, j) belongs to site (i, j) as its corner, to site (i, j - 1) as its right end and to site (i - 1, j) as its lower end
//   d s(i,j) / d x[i,j] = -2 (dh + dv),   d s(i,j-1) / d x[i,j] = 2 dh(i,j-1),   d s(i-1,j) / d x[i,j] = 2 dv(i-1,j)
// sq: the four first differences that end or start at the pixel
__global__ __launch_bounds__(256) void tv_loss_bwd_kernel(TvArgs p, const float* __restrict__ gloss, float* __restrict__ dx) {
    const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid >> 6;
    const int plane = blockIdx.z;
    const int H = p.H, W = p.W;
    const long pbase = (long)plane * H * W;
    const float* __restrict__ px = p.x + pbase;
    const int j = blockIdx.x * TW + lx, yb = blockIdx.y * BH;
    if (j >= W) return;
    const double g = (double)gloss[0];
    const bool left = j >= 1, right = j + 1 < W;
#pragma unroll 2
    for (int st = 0; st < STEPS; ++st) {
        const int i = yb + st * TH + ly;
        if (i >= H) break;
        const bool up = i >= 1, down = i + 1 < H;
        const float* r = px + (long)i * W + j;
        const double c = (double)r[0];
        double sum = 0.0;
        if (p.form == 0) {
            if (right && down) {
                const double dh = (double)r[1] - c, dv = (double)r[W] - c;
                sum -= dpow_beta(dh * dh + dv * dv, p.beta) * (dh + dv);
            }
            if (left && down) {
                const double o = (double)r[-1];
                const double dh = c - o, dv = (double)r[W - 1] - o;
                sum += dpow_beta(dh * dh + dv * dv, p.beta) * dh;
            }
            if (up && right) {
                const double o = (double)r[-W];
                const double dh = (double)r[1 - W] - o, dv = c - o;
                sum += dpow_beta(dh * dh + dv * dv, p.beta) * dv;
            }
        } else {
            double v = 0.0, h = 0.0;
            if (up) v += c - (double)r[-W];
            if (down) v -= (double)r[W] - c;
            if (left) h += c - (double)r[-1];
            if (right) h -= (double)r[1] - c;
            sum = p.cv * v + p.ch * h;
        }
        dx[pbase + (long)i * W + j] = (float)(g * (2.0 * p.scale * sum));
    }
}

bool shape_ok(int B, int C, int H, int W) {
    if (!(B >= 1 && C >= 1 && H >= 2 && W >= 2 && (long)B * C <= 65535 && H <= 65535 * BH)) return false;           // grid limits
    return (long)B * C * H * W < (1l << 31);
}
long bands_of(int H, int W) { return (long)((H + BH - 1) / BH) * ((W + TW - 1) / TW); }

struct Plan {
    TvArgs a;
    dim3 grid;
    long nparts;
};

int make_plan(const char* who, Plan& pl, const float* x, const void* scalar, const char* scalar_name, int B, int C, int H, int W, int form,
              double beta, double coeff) {
    DHZ_REQUIRE(x && scalar, "%s: null pointer (x or %s)", who, scalar_name);
    DHZ_REQUIRE(form == 0 || form == 1, "%s: form %d (0 beta, 1 sq)", who, form);
    DHZ_REQUIRE(std::isfinite(beta) && beta > 0.0, "%s: beta=%g (finite and > 0)", who, beta);
    DHZ_REQUIRE(B >= 1 && C >= 1 && H >= 2 && W >= 2, "%s: bad sizes B=%d C=%d H=%d W=%d (B, C >= 1; H, W >= 2: a plane needs a site)", who, B,
                C, H, W);
    DHZ_REQUIRE(shape_ok(B, C, H, W), "%s: sizes out of range B=%d C=%d H=%d W=%d (B C <= 65535, H <= 4194240, B C H W < 2^31)", who, B, C, H,
                W);
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(scalar) & 3) == 0,
                "%s: float pointers must be 4-byte aligned", who);
    TvArgs& a = pl.a;
    a = TvArgs{};
    a.x = x;
    a.H = H; a.W = W;
    a.form = form;
    a.beta = beta;
    a.cv = 1.0 / ((double)C * (H - 1) * W);
    a.ch = 1.0 / ((double)C * H * (W - 1));
    a.scale = form == 0 ? coeff / ((double)B * C * H * W) : 2.0 * coeff / (double)B;
    a.bands_x = (W + TW - 1) / TW;
    a.bands_y = (H + BH - 1) / BH;
    pl.grid = dim3(a.bands_x, a.bands_y, B * C);
    pl.nparts = (long)B * C * bands_of(H, W);
    return DHZ_OK;
}

}  // namespace

// one double per (plane, band)
extern "C" size_t dhz_tv_loss_workspace_bytes(int B, int C, int H, int W) {
    if (!shape_ok(B, C, H, W)) return 0;
    return (size_t)B * C * bands_of(H, W) * sizeof(double);
}

extern "C" int dhz_tv_loss_fwd(float* loss, const float* x, int B, int C, int H, int W, int form, double beta, double coeff, void* ws,
                               size_t ws_bytes, void* stream) {
    Plan pl;
    const int rc = make_plan("dhz_tv_loss_fwd", pl, x, loss, "loss", B, C, H, W, form, beta, coeff);
    if (rc != DHZ_OK) return rc;
    const size_t need = dhz_tv_loss_workspace_bytes(B, C, H, W);
    DHZ_REQUIRE(ws != nullptr, "dhz_tv_loss_fwd: workspace missing (%zu bytes needed)", need);
    DHZ_REQUIRE(ws_bytes >= need, "dhz_tv_loss_fwd: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "dhz_tv_loss_fwd: the workspace must be 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(ws);
    tv_loss_fwd_kernel<<<pl.grid, 256, 0, s>>>(pl.a, part);
    DHZ_CHECK_LAUNCH("dhz_tv_loss_fwd");
    tv_loss_finish_kernel<<<1, 256, 0, s>>>(part, pl.nparts, pl.a.scale, loss);
    DHZ_CHECK_LAUNCH("dhz_tv_loss_fwd (finish)");
    return DHZ_OK;
}

extern "C" int dhz_tv_loss_bwd(float* dx, const float* gloss, const float* x, int B, int C, int H, int W, int form, double beta,
                               double coeff, void* stream) {
    DHZ_REQUIRE(dx != nullptr, "dhz_tv_loss_bwd: null pointer (dx)");
    Plan pl;
    const int rc = make_plan("dhz_tv_loss_bwd", pl, x, gloss, "gloss", B, C, H, W, form, beta, coeff);
    if (rc != DHZ_OK) return rc;
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(dx) & 3) == 0, "dhz_tv_loss_bwd: float pointers must be 4-byte aligned");
    tv_loss_bwd_kernel<<<pl.grid, 256, 0, static_cast<hipStream_t>(stream)>>>(pl.a, gloss, dx);
    DHZ_CHECK_LAUNCH("dhz_tv_loss_bwd");
    return DHZ_OK;
}
