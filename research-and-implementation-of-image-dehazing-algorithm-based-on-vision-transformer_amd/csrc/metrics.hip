// SSIM and the squared error of image pairs, scored on the device in float64 (include/dehaze_hip.h, K14, has the formulas and contracts).
//
// One windowed-moments kernel, two instances (K = 11: FFA_model/metrics.py's Gaussian window; K = 7: the uniform window of utils/metrics.py).
// Per plane it forms the five local moments  sum w x, sum w y, sum w x^2, sum w y^2, sum w x y  over a K x K window whose weights are a table
// argument (the reference's 2-D window is the fp32-rounded outer product, so it is NOT separable to the last bit), the SSIM map and its sum,
// and in the same pass the plane's squared-error sum.  Inputs are fp32 planes; every product, window sum, map value and reduction is double.
//
// Cuts (functions of the shapes alone).  A plane is cut into bands of TW = 32 columns x BH = 64 rows; one workgroup of 256 threads walks its
// band in BH / TH = 8 steps of TH = 8 rows, one pixel per thread per step.  A step stages the (TH + K - 1) x (TW + K - 1) halo of both images
// in LDS as doubles (scalar fp32 loads: no alignment is assumed; taps outside the plane are zeros, clamped on the way in), then every thread
// runs the K x K taps of its pixel.  The two LDS planes are read with 8-byte reads by 32 consecutive lanes per row: one 256-byte bank row
// per half wave, conflict-free at any row stride.  Pixel (py, px) of the plane owns
//   zero-padded rule: map value (py, px), window centred on it (origin py - K/2, px - K/2)
//   valid rule:       map value (py, px) for py <= H - K, px <= W - K, window origin (py, px)
// and, under both rules, its own squared error: fp32 subtraction and fp32 square of the (optionally clamped) inputs, added in double.
// A workgroup adds its threads' values in a fixed tree (wave shuffles, then the four waves in order) and stores one (ssim, sqerr) pair of
// doubles to the workspace; ssim_reduce_kernel adds a plane's pairs in ascending band order, one owner thread per result.  No atomics: the
// same bits from run to run, under any dhz_set_reserved_cus, with the deterministic mode on or off.
#include "common.h"

namespace {

constexpr int TW = 32;       // band width = pixels of a row per half wave
constexpr int TH = 8;        // rows per step (256 threads)
constexpr int BH = 64;       // rows per band
constexpr int STEPS = BH / TH;

struct SsimArgs {
    const float* a;
    const float* b;
    long a_img, a_ch, b_img, b_ch;       // strides in elements; rows are W apart
    int C, H, W;
    int valid, clamp01;
    double wscale, C1, C2, cov_norm;
    int bands_x, bands_y;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int K>
__global__ __launch_bounds__(256) void ssim_pair_kernel(SsimArgs p, const float* __restrict__ window, double* __restrict__ part) {
    constexpr int HW_ = TW + K - 1, HH_ = TH + K - 1;
    __shared__ double sx[HH_ * HW_];
    __shared__ double sy[HH_ * HW_];
    __shared__ double sw[K * K];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, lx = tid & (TW - 1), ly = tid >> 5;
    const int plane = blockIdx.z;
    const int bi = plane / p.C, ci = plane - bi * p.C;
    const float* __restrict__ pa = p.a + (long)bi * p.a_img + (long)ci * p.a_ch;
    const float* __restrict__ pb = p.b + (long)bi * p.b_img + (long)ci * p.b_ch;
    const int H = p.H, W = p.W;
    const int off = p.valid ? 0 : K / 2;
    const int OH = p.valid ? H - K + 1 : H, OW = p.valid ? W - K + 1 : W;        // the map's extent
    const int x0 = blockIdx.x * TW, yb = blockIdx.y * BH;
    for (int i = tid; i < K * K; i += 256) sw[i] = (double)window[i];

    double acc_s = 0.0, acc_e = 0.0;
#pragma unroll 1
    for (int st = 0; st < STEPS; ++st) {
        const int y0 = yb + st * TH;
        if (y0 >= H) break;                                  // uniform over the workgroup
        __syncthreads();                                     // the previous step's reads are done (first step: orders nothing it must not)
        for (int i = tid; i < HH_ * HW_; i += 256) {
            const int r = i / HW_, c = i - r * HW_;
            const int gy = y0 - off + r, gx = x0 - off + c;
            float va = 0.f, vb = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                va = pa[(long)gy * W + gx];
                vb = pb[(long)gy * W + gx];
                if (p.clamp01) {
                    va = fminf(fmaxf(va, 0.f), 1.f);
                    vb = fminf(fmaxf(vb, 0.f), 1.f);
                }
            }
            sx[i] = (double)va;
            sy[i] = (double)vb;
        }
        __syncthreads();
        const int py = y0 + ly, px = x0 + lx;
        if (py < H && px < W) {
            const float fa = (float)sx[(ly + off) * HW_ + lx + off], fb = (float)sy[(ly + off) * HW_ + lx + off];
            const float d = __fsub_rn(fa, fb);
            acc_e += (double)__fmul_rn(d, d);
        }
        if (py < OH && px < OW) {
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
            {   // every product here is rounded on its own: with x == y the numerator and the denominator are then the same doubles, S == 1
#pragma clang fp contract(off)
                mx *= p.wscale; my *= p.wscale; mxx *= p.wscale; myy *= p.wscale; mxy *= p.wscale;
                const double mxmy = mx * my, mx2 = mx * mx, my2 = my * my;
                const double vx = p.cov_norm * (mxx - mx2), vy = p.cov_norm * (myy - my2), vxy = p.cov_norm * (mxy - mxmy);
                const double S = ((2.0 * mxmy + p.C1) * (2.0 * vxy + p.C2)) / ((mx2 + my2 + p.C1) * (vx + vy + p.C2));
                acc_s += S;
            }
        }
    }
    acc_s = wave_sum_d(acc_s);
    acc_e = wave_sum_d(acc_e);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = acc_s;
        red[1][tid >> 6] = acc_e;
    }
    __syncthreads();
    if (tid < 2) {
        const long slot = ((long)plane * p.bands_y + blockIdx.y) * p.bands_x + blockIdx.x;
        part[2 * slot + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    }
}

// thread i owns result (plane i / 2, which = i % 2: 0 the SSIM sum, 1 the squared-error sum) and adds its nb band values in ascending order
__global__ __launch_bounds__(64) void ssim_reduce_kernel(const double* __restrict__ part, double* __restrict__ ssim_sum,
                                                         double* __restrict__ sqerr_sum, int planes, int nb) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * planes) return;
    const int plane = i >> 1, which = i & 1;
    const double* src = part + (long)plane * nb * 2 + which;
    double s = 0.0;
    int t = 0;
    for (; t + 16 <= nb; t += 16) {              // sixteen loads in flight, added in order
        double v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = src[2 * (long)(t + j)];
#pragma unroll
        for (int j = 0; j < 16; ++j) s += v[j];
    }
    for (; t < nb; ++t) s += src[2 * (long)t];
    (which ? sqerr_sum : ssim_sum)[plane] = s;
}

bool shape_ok(int B, int C, int H, int W) {
    return B >= 1 && C >= 1 && H >= 1 && W >= 1 && (long)B * C <= 65535 && H <= 65535 * BH && (long)H * W < (1l << 31);      // grid limits
}
long bands_of(int H, int W) { return (long)((H + BH - 1) / BH) * ((W + TW - 1) / TW); }

}  // namespace

extern "C" size_t dhz_ssim_pair_workspace_bytes(int B, int C, int H, int W) {
    if (!shape_ok(B, C, H, W)) return 0;
    return (size_t)B * C * bands_of(H, W) * 2 * sizeof(double);
}

extern "C" int dhz_ssim_pair(double* ssim_sum, double* sqerr_sum, const float* a, int64_t a_img_stride, int64_t a_ch_stride, const float* b,
                             int64_t b_img_stride, int64_t b_ch_stride, int B, int C, int H, int W, int K, const float* window, double wscale,
                             int valid, double C1, double C2, double cov_norm, int clamp01, void* ws, size_t ws_bytes, void* stream) {
    DHZ_REQUIRE(ssim_sum && sqerr_sum && a && b && window, "dhz_ssim_pair: null pointer");
    DHZ_REQUIRE(K == 7 || K == 11, "dhz_ssim_pair: K=%d unsupported (7 or 11)", K);
    DHZ_REQUIRE(shape_ok(B, C, H, W), "dhz_ssim_pair: bad sizes B=%d C=%d H=%d W=%d (each >= 1, B C <= 65535, H <= 4194240, H W < 2^31)", B, C, H, W);
    DHZ_REQUIRE(valid == 0 || valid == 1, "dhz_ssim_pair: border rule %d (0 zero-padded, 1 valid)", valid);
    DHZ_REQUIRE(!valid || (H >= K && W >= K), "dhz_ssim_pair: the valid rule needs H, W >= K (H=%d W=%d K=%d)", H, W, K);
    DHZ_REQUIRE(a_img_stride >= 0 && a_ch_stride >= 0 && b_img_stride >= 0 && b_ch_stride >= 0, "dhz_ssim_pair: negative stride");
    const size_t need = dhz_ssim_pair_workspace_bytes(B, C, H, W);
    DHZ_REQUIRE(ws != nullptr, "dhz_ssim_pair: workspace missing (%zu bytes needed)", need);
    DHZ_REQUIRE(ws_bytes >= need, "dhz_ssim_pair: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(ssim_sum) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(sqerr_sum) & 7) == 0,
                "dhz_ssim_pair: workspace and outputs must be 8-byte aligned");
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(window) & 3) == 0,
                "dhz_ssim_pair: float pointers must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SsimArgs p{};
    p.a = a; p.b = b;
    p.a_img = a_img_stride; p.a_ch = a_ch_stride; p.b_img = b_img_stride; p.b_ch = b_ch_stride;
    p.C = C; p.H = H; p.W = W;
    p.valid = valid; p.clamp01 = clamp01 != 0;
    p.wscale = wscale; p.C1 = C1; p.C2 = C2; p.cov_norm = cov_norm;
    p.bands_x = (W + TW - 1) / TW;
    p.bands_y = (H + BH - 1) / BH;
    const dim3 grid(p.bands_x, p.bands_y, B * C);
    double* part = static_cast<double*>(ws);
    if (K == 11) ssim_pair_kernel<11><<<grid, 256, 0, s>>>(p, window, part);
    else ssim_pair_kernel<7><<<grid, 256, 0, s>>>(p, window, part);
    DHZ_CHECK_LAUNCH("dhz_ssim_pair");
    const int planes = B * C;
    ssim_reduce_kernel<<<(2 * planes + 63) / 64, 64, 0, s>>>(part, ssim_sum, sqerr_sum, planes, p.bands_x * p.bands_y);
    DHZ_CHECK_LAUNCH("dhz_ssim_pair (reduce)");
    return DHZ_OK;
}
