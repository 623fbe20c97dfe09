// Fourier and variance analysis of feature maps (include/dehaze_hip.h, K17, has the formulas and contracts): per n x n map f of a latent
//   A[k] = log(|F[k][k]| + 1e-6), k < n / 2      the half diagonal of the shifted log-amplitude spectrum (fourier_analysis.ipynb)
//   V    = the unbiased variance over the n^2 positions                                          (featuremap_variance.ipynb)
// and the sums of both over all maps.  The diagonal needs no 2-D transform: with g[s] = sum of f[y][x] over (y + x) mod n = s,
//   F[k][k] = sum_s g[s] exp(-2 pi i k s / n),
// so the analysis is ONE read of the latent (stage 1), an n-point DFT of n / 2 frequencies per map (stage 2) and a sum over maps
// (stage 3).  Everything is double; nothing is an atomic; every cut is a function of the shapes, so two calls give the same bits.
//
// Stage 1, fourier_partial_*: the rows of a map are cut into `chunks` runs of R rows (plan(): R >= 8, enough workgroups for the chip
//   where the maps are few).  Gather form: a thread OWNS residues s and adds f[y][(s - y) mod n] over the rows y of its run in a
//   register, so every element is read once, by one thread, and no two threads meet in a sum.  The same loads feed the variance
//   sums sum(f - f0) and sum((f - f0)^2) around the map's first element f0.
//     tokens [B, n n, C]: a workgroup takes 32 channels; a thread V = 4 consecutive channels (16-byte loads) where C % 4 == 0, else
//       V = 1; neighbouring lanes own neighbouring channels, then neighbouring residues: a wave reads whole runs of pixels.
//     NCHW [B, C, n, n]: a map takes LP lanes, the power of two >= n (8 .. 256), and a workgroup 256 / LP maps; lane t of a map owns
//       the residues t, t + LP, ...: neighbouring lanes read neighbouring floats of a row, and small maps leave no lanes idle.
//   The partial g go to the workspace ([b][chunk][s][c] / [b][c][chunk][s]), the variance pairs to [b][chunk][c][2].
// Stage 2, fourier_finish_kernel: a workgroup takes FT channels of one image (32 for n <= 512, 4 above: n FT doubles of g and the n
//   twiddles live in LDS), adds the chunks in ascending order, and thread (k, c) forms F[k][k] over s = 0 .. n - 1 in that order.
//   The twiddle index is (k s) mod n, kept in integers; the table entry of j comes from an argument reduced to the first octant.
// Stage 3, fourier_sum_kernel: sum over the M = B C maps, partial j = maps j, j + 16, ... in ascending order, then partials 0 .. 15 in
//   order.
#include <atomic>
#include <cmath>

#include "common.h"
#include "twiddle.h"

namespace {

constexpr int NMIN = 2, NMAX = 2048;
constexpr int CT = 32;              // channels per stage-1 workgroup (tokens)
constexpr int RMIN = 8;             // least rows per chunk
constexpr int WG_TARGET = 1024;     // stage-1 workgroups wanted where the maps are few
constexpr int FT_SMALL = 32, FT_LARGE = 4, N_SMALL = 512;      // stage 2: channels per workgroup by side
constexpr int SUMJ = 16;            // stage 3: partial sums per column

struct Plan {
    int R, chunks, FT;
    size_t g_elems, v_elems;        // doubles
};

bool shape_ok(int B, int C, int n, int layout) {
    return B >= 1 && C >= 1 && B <= 65535 && C <= 65535 && n >= NMIN && n <= NMAX && n % 2 == 0 && (layout == 0 || layout == 1);
}

Plan plan(int B, int C, int n, int layout) {
    Plan p;
    const long units = layout == 0 ? (long)B * ((C + CT - 1) / CT) : (long)B * C;
    const long want = (WG_TARGET + units - 1) / units;
    long R = (n + want - 1) / want;
    if (R < RMIN) R = RMIN;
    p.R = (int)R;
    p.chunks = (n + p.R - 1) / p.R;
    p.FT = n <= N_SMALL ? FT_SMALL : FT_LARGE;
    p.g_elems = (size_t)B * p.chunks * n * C;
    p.v_elems = (size_t)B * p.chunks * C * 2;
    return p;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int V, class T> struct LoadV;
template <class T> struct LoadV<1, T> {
    static __device__ __forceinline__ void ld(const T* p, double (&v)[1]) { v[0] = (double)ld1(p); }
};
template <class T> struct LoadV<4, T> {
    static __device__ __forceinline__ void ld(const T* p, double (&v)[4]) {
        const float4 r = ld4(p);
        v[0] = (double)r.x; v[1] = (double)r.y; v[2] = (double)r.z; v[3] = (double)r.w;
    }
};

// tokens: grid (chunks, ceil(C / 32), B); thread = (channel group cl, residue group sg), 32 / V channel groups x 8 V residue groups
template <int V, class T>
__global__ __launch_bounds__(256) void fourier_partial_tokens_kernel(const T* __restrict__ x, double* __restrict__ wg, double* __restrict__ wv,
                                                                     int n, int C, int R, int chunks) {
    constexpr int CL = CT / V, SG = 256 / CL;
    __shared__ double red[2][SG][CT];
    const int tid = threadIdx.x, cl = tid % CL, sg = tid / CL;
    const int c = blockIdx.y * CT + cl * V, b = blockIdx.z, ch = blockIdx.x;
    const int y0 = ch * R, y1 = min(n, y0 + R);
    double s1[V], s2[V];
#pragma unroll
    for (int i = 0; i < V; ++i) s1[i] = s2[i] = 0.0;
    if (c < C) {                                                   // V = 4 only where C % 4 == 0: a group is inside or outside as a whole
        const T* __restrict__ xb = x + (long)b * n * n * C + c;
        double f0[V];
        LoadV<V, T>::ld(xb, f0);
        double* __restrict__ g = wg + ((long)b * chunks + ch) * n * C + c;
        for (int s = sg; s < n; s += SG) {
            double acc[V];
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = 0.0;
            int xx = s - y0;
            if (xx < 0) xx += n;
#pragma unroll 4
            for (int y = y0; y < y1; ++y) {
                double v[V];
                LoadV<V, T>::ld(xb + ((long)y * n + xx) * C, v);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const double d = v[i] - f0[i];
                    acc[i] += v[i];
                    s1[i] += d;
                    s2[i] += d * d;
                }
                xx = xx == 0 ? n - 1 : xx - 1;
            }
#pragma unroll
            for (int i = 0; i < V; ++i) g[(long)s * C + i] = acc[i];
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        red[0][sg][cl * V + i] = s1[i];
        red[1][sg][cl * V + i] = s2[i];
    }
    __syncthreads();
    if (tid < CT && blockIdx.y * CT + tid < C) {                   // the residue groups of a channel in ascending order
        double a = 0.0, q = 0.0;
        for (int j = 0; j < SG; ++j) {
            a += red[0][j][tid];
            q += red[1][j][tid];
        }
        double* o = wv + (((long)b * chunks + ch) * C + blockIdx.y * CT + tid) * 2;
        o[0] = a;
        o[1] = q;
    }
}

// NCHW: grid (chunks, C, B); lane t owns the residues t, t + 256, ...
// NCHW: grid (map groups, chunks, more map groups); LP lanes per map (the power of two >= n, 8 .. 256), MP = 256 / LP maps per workgroup; lane t of a
// map owns the residues t, t + LP, ...
template <int LP, class T>
__global__ __launch_bounds__(256) void fourier_partial_nchw_kernel(const T* __restrict__ x, double* __restrict__ wg, double* __restrict__ wv, int n,
                                                                   int C, long maps, int R, int chunks) {
    constexpr int MP = 256 / LP, WAVES = LP > 64 ? LP / 64 : 1;
    __shared__ double red[2][4];
    const int tid = threadIdx.x, t = tid % LP;
    const long m = ((long)blockIdx.z * gridDim.x + blockIdx.x) * MP + tid / LP;              // map b C + c
    const int ch = blockIdx.y;
    const int y0 = ch * R, y1 = min(n, y0 + R);
    double s1 = 0.0, s2 = 0.0;
    if (m < maps) {
        const T* __restrict__ xm = x + m * n * n;
        const double f0 = (double)ld1(xm);
        double* __restrict__ g = wg + (m * chunks + ch) * n;
        for (int s = t; s < n; s += LP) {
            double acc = 0.0;
            int xx = s - y0;
            if (xx < 0) xx += n;
#pragma unroll 4
            for (int y = y0; y < y1; ++y) {
                const double v = (double)ld1(xm + (long)y * n + xx);
                const double d = v - f0;
                acc += v;
                s1 += d;
                s2 += d * d;
                xx = xx == 0 ? n - 1 : xx - 1;
            }
            g[s] = acc;
        }
    }
    // the lanes of a map in a fixed tree: shuffles inside a wave (a map's lanes are an aligned group of LP), then its waves in order
#pragma unroll
    for (int o = (LP < 64 ? LP : 64) / 2; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if constexpr (WAVES > 1) {
        if ((tid & 63) == 0) {
            red[0][tid >> 6] = s1;
            red[1][tid >> 6] = s2;
        }
        __syncthreads();
        if (t == 0) {
            s1 = red[0][tid >> 6];
            s2 = red[1][tid >> 6];
            for (int w = 1; w < WAVES; ++w) {
                s1 += red[0][(tid >> 6) + w];
                s2 += red[1][(tid >> 6) + w];
            }
        }
    }
    if (t == 0 && m < maps) {
        const long b = m / C, c = m - b * C;
        double* o = wv + ((b * chunks + ch) * C + c) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

// grid (ceil(C / FT), B); LDS: g [n][FT] doubles, then the twiddles [n][2]
template <int LAYOUT>
__global__ __launch_bounds__(256) void fourier_finish_kernel(const double* __restrict__ wg, const double* __restrict__ wv, double* __restrict__ A,
                                                             double* __restrict__ Vout, int n, int C, int chunks, int FT) {
    extern __shared__ __align__(16) double sm[];
    double* gl = sm;
    double* tw = sm + (long)n * FT;
    const int tid = threadIdx.x, b = blockIdx.y, c0 = blockIdx.x * FT;
    const int ft = min(FT, C - c0), half = n / 2;
    for (int i = tid; i < n * ft; i += 256) {
        int s, cl;
        long base, step;
        if (LAYOUT == 0) {
            cl = i % ft; s = i / ft;
            base = ((long)b * chunks * n + s) * C + c0 + cl;
            step = (long)n * C;
        } else {
            s = i % n; cl = i / n;
            base = ((long)b * C + c0 + cl) * chunks * n + s;
            step = n;
        }
        double acc = 0.0;
        for (int ch = 0; ch < chunks; ++ch) acc += wg[base + ch * step];
        gl[s * FT + cl] = acc;
    }
    for (int j = tid; j < n; j += 256) {
        const double2 t = dhz_twiddle(j, n);
        tw[2 * j] = t.x;
        tw[2 * j + 1] = t.y;
    }
    __syncthreads();
    for (int o = tid; o < half * ft; o += 256) {
        const int cl = o % ft, k = o / ft;
        double re = 0.0, im = 0.0;
        int idx = 0;                                               // (k s) mod n
        for (int s = 0; s < n; ++s) {
            const double gv = gl[s * FT + cl];
            re += gv * tw[2 * idx];
            im -= gv * tw[2 * idx + 1];
            idx += k;
            if (idx >= n) idx -= n;
        }
        A[((long)b * C + c0 + cl) * half + k] = log(hypot(re, im) + 1e-6);
    }
    if (tid < ft) {
        double a = 0.0, q = 0.0;
        for (int ch = 0; ch < chunks; ++ch) {
            const double* p = wv + (((long)b * chunks + ch) * C + c0 + tid) * 2;
            a += p[0];
            q += p[1];
        }
        const double N = (double)n * (double)n;
        Vout[(long)b * C + c0 + tid] = fmax(0.0, (q - a * a / N) / (N - 1.0));
    }
}

// grid ceil(half / 16) + 1: the last workgroup sums V (one column)
__global__ __launch_bounds__(256) void fourier_sum_kernel(const double* __restrict__ A, const double* __restrict__ V, double* __restrict__ sumA,
                                                          double* __restrict__ sumV, long M, int half) {
    __shared__ double part[SUMJ][16];
    const int kl = threadIdx.x & 15, j = threadIdx.x >> 4;
    const bool var = blockIdx.x == gridDim.x - 1;
    const double* src = var ? V : A;
    double* dst = var ? sumV : sumA;
    const int K = var ? 1 : half;
    const int k = var ? kl : blockIdx.x * 16 + kl;
    double acc = 0.0;
    if (k < K) {
        constexpr int UN = 16;                                     // UN loads in flight, added in the same ascending order
        long m = j;
        for (; m + (UN - 1) * SUMJ < M; m += UN * SUMJ) {
            double v[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) v[u] = src[(m + u * SUMJ) * K + k];
#pragma unroll
            for (int u = 0; u < UN; ++u) acc += v[u];
        }
        for (; m < M; m += SUMJ) acc += src[m * K + k];
    }
    part[j][kl] = acc;
    __syncthreads();
    if (j == 0 && k < K) {
        double t = part[0][kl];
        for (int i = 1; i < SUMJ; ++i) t += part[i][kl];
        dst[k] = t;
    }
}

template <class T>
void launch_partial(const T* x, double* wg, double* wv, int B, int C, int n, int layout, const Plan& p, hipStream_t s) {
    if (layout == 0) {
        const dim3 grid(p.chunks, (C + CT - 1) / CT, B);
        const bool vec = C % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (4 * sizeof(T) - 1)) == 0;
        if (vec) fourier_partial_tokens_kernel<4, T><<<grid, 256, 0, s>>>(x, wg, wv, n, C, p.R, p.chunks);
        else fourier_partial_tokens_kernel<1, T><<<grid, 256, 0, s>>>(x, wg, wv, n, C, p.R, p.chunks);
    } else {
        const long maps = (long)B * C;
        int LP = 8;
        while (LP < n && LP < 256) LP *= 2;
        const long groups = (maps + 256 / LP - 1) / (256 / LP);          // up to 2^32: over x and z, 2^20 per z at the most
        const long gz = (groups + (1L << 20) - 1) >> 20, gx = (groups + gz - 1) / gz;
        const dim3 grid((unsigned)gx, p.chunks, (unsigned)gz);
#define DHZ_FOURIER_NCHW(L) \
    case L: fourier_partial_nchw_kernel<L, T><<<grid, 256, 0, s>>>(x, wg, wv, n, C, maps, p.R, p.chunks); break
        switch (LP) {
            DHZ_FOURIER_NCHW(8);
            DHZ_FOURIER_NCHW(16);
            DHZ_FOURIER_NCHW(32);
            DHZ_FOURIER_NCHW(64);
            DHZ_FOURIER_NCHW(128);
            DHZ_FOURIER_NCHW(256);
        }
#undef DHZ_FOURIER_NCHW
    }
}

// Stage 2 keeps up to LDS_MAX bytes of dynamic LDS (n = 512: 32 channels of g and the twiddles).  The allowance above 48 KiB is asked for
// once per instantiation and device, for that maximum, and its answer is kept: a refusal is this entry's error, not a later launch failure.
constexpr size_t LDS_MAX = ((size_t)N_SMALL * FT_SMALL + 2 * (size_t)N_SMALL) * sizeof(double);
static_assert(LDS_MAX <= 160 * 1024 && ((size_t)NMAX * FT_LARGE + 2 * (size_t)NMAX) * sizeof(double) <= LDS_MAX, "stage 2 exceeds the LDS");
constexpr int MAX_DEVICES = 64;

template <int LAYOUT>
hipError_t finish_allow_lds() {
    static std::atomic<int> state[MAX_DEVICES];      // 0 not asked, 1 granted, 2 + hipError_t refused
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
    int st = state[dev].load(std::memory_order_acquire);
    if (st == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fourier_finish_kernel<LAYOUT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
        st = e == hipSuccess ? 1 : 2 + (int)e;
        state[dev].store(st, std::memory_order_release);
    }
    return st == 1 ? hipSuccess : (hipError_t)(st - 2);
}

}  // namespace

// the partial g vectors and variance pairs of stage 1, as doubles
extern "C" size_t dhz_fourier_diag_workspace_bytes(int B, int C, int n, int layout) {
    if (!shape_ok(B, C, n, layout)) return 0;
    const Plan p = plan(B, C, n, layout);
    return (p.g_elems + p.v_elems) * sizeof(double);
}

extern "C" int dhz_fourier_diag(double* A, double* V, double* sumA, double* sumV, const void* x, int B, int C, int n, int layout, int dtype,
                                void* ws, size_t ws_bytes, void* stream) {
    DHZ_REQUIRE(n % 2 == 0, "dhz_fourier_diag: n=%d is odd (the half diagonal needs an even side)", n);
    DHZ_REQUIRE(n >= NMIN && n <= NMAX, "dhz_fourier_diag: n=%d out of range (%d <= n <= %d)", n, NMIN, NMAX);
    DHZ_REQUIRE(layout == 0 || layout == 1, "dhz_fourier_diag: layout %d (0 tokens [B, n n, C], 1 NCHW [B, C, n, n])", layout);
    DHZ_REQUIRE(dtype == DHZ_F32 || dtype == DHZ_BF16, "dhz_fourier_diag: dtype %d (DHZ_F32 = 0, DHZ_BF16 = 1)", dtype);
    DHZ_REQUIRE(B >= 1 && C >= 1 && B <= 65535 && C <= 65535, "dhz_fourier_diag: bad sizes B=%d C=%d (1 <= B, C <= 65535)", B, C);
    DHZ_REQUIRE(A && V && sumA && sumV && x, "dhz_fourier_diag: null pointer (A, V, sumA, sumV or x)");
    const size_t need = dhz_fourier_diag_workspace_bytes(B, C, n, layout);
    DHZ_REQUIRE(ws != nullptr, "dhz_fourier_diag: workspace missing (%zu bytes needed)", need);
    DHZ_REQUIRE(ws_bytes >= need, "dhz_fourier_diag: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    const size_t elem = dtype == DHZ_F32 ? 4 : 2;
    DHZ_REQUIRE((reinterpret_cast<uintptr_t>(x) & (elem - 1)) == 0, "dhz_fourier_diag: x must be aligned to its element size");
    DHZ_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(sumA) |
                  reinterpret_cast<uintptr_t>(sumV) | reinterpret_cast<uintptr_t>(ws)) & 7) == 0,
                "dhz_fourier_diag: A, V, sumA, sumV and the workspace must be 8-byte aligned");
    const Plan p = plan(B, C, n, layout);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* wg = static_cast<double*>(ws);
    double* wv = wg + p.g_elems;
    if (dtype == DHZ_F32) launch_partial(static_cast<const float*>(x), wg, wv, B, C, n, layout, p, s);
    else launch_partial(static_cast<const bf16s*>(x), wg, wv, B, C, n, layout, p, s);
    DHZ_CHECK_LAUNCH("dhz_fourier_diag (partial)");
    const size_t lds = ((size_t)n * p.FT + 2 * (size_t)n) * sizeof(double);
    const dim3 fgrid((C + p.FT - 1) / p.FT, B);
    if (lds > 48 * 1024) {
        const hipError_t e = layout == 0 ? finish_allow_lds<0>() : finish_allow_lds<1>();
        if (e != hipSuccess) {
            dhz_set_error("dhz_fourier_diag: %zu bytes of LDS for stage 2 were refused: %s", lds, hipGetErrorString(e));
            return DHZ_ELAUNCH;
        }
    }
    if (layout == 0) fourier_finish_kernel<0><<<fgrid, 256, lds, s>>>(wg, wv, A, V, n, C, p.chunks, p.FT);
    else fourier_finish_kernel<1><<<fgrid, 256, lds, s>>>(wg, wv, A, V, n, C, p.chunks, p.FT);
    DHZ_CHECK_LAUNCH("dhz_fourier_diag (finish)");
    const int half = n / 2;
    fourier_sum_kernel<<<(half + 15) / 16 + 1, 256, 0, s>>>(A, V, sumA, sumV, (long)B * C, half);
    DHZ_CHECK_LAUNCH("dhz_fourier_diag (sum)");
    return DHZ_OK;
}
