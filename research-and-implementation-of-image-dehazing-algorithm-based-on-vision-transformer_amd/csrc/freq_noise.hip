// Frequency-band noise (include/dehaze_hip.h, K18, has the formulas and contracts): the reference's FreqAttack._fourier_mask without a 2-D
// transform.  For an n x n plane d, a width w keeps the frequencies B(w) = {-w/2 .. w/2 - 1} on each axis; with
//   c_w[t] = (1/n) sum_{k in B(w)} cos(2 pi k t / n),   s_w[t] = (1/n) sum_{k in B(w)} sin(2 pi k t / n)
// and C_w, S_w their circulants (C_w[a][b] = c_w[(a - b) mod n]),
//   band(d) = (C_w1 d C_w1^T - S_w1 d S_w1^T) - (C_w2 d C_w2^T - S_w2 d S_w2^T),   noise = scale band(d),   out = (float)(x + noise).
// Everything is double; nothing is an atomic; every cut is a function of n, M and the two widths, so two calls give the same bits.
//
// Vectors v = 0 .. 3 are c_w1, s_w1, c_w2, s_w2; a width of 0 contributes nothing, so NV = 2 vectors are live when w2 = 0 and 4 otherwise.
// Stage 1, band_vectors_kernel: one workgroup per live width builds the n twiddles in LDS (integer-reduced index, csrc/twiddle.h) and
//   thread t sums its w entries in ascending k with the index (k t) mod n kept in integers.  ws[v][t], 4 n doubles.
// Stage 2, band_rows_kernel: U_v = d Circ(v)^T, U_v[a][j] = sum_b d[a][b] v[(j - b) mod n].  The rows of all planes are one [M n, n] operand;
//   a workgroup takes 64 rows x 64 columns, a thread 4 x 4 of them for every live vector.  d goes through LDS in runs of 32 columns (as
//   doubles, the sign taken there); the circulant operand is never formed: a thread's four neighbouring columns over four neighbouring b
//   read SEVEN neighbouring entries of v, a window that slides with b, taken from the n + 72 entries of each vector that the column tile
//   can reach (LDS, wrapped there once).  U: ws [M][4][n][n] doubles.
// Stage 3, band_cols_kernel: noise[i][j] = scale sum_v sg_v sum_a v[(i - a) mod n] U_v[a][j], sg = + - - +, v and a ascending.  A workgroup
//   takes 64 x 64 of one plane, U_v through LDS in runs of 32 rows, the same sliding window down the rows.  The epilogue rounds
//   scale * sum, stores it where asked, adds x and rounds once to fp32.
// w1 = w2: band_copy_kernel, out = x bit for bit and noise = +0.0.
#include "common.h"
#include "twiddle.h"

namespace {

constexpr int NMIN = 2, NMAX = 512;
constexpr int T = 64;               // tile side of stages 2 and 3 (rows and columns): 16 x 16 threads of 4 x 4
constexpr int KB = 32;              // contraction run held in LDS
constexpr int KS = KB + 2;          // row stride of the d tile: rows 4 apart fall into different banks, 16-byte alignment kept
constexpr int WIN = T + 8;          // a tile's window of a vector is n + WIN entries

__global__ __launch_bounds__(256) void band_vectors_kernel(double* __restrict__ vec, int n, int w1, int w2) {
    __shared__ double tw[2 * NMAX];
    const int w = blockIdx.x == 0 ? w1 : w2;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double2 t = dhz_twiddle(j, n);
        tw[2 * j] = t.x;
        tw[2 * j + 1] = t.y;
    }
    __syncthreads();
    double* __restrict__ c = vec + (long)(2 * blockIdx.x) * n;
    double* __restrict__ s = c + n;
    const double inv = 1.0 / (double)n;
    for (int t = threadIdx.x; t < n; t += 256) {
        int idx = (int)(((long)(n - w / 2) * t) % n);              // (k t) mod n at k = -w/2
        double cs = 0.0, sn = 0.0;
        for (int k = 0; k < w; ++k) {
            cs += tw[2 * idx];
            sn += tw[2 * idx + 1];
            idx += t;
            if (idx >= n) idx -= n;
        }
        c[t] = cs * inv;
        s[t] = sn * inv;
    }
}

// entries (o + u - 4) mod n, u < n + WIN, of the NV vectors, each times sg[v]: the window a tile at offset o slides over
template <int NV>
__device__ __forceinline__ void load_window(double* __restrict__ lext, const double* __restrict__ vec, int n, int o, bool signs) {
    const int len = n + WIN;
    int start = (o - 4) % n;
    if (start < 0) start += n;
    for (int i = threadIdx.x; i < NV * len; i += 256) {
        const int v = i / len, u = i - v * len;
        const double val = vec[(long)v * n + (start + u) % n];
        lext[i] = signs && (v == 1 || v == 2) ? -val : val;
    }
}

// grid (row tiles of the M n rows, column tiles); LDS: the windows [NV][n + WIN], then the d tile [T][KS]
template <int NV>
__global__ __launch_bounds__(256) void band_rows_kernel(const float* __restrict__ delta, const double* __restrict__ vec, double* __restrict__ U,
                                                        long rows, int n, int take_sign) {
    extern __shared__ __align__(16) double sm[];
    const int len = n + WIN;
    double* lext = sm;
    double* dt = sm + NV * len;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long R0 = (long)blockIdx.x * T;
    const int J0 = blockIdx.y * T;
    load_window<NV>(lext, vec, n, J0, false);
    double acc[NV][4][4];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[v][r][c] = 0.0;
    for (int k0 = 0; k0 < n; k0 += KB) {
        __syncthreads();
        for (int i = tid; i < T * KB; i += 256) {
            const int r = i / KB, b = k0 + (i % KB);
            const long row = R0 + r;
            double d = 0.0;
            if (row < rows && b < n) {
                const float f = delta[row * n + b];
                d = take_sign ? (double)((f > 0.0f) - (f < 0.0f)) : (double)f;
            }
            dt[r * KS + (i % KB)] = d;
        }
        __syncthreads();
#pragma unroll 2
        for (int bb0 = 0; bb0 < KB; bb0 += 4) {
            const int b0 = k0 + bb0;
            if (b0 >= n) break;
            const int u0 = 4 * tx - b0 + n + 1;                    // win[i] = v[(j0 - b0 + i - 3) mod n], j0 = J0 + 4 tx
            double dv[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int b = 0; b < 4; ++b) dv[r][b] = dt[(4 * ty + r) * KS + bb0 + b];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                double win[7];
#pragma unroll
                for (int i = 0; i < 7; ++i) win[i] = lext[v * len + u0 + i];
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[v][r][c] = fma(dv[r][b], win[c - b + 3], acc[v][r][c]);
            }
        }
    }
    const int j0 = J0 + 4 * tx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long row = R0 + 4 * ty + r;
        if (row >= rows) continue;
        const long m = row / n, a = row - m * n;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double* __restrict__ o = U + ((m * 4 + v) * n + a) * n;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j0 + c < n) o[j0 + c] = acc[v][r][c];
        }
    }
}

// grid (column tiles, row tiles, M); LDS: the signed windows [NV][n + WIN], then the U tile [KB][T]
template <int NV>
__global__ __launch_bounds__(256) void band_cols_kernel(float* __restrict__ out, double* __restrict__ noise, const float* __restrict__ x,
                                                        const double* __restrict__ vec, const double* __restrict__ U, int n, double scale) {
    extern __shared__ __align__(16) double sm[];
    const int len = n + WIN;
    double* lext = sm;
    double* ut = sm + NV * len;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int J0 = blockIdx.x * T, I0 = blockIdx.y * T;
    const long m = blockIdx.z;
    load_window<NV>(lext, vec, n, I0, true);
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    for (int v = 0; v < NV; ++v) {
        const double* __restrict__ Uv = U + (m * 4 + v) * n * n;
        for (int k0 = 0; k0 < n; k0 += KB) {
            __syncthreads();
            for (int i = tid; i < KB * T; i += 256) {
                const int a = k0 + i / T, j = J0 + (i % T);
                ut[i] = a < n && j < n ? Uv[(long)a * n + j] : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int aa0 = 0; aa0 < KB; aa0 += 4) {
                const int a0 = k0 + aa0;
                if (a0 >= n) break;
                const int u0 = 4 * ty - a0 + n + 1;                // win[i] = sg v[(i0 - a0 + i - 3) mod n], i0 = I0 + 4 ty
                double win[7], uv[4][4];
#pragma unroll
                for (int i = 0; i < 7; ++i) win[i] = lext[v * len + u0 + i];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int c = 0; c < 4; ++c) uv[a][c] = ut[(aa0 + a) * T + 4 * tx + c];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[r][c] = fma(win[r - a + 3], uv[a][c], acc[r][c]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = I0 + 4 * ty + r;
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = J0 + 4 * tx + c;
            if (j >= n) continue;
            const long at = (m * n + i) * n + j;
            const double nz = __dmul_rn(scale, acc[r][c]);          // rounded before the add: out is (float)(x + the stored noise)
            if (noise) noise[at] = nz;
            out[at] = (float)__dadd_rn((double)x[at], nz);
        }
    }
}

__global__ __launch_bounds__(256) void band_copy_kernel(float* __restrict__ out, double* __restrict__ noise, const float* __restrict__ x, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        out[i] = x[i];
        if (noise) noise[i] = 0.0;
    }
}

bool shape_ok(int M, int n) {
    return n >= NMIN && n <= NMAX && n % 2 == 0 && M >= 1 && M <= 65535 && (long)M * n * n < (1L << 31);
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return p < q + bytes && q < p + bytes;
}

constexpr size_t LDS_MAX = ((size_t)4 * (NMAX + WIN) + (size_t)T * KS) * sizeof(double);
static_assert(LDS_MAX <= 48 * 1024 && (size_t)KB * T <= (size_t)T * KS, "stages 2 and 3 stay inside the LDS a kernel may use without asking");

template <int NV>
void launch_band(float* out, double* noise, const float* x, const float* delta, int M, int n, double scale, int take_sign, double* vec,
                 double* U, hipStream_t s) {
    const long rows = (long)M * n;
    const int tiles = (n + T - 1) / T;
    const size_t lds_r = ((size_t)NV * (n + WIN) + (size_t)T * KS) * sizeof(double);
    const size_t lds_c = ((size_t)NV * (n + WIN) + (size_t)KB * T) * sizeof(double);
    band_rows_kernel<NV><<<dim3((unsigned)((rows + T - 1) / T), tiles), 256, lds_r, s>>>(delta, vec, U, rows, n, take_sign);
    band_cols_kernel<NV><<<dim3(tiles, tiles, M), 256, lds_c, s>>>(out, noise, x, vec, U, n, scale);
}

}  // namespace

// the four vectors [4][n] and the row products [M][4][n][n], as doubles
extern "C" size_t dhz_band_noise_workspace_bytes(int M, int n) {
    if (!shape_ok(M, n)) return 0;
    return ((size_t)4 * n + (size_t)4 * M * n * n) * sizeof(double);
}

extern "C" int dhz_band_noise(float* out, double* noise, const float* x, const float* delta, int M, int n, int w1, int w2, double scale,
                              int take_sign, void* ws, size_t ws_bytes, void* stream) {
    DHZ_REQUIRE(n % 2 == 0, "dhz_band_noise: n=%d is odd (the band widths are even: the side must be)", n);
    DHZ_REQUIRE(n >= NMIN && n <= NMAX, "dhz_band_noise: n=%d out of range (%d <= n <= %d)", n, NMIN, NMAX);
    DHZ_REQUIRE(M >= 1 && M <= 65535, "dhz_band_noise: bad sizes M=%d (1 <= M <= 65535 planes)", M);
    DHZ_REQUIRE((long)M * n * n < (1L << 31), "dhz_band_noise: M n n = %ld elements, 2^31 or more", (long)M * n * n);
    DHZ_REQUIRE(w1 >= 0 && w1 <= n && w1 % 2 == 0 && w2 >= 0 && w2 <= n && w2 % 2 == 0,
                "dhz_band_noise: bad widths w1=%d w2=%d (even, 0 <= w <= n=%d)", w1, w2, n);
    DHZ_REQUIRE(w2 <= w1, "dhz_band_noise: w2=%d exceeds w1=%d (the band is B(w1) x B(w1) minus B(w2) x B(w2))", w2, w1);
    DHZ_REQUIRE(take_sign == 0 || take_sign == 1, "dhz_band_noise: take_sign %d (0 delta as it is, 1 its sign)", take_sign);
    DHZ_REQUIRE(out && x && delta, "dhz_band_noise: null pointer (out, x or delta)");
    const size_t need = dhz_band_noise_workspace_bytes(M, n);
    DHZ_REQUIRE(ws != nullptr, "dhz_band_noise: workspace missing (%zu bytes needed)", need);
    DHZ_REQUIRE(ws_bytes >= need, "dhz_band_noise: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    DHZ_REQUIRE(((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(noise)) & 7) == 0,
                "dhz_band_noise: noise and the workspace must be 8-byte aligned");
    DHZ_REQUIRE(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(delta)) & 3) == 0,
                "dhz_band_noise: out, x and delta must be 4-byte aligned");
    const long total = (long)M * n * n;
    const size_t bytes = (size_t)total * sizeof(float);
    DHZ_REQUIRE(!overlap(out, x, bytes) && !overlap(out, delta, bytes), "dhz_band_noise: out aliases x or delta (it must not overlap either)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (w1 == w2) {
        band_copy_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(out, noise, x, total);
        DHZ_CHECK_LAUNCH("dhz_band_noise (copy)");
        return DHZ_OK;
    }
    double* vec = static_cast<double*>(ws);
    double* U = vec + 4 * (size_t)n;
    const int nw = w2 > 0 ? 2 : 1;
    band_vectors_kernel<<<nw, 256, 0, s>>>(vec, n, w1, w2);
    DHZ_CHECK_LAUNCH("dhz_band_noise (vectors)");
    if (nw == 1) launch_band<2>(out, noise, x, delta, M, n, scale, take_sign, vec, U, s);
    else launch_band<4>(out, noise, x, delta, M, n, scale, take_sign, vec, U, s);
    DHZ_CHECK_LAUNCH("dhz_band_noise (rows, columns)");
    return DHZ_OK;
}
