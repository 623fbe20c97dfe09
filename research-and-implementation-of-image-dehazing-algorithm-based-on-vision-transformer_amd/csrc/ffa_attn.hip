// FFA-Net's own layers (FFA_model/models/FFA.py) on the channel-blocked layout [B][8][H*W][8] of the Winograd kernels, fp32, C = 64:
// channel attention (global mean -> 1x1 -> ReLU -> 1x1 -> sigmoid gate, FFA.py:24-38), pixel attention (per-pixel 64 -> 8 -> 1 gate,
// FFA.py:9-21), their composition with the block residual (FFA.py:54-56, G = 1) and the fusion head over the three group outputs
// (FFA.py:105-108, G = 3: the concatenated tensor is never built).  include/dehaze_hip.h, K13, has the formulas and the contracts.
//
// Cuts (functions of the shapes alone).  The entries without `_any` take H and W in multiples of 16, so H*W is a multiple of 256 and every
// workgroup below is full; the `_any` entries take any H, W >= 1 on the same launch code (on a multiple-of-16 shape: the same launch):
//   pooling      chunks of PCH = 1024 pixels (the last one may be shorter, of any length), one 64-vector per (image, group, chunk)
//   gate forward / backward-b   one thread per pixel / per float4, nothing reduced; ceil(HW / 256) workgroups per image, pixels >= HW idle
//   backward-a   chunks of BCH = 128 pixels, ceil(HW / 128) per image, one slot of slot_len(G) floats per (image, chunk):
//                [dca 64 G | dWp1 512 | dbp1 8 | dwp2 8 | dbp2 1].  In a partly filled last chunk the pixels >= HW are neither loaded nor
//                stored and enter the slot's sums as zeros
//   ca_bwd       level 1 sums SEG = 16 consecutive slots per (image, segment), level 2 (one workgroup per image) the segments, level 3 the
//                images, all in ascending order
// No atomics anywhere: the same bits from run to run, under any dhz_set_reserved_cus, with the deterministic mode on or off.
#include "common.h"

namespace {

constexpr int PCH = 1024;      // pixels per pooling chunk
constexpr int BCH = 128;       // pixels per backward-a workgroup
constexpr int SEG = 16;        // backward-a slots per level-1 segment
constexpr int NPA = 529;       // dWp1 512 | dbp1 8 | dwp2 8 | dbp2 1

__host__ __device__ inline int slot_len(int G) { return 64 * G + 532; }      // 64 G + NPA rounded up to a multiple of 4
// one image's share of the parameter gradients: dWa, dWb (64 G x hc each), dba (hc), dbb (64 G), the NPA pixel-attention sums; padded
__host__ __device__ inline int img_len(int G) { return (G == 1 ? 2 * 64 * 8 + 8 + 64 : 2 * 192 * 4 + 4 + 192) + 532; }

struct Maps { const float* m[3]; };
struct MapsOut { float* m[3]; };

struct Cut {
    bool ok, ragged;
    long HW;
    int npch, nbch, nseg, slot;
    size_t fwd_floats, bwd_a_floats, seg_floats, bwd_floats;
};

// any: the `_any` entries (H, W >= 1); otherwise multiples of 16.  ragged: HW is no multiple of 256 - the bounded kernel instances
Cut make_cut(int B, int H, int W, int G, bool any) {
    Cut c{};
    c.ok = B >= 1 && (any ? H >= 1 && W >= 1 : H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0) && (G == 1 || G == 3) &&
           (long)H * W * 64 < (1l << 31);
    if (!c.ok) return c;
    c.HW = (long)H * W;
    c.ragged = c.HW % 256 != 0;
    c.npch = (int)((c.HW + PCH - 1) / PCH);
    c.nbch = (int)((c.HW + BCH - 1) / BCH);
    c.nseg = (c.nbch + SEG - 1) / SEG;
    c.slot = slot_len(G);
    c.fwd_floats = (size_t)B * G * c.npch * 64;
    c.bwd_a_floats = (size_t)B * c.nbch * c.slot;
    c.seg_floats = (size_t)B * c.nseg * c.slot;
    c.bwd_floats = c.bwd_a_floats + c.seg_floats + (size_t)B * img_len(G);
    return c;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- (a) stage 1: partial channel sums of one (image, group, pooling chunk).  Thread t reads float4 number t + 256 k of an octet's
// [pixels][8] slab: its half of the octet (t & 1) is fixed, so it sums 4 channels over its pixels; lanes of equal parity are summed by
// shuffles, the four waves through LDS.
__global__ __launch_bounds__(256) void ffa_pool_kernel(Maps maps, float* __restrict__ part, int HW, int npch, int G) {
    __shared__ float red[4][64];
    const int ch = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = ch * PCH;
    const int np = min(PCH, HW - p0);                      // pixels of this chunk (any number: thread t sums float4s t, t + 256, ... < 2 np)
    const float* __restrict__ m = maps.m[g] + (size_t)b * 64 * HW;
#pragma unroll 1
    for (int o = 0; o < 8; ++o) {
        const float* src = m + ((size_t)o * HW + p0) * 8;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < 2 * np; i += 256) acc += ld4v(src + 4 * (size_t)i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = acc[j];
#pragma unroll
            for (int s = 32; s > 1; s >>= 1) v += __shfl_xor(v, s);
            acc[j] = v;
        }
        if (lane < 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[wave][o * 8 + lane * 4 + j] = acc[j];
        }
    }
    __syncthreads();
    if (tid < 64) part[(((size_t)b * G + g) * npch + ch) * 64 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---- (a) stage 2: one workgroup per image: chunk partials in ascending order, then the gate MLP
__global__ __launch_bounds__(256) void ffa_ca_mlp_kernel(const float* __restrict__ part, const float* __restrict__ Wa,
                                                         const float* __restrict__ ba, const float* __restrict__ Wb,
                                                         const float* __restrict__ bb, float* __restrict__ mean, float* __restrict__ hid,
                                                         float* __restrict__ ca, int HW, int npch, int G) {
    __shared__ float smean[192];
    __shared__ float shid[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = 64 * G, hc = G == 1 ? 8 : 4;
    if (tid < n) {
        const float* src = part + ((size_t)b * G + (tid >> 6)) * npch * 64 + (tid & 63);
        float s = 0.f;
        for (int c = 0; c < npch; ++c) s += src[(size_t)c * 64];
        s *= 1.0f / (float)HW;
        smean[tid] = s;
        mean[(size_t)b * n + tid] = s;
    }
    __syncthreads();
    if (tid < hc) {
        float s = ba[tid];
        for (int k = 0; k < n; ++k) s = fmaf(Wa[tid * n + k], smean[k], s);
        s = fmaxf(s, 0.f);
        shid[tid] = s;
        hid[(size_t)b * hc + tid] = s;
    }
    __syncthreads();
    if (tid < n) {
        float s = bb[tid];
        for (int j = 0; j < hc; ++j) s = fmaf(Wb[tid * hc + j], shid[j], s);
        ca[(size_t)b * n + tid] = sigmoidf_(s);
    }
}

// pixel-attention parameters + one image's channel gates in LDS
struct PaSmem {
    float w1[8][64];
    float b1[8], w2[8];
    float b2;
    float ca[192];
};

__device__ __forceinline__ void stage_pa(PaSmem& S, const float* __restrict__ ca, const float* __restrict__ Wp1,
                                         const float* __restrict__ bp1, const float* __restrict__ wp2, const float* __restrict__ bp2,
                                         int b, int G, int nthr) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 512; i += nthr) (&S.w1[0][0])[i] = Wp1[i];
    if (tid < 8) { S.b1[tid] = bp1[tid]; S.w2[tid] = wp2[tid]; }
    if (tid == 0) S.b2 = bp2[0];
    for (int i = tid; i < 64 * G; i += nthr) S.ca[i] = ca[(size_t)b * 64 * G + i];
    __syncthreads();
}

// t[c] = sum_g ca[g][c] m_g[c][p] for one pixel, channels in registers
__device__ __forceinline__ void load_t(float (&t)[64], const Maps& maps, const PaSmem& S, size_t img, int HW, int p, int G) {
#pragma unroll
    for (int c = 0; c < 64; ++c) t[c] = 0.f;
    for (int g = 0; g < G; ++g) {
        const float* __restrict__ m = maps.m[g] + img;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const f32x4 lo = ld4v(m + ((size_t)o * HW + p) * 8), hi = ld4v(m + ((size_t)o * HW + p) * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t[o * 8 + j] = fmaf(S.ca[g * 64 + o * 8 + j], lo[j], t[o * 8 + j]);
                t[o * 8 + 4 + j] = fmaf(S.ca[g * 64 + o * 8 + 4 + j], hi[j], t[o * 8 + 4 + j]);
            }
        }
    }
}

// h[i] = Wp1[i] . t + bp1[i] (before the ReLU), pg = sigmoid(wp2 . relu(h) + bp2)
__device__ __forceinline__ float pixel_gate(const float (&t)[64], float (&h)[8], const PaSmem& S) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float s = S.b1[i];
#pragma unroll
        for (int c = 0; c < 64; ++c) s = fmaf(S.w1[i][c], t[c], s);
        h[i] = s;
    }
    float z = S.b2;
#pragma unroll
    for (int i = 0; i < 8; ++i) z = fmaf(S.w2[i], fmaxf(h[i], 0.f), z);
    return sigmoidf_(z);
}

// ---- (b) out = t * pg (+ res): one pixel per thread, 256 pixels of one image per workgroup (RAGGED: the last one may hold fewer)
template <bool RAGGED>
__global__ __launch_bounds__(256) void ffa_gate_pa_fwd_kernel(Maps maps, const float* __restrict__ ca, const float* __restrict__ Wp1,
                                                              const float* __restrict__ bp1, const float* __restrict__ wp2,
                                                              const float* __restrict__ bp2, const float* __restrict__ res,
                                                              float* __restrict__ out, int HW, int G) {
    __shared__ PaSmem S;
    const int b = blockIdx.y;
    stage_pa(S, ca, Wp1, bp1, wp2, bp2, b, G, 256);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (RAGGED && p >= HW) return;                          // behind the parameters' barrier; no other follows
    const size_t img = (size_t)b * 64 * HW;
    float t[64], h[8];
    load_t(t, maps, S, img, HW, p, G);
    const float pg = pixel_gate(t, h, S);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const size_t e = img + ((size_t)o * HW + p) * 8;
        f32x4 lo = {t[o * 8] * pg, t[o * 8 + 1] * pg, t[o * 8 + 2] * pg, t[o * 8 + 3] * pg};
        f32x4 hi = {t[o * 8 + 4] * pg, t[o * 8 + 5] * pg, t[o * 8 + 6] * pg, t[o * 8 + 7] * pg};
        if (res) { lo += ld4v(res + e); hi += ld4v(res + e + 4); }
        st4v(out + e, lo);
        st4v(out + e + 4, hi);
    }
}

// ---- (c) backward a: recompute t, h, pg; dt to memory; the workgroup's partial sums to its slot.  128 pixels per workgroup; a reduction
// round puts one 64-vector per pixel into LDS ([pixel][65]: conflict-free both ways), thread (c = tid & 63, q = tid >> 6) sums the 64
// pixels of wave q for channel c in ascending order, and the two halves are added.  RAGGED: the image's last workgroup may hold fewer than
// 128 pixels; a thread whose pixel is >= HW loads and stores nothing and puts zeros into every LDS row it owns, so the sums keep their order.
struct BwdSmem {
    PaSmem pa;
    float v[BCH][65];
    float d[BCH][17];          // dh[8] | dz relu(h)[8] | dz
    float r[2][64 * 9];
};

template <bool RAGGED>
__global__ __launch_bounds__(BCH) void ffa_gate_pa_bwd_a_kernel(Maps maps, const float* __restrict__ ca, const float* __restrict__ Wp1,
                                                                const float* __restrict__ bp1, const float* __restrict__ wp2,
                                                                const float* __restrict__ bp2, const float* __restrict__ dout,
                                                                float* __restrict__ dt, float* __restrict__ ws, int HW, int G) {
    __shared__ BwdSmem S;
    const int b = blockIdx.y, tid = threadIdx.x, c = tid & 63, q = tid >> 6;
    stage_pa(S.pa, ca, Wp1, bp1, wp2, bp2, b, G, BCH);
    const int p = blockIdx.x * BCH + tid;
    const size_t img = (size_t)b * 64 * HW;
    float* __restrict__ slot = ws + ((size_t)b * gridDim.x + blockIdx.x) * slot_len(G);
    const bool live = !RAGGED || p < HW;
    float t[64], h[8], dh[8], g[64];
    float pg = 0.f, dz = 0.f;
    if (live) {
        load_t(t, maps, S.pa, img, HW, p, G);
        pg = pixel_gate(t, h, S.pa);
        // dpg = sum_c dout_c t_c, with dout read once: it is turned into dt in place below
        float dpg = 0.f;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const size_t e = img + ((size_t)o * HW + p) * 8;
            const f32x4 lo = ld4v(dout + e), hi = ld4v(dout + e + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                g[o * 8 + j] = lo[j]; g[o * 8 + 4 + j] = hi[j];
                dpg = fmaf(lo[j], t[o * 8 + j], dpg);
                dpg = fmaf(hi[j], t[o * 8 + 4 + j], dpg);
            }
        }
        dz = dpg * pg * (1.0f - pg);
    } else {                                                                   // a pixel behind the map: zeros all the way down
#pragma unroll
        for (int cc = 0; cc < 64; ++cc) { t[cc] = 0.f; g[cc] = 0.f; }
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        dh[i] = h[i] > 0.f ? dz * S.pa.w2[i] : 0.f;
        S.d[tid][i] = dh[i];
        S.d[tid][8 + i] = dz * fmaxf(h[i], 0.f);
    }
    S.d[tid][16] = dz;
#pragma unroll
    for (int cc = 0; cc < 64; ++cc) {
        float s = g[cc] * pg;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(S.pa.w1[i][cc], dh[i], s);
        g[cc] = s;                                                            // dt
        S.v[tid][cc] = t[cc];
    }
    if (live) {
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const size_t e = img + ((size_t)o * HW + p) * 8;
            st4v(dt + e, f32x4{g[o * 8], g[o * 8 + 1], g[o * 8 + 2], g[o * 8 + 3]});
            st4v(dt + e + 4, f32x4{g[o * 8 + 4], g[o * 8 + 5], g[o * 8 + 6], g[o * 8 + 7]});
        }
    }
    __syncthreads();
    // round 0: dWp1[i][c] = sum_p dh_i[p] t_c[p]
    {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int pp = 64 * q; pp < 64 * q + 64; ++pp) {
            const float tv = S.v[pp][c];
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = fmaf(S.d[pp][i], tv, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) S.r[q][i * 64 + c] = acc[i];
        if (c < 17) {                                                          // dbp1 | dwp2 | dbp2: column sums of d
            float s = 0.f;
            for (int pp = 64 * q; pp < 64 * q + 64; ++pp) s += S.d[pp][c];
            S.r[q][512 + c] = s;
        }
    }
    __syncthreads();
    for (int i = tid; i < NPA; i += BCH) slot[64 * G + i] = S.r[0][i] + S.r[1][i];
    // rounds 1..G: dca[g][c] = sum_p dt_c[p] m_g[c][p]   (m_g is read a second time: it is in the cache from load_t)
    for (int gi = 0; gi < G; ++gi) {
        __syncthreads();
        const float* __restrict__ m = maps.m[gi] + img;
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};      // g is zero there too
            if (live) { lo = ld4v(m + ((size_t)o * HW + p) * 8); hi = ld4v(m + ((size_t)o * HW + p) * 8 + 4); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                S.v[tid][o * 8 + j] = g[o * 8 + j] * lo[j];
                S.v[tid][o * 8 + 4 + j] = g[o * 8 + 4 + j] * hi[j];
            }
        }
        __syncthreads();
        float s = 0.f;
        for (int pp = 64 * q; pp < 64 * q + 64; ++pp) s += S.v[pp][c];
        S.r[q][c] = s;
        __syncthreads();
        if (tid < 64) slot[gi * 64 + tid] = S.r[0][tid] + S.r[1][tid];
    }
}

// ---- (c) ca_bwd level 1: element e of SEG consecutive slots of one image, ascending.  `used` = 64 G + NPA: the padding floats at the end of a
// slot are never written by backward-a and never read here
__global__ __launch_bounds__(256) void ffa_seg_sum_kernel(const float* __restrict__ slots, float* __restrict__ segs, int nbch, int nseg,
                                                          int slot, int used) {
    const int e = blockIdx.x * 256 + threadIdx.x, sg = blockIdx.y, b = blockIdx.z;
    if (e >= used) return;
    const int c0 = sg * SEG, c1 = min(c0 + SEG, nbch);
    const float* src = slots + ((size_t)b * nbch) * slot + e;
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += src[(size_t)c * slot];
    segs[((size_t)b * nseg + sg) * slot + e] = s;
}

// ---- (c) ca_bwd level 2: one workgroup per image: the segments in ascending order, the gate MLP backwards; dmean is final, the image's
// share of the eight parameter gradients goes to its record [dWa hc n | dba hc | dWb n hc | dbb n | dWp1 512 | dbp1 8 | dwp2 8 | dbp2 1]
__global__ __launch_bounds__(256) void ffa_ca_bwd_image_kernel(const float* __restrict__ segs, const float* __restrict__ Wa,
                                                               const float* __restrict__ Wb, const float* __restrict__ mean,
                                                               const float* __restrict__ hid, const float* __restrict__ ca,
                                                               float* __restrict__ dmean, float* __restrict__ recs, int nseg, int G) {
    __shared__ float sdzb[192];
    __shared__ float sdhid[8], shid[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = 64 * G, hc = G == 1 ? 8 : 4, slot = slot_len(G);
    const float* __restrict__ src = segs + (size_t)b * nseg * slot;
    float* __restrict__ rec = recs + (size_t)b * img_len(G);
    if (tid < n) {
        float s = 0.f;
        for (int sg = 0; sg < nseg; ++sg) s += src[(size_t)sg * slot + tid];
        const float cv = ca[(size_t)b * n + tid];
        sdzb[tid] = s * cv * (1.0f - cv);
    }
    if (tid < hc) shid[tid] = hid[(size_t)b * hc + tid];
    __syncthreads();
    {   // dhid[j] = (sum_k Wb[k][j] dzb[k]) [hid_j > 0]: 32 threads per j, strided partial sums, then a fixed shuffle tree
        const int j = tid >> 5, l = tid & 31;
        float s = 0.f;
        if (j < hc)
            for (int k = l; k < n; k += 32) s = fmaf(Wb[k * hc + j], sdzb[k], s);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (j < hc && l == 0) sdhid[j] = shid[j] > 0.f ? s : 0.f;
    }
    __syncthreads();
    if (tid < n) {
        const float z = sdzb[tid], mv = mean[(size_t)b * n + tid];
        float dm = 0.f;
        for (int j = 0; j < hc; ++j) {
            rec[j * n + tid] = sdhid[j] * mv;                          // dWa
            rec[hc * n + hc + tid * hc + j] = z * shid[j];             // dWb
            dm = fmaf(Wa[j * n + tid], sdhid[j], dm);
        }
        rec[hc * n + hc + n * hc + tid] = z;                           // dbb
        dmean[(size_t)b * n + tid] = dm;
    }
    if (tid < hc) rec[hc * n + tid] = sdhid[tid];                      // dba
    float* __restrict__ pa = rec + 2 * hc * n + hc + n;
    for (int e = tid; e < NPA; e += 256) {
        float s = 0.f;
        for (int sg = 0; sg < nseg; ++sg) s += src[(size_t)sg * slot + n + e];
        pa[e] = s;
    }
}

// ---- (c) ca_bwd level 3: the images' records in ascending order, one owner thread per gradient element
__global__ __launch_bounds__(256) void ffa_ca_bwd_sum_kernel(const float* __restrict__ recs, float* __restrict__ dWa, float* __restrict__ dba,
                                                             float* __restrict__ dWb, float* __restrict__ dbb, float* __restrict__ dWp1,
                                                             float* __restrict__ dbp1, float* __restrict__ dwp2, float* __restrict__ dbp2,
                                                             int B, int G) {
    const int n = 64 * G, hc = G == 1 ? 8 : 4, len = img_len(G);
    const int used = 2 * hc * n + hc + n + NPA;
    int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= used) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += recs[(size_t)b * len + e];
    if (e < hc * n) { dWa[e] = s; return; }
    e -= hc * n;
    if (e < hc) { dba[e] = s; return; }
    e -= hc;
    if (e < n * hc) { dWb[e] = s; return; }
    e -= n * hc;
    if (e < n) { dbb[e] = s; return; }
    e -= n;
    if (e < 512) dWp1[e] = s;
    else if (e < 520) dbp1[e - 512] = s;
    else if (e < 528) dwp2[e - 520] = s;
    else dbp2[0] = s;
}

// ---- (c) backward b: dm_g = ca[b][g][c] dt + dmean[b][g][c] / HW; one float4 per thread
__global__ __launch_bounds__(256) void ffa_gate_pa_bwd_b_kernel(const float* __restrict__ dt, const float* __restrict__ ca,
                                                                const float* __restrict__ dmean, MapsOut dm, int HW, int G, size_t total4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const size_t per_img = (size_t)16 * HW;                 // float4s of one image
    const int b = (int)(i / per_img);
    const size_t r = i % per_img;
    const int o = (int)(r / (2 * (size_t)HW)), c0 = o * 8 + (int)(r & 1) * 4;
    const f32x4 d = ld4v(dt + 4 * i);
    const float inv = 1.0f / (float)HW;
    for (int g = 0; g < G; ++g) {
        const float* cg = ca + ((size_t)b * G + g) * 64 + c0;
        const float* mg = dmean + ((size_t)b * G + g) * 64 + c0;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(cg[j], d[j], mg[j] * inv);
        st4v(dm.m[g] + 4 * i, v);
    }
}

// ---- (d) the two elementwise helpers of a block
__global__ __launch_bounds__(256) void ffa_add_kernel(const float* __restrict__ a, const float* __restrict__ x, float* __restrict__ y,
                                                      size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) st4v(y + 4 * i, ld4v(a + 4 * i) + ld4v(x + 4 * i));
}

// the same for any n: thread i owns floats 4 i .. 4 i + 3; the one that meets the end adds the last n % 4 floats one by one
__global__ __launch_bounds__(256) void ffa_add_any_kernel(const float* __restrict__ a, const float* __restrict__ x, float* __restrict__ y,
                                                          size_t n) {
    const size_t e = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (e + 4 <= n) st4v(y + e, ld4v(a + e) + ld4v(x + e));
    else
        for (size_t k = e; k < n; ++k) y[k] = a[k] + x[k];
}

__global__ __launch_bounds__(256) void ffa_relu_bwd_add_kernel(const float* __restrict__ a1, const float* __restrict__ dr,
                                                               const float* __restrict__ dout, float* __restrict__ dpre1,
                                                               float* __restrict__ s, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 a = ld4v(a1 + 4 * i), d = ld4v(dr + 4 * i);
    f32x4 m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = a[j] > 0.f ? d[j] : 0.f;
    st4v(dpre1 + 4 * i, m);
    st4v(s + 4 * i, ld4v(dout + 4 * i) + d);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define FFA_SHAPE(who)                                                                                                                 \
    DHZ_REQUIRE(B >= 1, "%s: B=%d (at least 1)", who, B);                                                                              \
    if (any) DHZ_REQUIRE(H >= 1 && W >= 1, "%s: H=%d W=%d (at least 1)", who, H, W);                                                   \
    else DHZ_REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0, "%s: H=%d W=%d (multiples of 16)", who, H, W);                  \
    DHZ_REQUIRE(G == 1 || G == 3, "%s: G=%d (1 or 3)", who, G);                                                                        \
    const Cut c = make_cut(B, H, W, G, any);                                                                                           \
    DHZ_REQUIRE(c.ok, "%s: map of H=%d W=%d too large (64 H W must stay below 2^31)", who, H, W)

#define FFA_MAPS(who, a0, a1, a2)                                                                                                      \
    DHZ_REQUIRE(a0 && (G == 1 || (a1 && a2)), "%s: null map pointer (G=%d: %p %p %p)", who, G, (const void*)a0, (const void*)a1,       \
                (const void*)a2);                                                                                                      \
    DHZ_REQUIRE(aligned16(a0) && (G == 1 || (aligned16(a1) && aligned16(a2))), "%s: maps must be 16-byte aligned (%p %p %p)", who,     \
                (const void*)a0, (const void*)a1, (const void*)a2)

// the caller's workspace, or the deterministic mode's
#define FFA_WS(who, floats)                                                                                                            \
    do {                                                                                                                               \
        const size_t need_ = (floats) * sizeof(float);                                                                                 \
        if (dhz_det()) {                                                                                                               \
            ws = dhz_det_ws(who, 1, (long)(floats));                                                                                   \
            if (!ws) return DHZ_EINVAL;                                                                                                \
        } else {                                                                                                                       \
            DHZ_REQUIRE(ws, "%s: null workspace (%zu bytes needed: dhz_ffa_workspace_bytes%s)", who, need_, any ? "_any" : "");        \
            DHZ_REQUIRE(aligned16(ws), "%s: workspace %p must be 16-byte aligned", who, (void*)ws);                                    \
            DHZ_REQUIRE(ws_bytes >= need_, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need_);                            \
        }                                                                                                                              \
    } while (0)

size_t workspace_bytes(int B, int H, int W, int G, bool any) {
    const Cut c = make_cut(B, H, W, G, any);
    if (!c.ok) return 0;
    return (c.bwd_floats > c.fwd_floats ? c.bwd_floats : c.fwd_floats) * sizeof(float);
}

int ca_fwd(const char* who, bool any, const float* m0, const float* m1, const float* m2, const float* Wa, const float* ba, const float* Wb,
                              const float* bb, float* mean, float* hid, float* ca, float* ws, size_t ws_bytes, int B, int H, int W, int G,
                              void* stream) {
    FFA_SHAPE(who);
    FFA_MAPS(who, m0, m1, m2);
    DHZ_REQUIRE(Wa && ba && Wb && bb && mean && hid && ca, "%s: null pointer (Wa=%p ba=%p Wb=%p bb=%p mean=%p hid=%p ca=%p)", who,
                (const void*)Wa, (const void*)ba, (const void*)Wb, (const void*)bb, (void*)mean, (void*)hid, (void*)ca);
    FFA_WS(who, c.fwd_floats);
    hipStream_t s = (hipStream_t)stream;
    const Maps maps{{m0, m1, m2}};
    hipLaunchKernelGGL(ffa_pool_kernel, dim3(c.npch, G, B), dim3(256), 0, s, maps, ws, (int)c.HW, c.npch, G);
    DHZ_CHECK_LAUNCH(any ? "dhz_ffa_ca_fwd_any (pooling)" : "dhz_ffa_ca_fwd (pooling)");
    hipLaunchKernelGGL(ffa_ca_mlp_kernel, dim3(B), dim3(256), 0, s, ws, Wa, ba, Wb, bb, mean, hid, ca, (int)c.HW, c.npch, G);
    DHZ_CHECK_LAUNCH(any ? "dhz_ffa_ca_fwd_any (gate)" : "dhz_ffa_ca_fwd (gate)");
    return DHZ_OK;
}

int gate_pa_fwd(const char* who, bool any, const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1, const float* bp1,
                                   const float* wp2, const float* bp2, const float* res, float* out, int B, int H, int W, int G,
                                   void* stream) {
    FFA_SHAPE(who);
    FFA_MAPS(who, m0, m1, m2);
    DHZ_REQUIRE(ca && Wp1 && bp1 && wp2 && bp2 && out, "%s: null pointer (ca=%p Wp1=%p bp1=%p wp2=%p bp2=%p out=%p)", who, (const void*)ca,
                (const void*)Wp1, (const void*)bp1, (const void*)wp2, (const void*)bp2, (void*)out);
    DHZ_REQUIRE(aligned16(out) && aligned16(res), "%s: out=%p / res=%p must be 16-byte aligned", who, (void*)out, (const void*)res);
    const Maps maps{{m0, m1, m2}};
    const dim3 grid((unsigned)((c.HW + 255) / 256), B);
    if (c.ragged)
        hipLaunchKernelGGL(ffa_gate_pa_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, maps, ca, Wp1, bp1, wp2, bp2, res, out,
                           (int)c.HW, G);
    else
        hipLaunchKernelGGL(ffa_gate_pa_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, maps, ca, Wp1, bp1, wp2, bp2, res, out,
                           (int)c.HW, G);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

int gate_pa_bwd_a(const char* who, bool any, const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1,
                                     const float* bp1, const float* wp2, const float* bp2, const float* dout, float* dt, float* ws,
                                     size_t ws_bytes, int B, int H, int W, int G, void* stream) {
    FFA_SHAPE(who);
    FFA_MAPS(who, m0, m1, m2);
    DHZ_REQUIRE(ca && Wp1 && bp1 && wp2 && bp2 && dout && dt, "%s: null pointer (ca=%p Wp1=%p bp1=%p wp2=%p bp2=%p dout=%p dt=%p)", who,
                (const void*)ca, (const void*)Wp1, (const void*)bp1, (const void*)wp2, (const void*)bp2, (const void*)dout, (void*)dt);
    DHZ_REQUIRE(aligned16(dout) && aligned16(dt), "%s: dout=%p / dt=%p must be 16-byte aligned", who, (const void*)dout, (void*)dt);
    FFA_WS(who, c.bwd_floats);
    const Maps maps{{m0, m1, m2}};
    if (c.HW % BCH)
        hipLaunchKernelGGL(ffa_gate_pa_bwd_a_kernel<true>, dim3(c.nbch, B), dim3(BCH), 0, (hipStream_t)stream, maps, ca, Wp1, bp1, wp2, bp2,
                           dout, dt, ws, (int)c.HW, G);
    else
        hipLaunchKernelGGL(ffa_gate_pa_bwd_a_kernel<false>, dim3(c.nbch, B), dim3(BCH), 0, (hipStream_t)stream, maps, ca, Wp1, bp1, wp2, bp2,
                           dout, dt, ws, (int)c.HW, G);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

int ca_bwd(const char* who, bool any, float* ws, size_t ws_bytes, const float* Wa, const float* Wb, const float* mean, const float* hid,
                              const float* ca, float* dWa, float* dba, float* dWb, float* dbb, float* dmean, float* dWp1, float* dbp1,
                              float* dwp2, float* dbp2, int B, int H, int W, int G, void* stream) {
    FFA_SHAPE(who);
    DHZ_REQUIRE(Wa && Wb && mean && hid && ca, "%s: null pointer (Wa=%p Wb=%p mean=%p hid=%p ca=%p)", who, (const void*)Wa, (const void*)Wb,
                (const void*)mean, (const void*)hid, (const void*)ca);
    DHZ_REQUIRE(dWa && dba && dWb && dbb && dmean && dWp1 && dbp1 && dwp2 && dbp2,
                "%s: null gradient pointer (dWa=%p dba=%p dWb=%p dbb=%p dmean=%p dWp1=%p dbp1=%p dwp2=%p dbp2=%p)", who, (void*)dWa,
                (void*)dba, (void*)dWb, (void*)dbb, (void*)dmean, (void*)dWp1, (void*)dbp1, (void*)dwp2, (void*)dbp2);
    FFA_WS(who, c.bwd_floats);
    hipStream_t s = (hipStream_t)stream;
    float* segs = ws + c.bwd_a_floats;
    hipLaunchKernelGGL(ffa_seg_sum_kernel, dim3((c.slot + 255) / 256, c.nseg, B), dim3(256), 0, s, ws, segs, c.nbch, c.nseg, c.slot,
                       64 * G + NPA);
    DHZ_CHECK_LAUNCH(any ? "dhz_ffa_ca_bwd_any (segments)" : "dhz_ffa_ca_bwd (segments)");
    float* recs = segs + c.seg_floats;
    hipLaunchKernelGGL(ffa_ca_bwd_image_kernel, dim3(B), dim3(256), 0, s, segs, Wa, Wb, mean, hid, ca, dmean, recs, c.nseg, G);
    DHZ_CHECK_LAUNCH(any ? "dhz_ffa_ca_bwd_any (images)" : "dhz_ffa_ca_bwd (images)");
    hipLaunchKernelGGL(ffa_ca_bwd_sum_kernel, dim3((img_len(G) + 255) / 256), dim3(256), 0, s, recs, dWa, dba, dWb, dbb, dWp1, dbp1, dwp2,
                       dbp2, B, G);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

int gate_pa_bwd_b(const char* who, bool any, const float* dt, const float* ca, const float* dmean, float* dm0, float* dm1, float* dm2, int B, int H,
                                     int W, int G, void* stream) {
    FFA_SHAPE(who);
    FFA_MAPS(who, dm0, dm1, dm2);
    DHZ_REQUIRE(dt && ca && dmean, "%s: null pointer (dt=%p ca=%p dmean=%p)", who, (const void*)dt, (const void*)ca, (const void*)dmean);
    DHZ_REQUIRE(aligned16(dt) && aligned16(ca) && aligned16(dmean), "%s: dt=%p / ca=%p / dmean=%p must be 16-byte aligned", who,
                (const void*)dt, (const void*)ca, (const void*)dmean);
    const size_t total4 = (size_t)B * 16 * c.HW;
    const MapsOut dm{{dm0, dm1, dm2}};
    hipLaunchKernelGGL(ffa_gate_pa_bwd_b_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dt, ca, dmean,
                       dm, (int)c.HW, G, total4);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

}  // namespace

// every entry twice: multiples of 16 only, and (`_any`) any H, W >= 1 on the same launch code
extern "C" size_t dhz_ffa_workspace_bytes(int B, int H, int W, int G) { return workspace_bytes(B, H, W, G, false); }
extern "C" size_t dhz_ffa_workspace_bytes_any(int B, int H, int W, int G) { return workspace_bytes(B, H, W, G, true); }

#define FFA_CA_FWD_ARGS                                                                                                                \
    const float *m0, const float *m1, const float *m2, const float *Wa, const float *ba, const float *Wb, const float *bb, float *mean, \
        float *hid, float *ca, float *ws, size_t ws_bytes, int B, int H, int W, int G, void *stream
extern "C" int dhz_ffa_ca_fwd(FFA_CA_FWD_ARGS) {
    return ca_fwd("dhz_ffa_ca_fwd", false, m0, m1, m2, Wa, ba, Wb, bb, mean, hid, ca, ws, ws_bytes, B, H, W, G, stream);
}
extern "C" int dhz_ffa_ca_fwd_any(FFA_CA_FWD_ARGS) {
    return ca_fwd("dhz_ffa_ca_fwd_any", true, m0, m1, m2, Wa, ba, Wb, bb, mean, hid, ca, ws, ws_bytes, B, H, W, G, stream);
}
#undef FFA_CA_FWD_ARGS

#define FFA_GATE_FWD_ARGS                                                                                                              \
    const float *m0, const float *m1, const float *m2, const float *ca, const float *Wp1, const float *bp1, const float *wp2,           \
        const float *bp2, const float *res, float *out, int B, int H, int W, int G, void *stream
extern "C" int dhz_ffa_gate_pa_fwd(FFA_GATE_FWD_ARGS) {
    return gate_pa_fwd("dhz_ffa_gate_pa_fwd", false, m0, m1, m2, ca, Wp1, bp1, wp2, bp2, res, out, B, H, W, G, stream);
}
extern "C" int dhz_ffa_gate_pa_fwd_any(FFA_GATE_FWD_ARGS) {
    return gate_pa_fwd("dhz_ffa_gate_pa_fwd_any", true, m0, m1, m2, ca, Wp1, bp1, wp2, bp2, res, out, B, H, W, G, stream);
}
#undef FFA_GATE_FWD_ARGS

#define FFA_BWD_A_ARGS                                                                                                                 \
    const float *m0, const float *m1, const float *m2, const float *ca, const float *Wp1, const float *bp1, const float *wp2,           \
        const float *bp2, const float *dout, float *dt, float *ws, size_t ws_bytes, int B, int H, int W, int G, void *stream
extern "C" int dhz_ffa_gate_pa_bwd_a(FFA_BWD_A_ARGS) {
    return gate_pa_bwd_a("dhz_ffa_gate_pa_bwd_a", false, m0, m1, m2, ca, Wp1, bp1, wp2, bp2, dout, dt, ws, ws_bytes, B, H, W, G, stream);
}
extern "C" int dhz_ffa_gate_pa_bwd_a_any(FFA_BWD_A_ARGS) {
    return gate_pa_bwd_a("dhz_ffa_gate_pa_bwd_a_any", true, m0, m1, m2, ca, Wp1, bp1, wp2, bp2, dout, dt, ws, ws_bytes, B, H, W, G, stream);
}
#undef FFA_BWD_A_ARGS

#define FFA_CA_BWD_ARGS                                                                                                                \
    float *ws, size_t ws_bytes, const float *Wa, const float *Wb, const float *mean, const float *hid, const float *ca, float *dWa,    \
        float *dba, float *dWb, float *dbb, float *dmean, float *dWp1, float *dbp1, float *dwp2, float *dbp2, int B, int H, int W,     \
        int G, void *stream
extern "C" int dhz_ffa_ca_bwd(FFA_CA_BWD_ARGS) {
    return ca_bwd("dhz_ffa_ca_bwd", false, ws, ws_bytes, Wa, Wb, mean, hid, ca, dWa, dba, dWb, dbb, dmean, dWp1, dbp1, dwp2, dbp2, B, H, W, G,
                  stream);
}
extern "C" int dhz_ffa_ca_bwd_any(FFA_CA_BWD_ARGS) {
    return ca_bwd("dhz_ffa_ca_bwd_any", true, ws, ws_bytes, Wa, Wb, mean, hid, ca, dWa, dba, dWb, dbb, dmean, dWp1, dbp1, dwp2, dbp2, B, H, W,
                  G, stream);
}
#undef FFA_CA_BWD_ARGS

#define FFA_BWD_B_ARGS                                                                                                                 \
    const float *dt, const float *ca, const float *dmean, float *dm0, float *dm1, float *dm2, int B, int H, int W, int G, void *stream
extern "C" int dhz_ffa_gate_pa_bwd_b(FFA_BWD_B_ARGS) {
    return gate_pa_bwd_b("dhz_ffa_gate_pa_bwd_b", false, dt, ca, dmean, dm0, dm1, dm2, B, H, W, G, stream);
}
extern "C" int dhz_ffa_gate_pa_bwd_b_any(FFA_BWD_B_ARGS) {
    return gate_pa_bwd_b("dhz_ffa_gate_pa_bwd_b_any", true, dt, ca, dmean, dm0, dm1, dm2, B, H, W, G, stream);
}
#undef FFA_BWD_B_ARGS

extern "C" int dhz_ffa_add(const float* a, const float* x, float* y, int64_t n, void* stream) {
    DHZ_REQUIRE(a && x && y, "dhz_ffa_add: null pointer (a=%p x=%p y=%p)", (const void*)a, (const void*)x, (void*)y);
    DHZ_REQUIRE(n > 0 && n % 4 == 0, "dhz_ffa_add: n=%lld (a positive multiple of 4)", (long long)n);
    DHZ_REQUIRE(aligned16(a) && aligned16(x) && aligned16(y), "dhz_ffa_add: pointers must be 16-byte aligned (a=%p x=%p y=%p)",
                (const void*)a, (const void*)x, (void*)y);
    const size_t n4 = (size_t)n / 4;
    hipLaunchKernelGGL(ffa_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, x, y, n4);
    DHZ_CHECK_LAUNCH("dhz_ffa_add");
    return DHZ_OK;
}

extern "C" int dhz_ffa_add_any(const float* a, const float* x, float* y, int64_t n, void* stream) {
    DHZ_REQUIRE(a && x && y, "dhz_ffa_add_any: null pointer (a=%p x=%p y=%p)", (const void*)a, (const void*)x, (void*)y);
    DHZ_REQUIRE(n > 0, "dhz_ffa_add_any: n=%lld (positive)", (long long)n);
    DHZ_REQUIRE(aligned16(a) && aligned16(x) && aligned16(y), "dhz_ffa_add_any: pointers must be 16-byte aligned (a=%p x=%p y=%p)",
                (const void*)a, (const void*)x, (void*)y);
    const size_t n4 = ((size_t)n + 3) / 4;
    hipLaunchKernelGGL(ffa_add_any_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, x, y, (size_t)n);
    DHZ_CHECK_LAUNCH("dhz_ffa_add_any");
    return DHZ_OK;
}

extern "C" int dhz_ffa_relu_bwd_add(const float* a1, const float* dr, const float* dout, float* dpre1, float* s, int64_t n, void* stream) {
    DHZ_REQUIRE(a1 && dr && dout && dpre1 && s, "dhz_ffa_relu_bwd_add: null pointer (a1=%p dr=%p dout=%p dpre1=%p s=%p)", (const void*)a1,
                (const void*)dr, (const void*)dout, (void*)dpre1, (void*)s);
    DHZ_REQUIRE(n > 0 && n % 4 == 0, "dhz_ffa_relu_bwd_add: n=%lld (a positive multiple of 4)", (long long)n);
    DHZ_REQUIRE(aligned16(a1) && aligned16(dr) && aligned16(dout) && aligned16(dpre1) && aligned16(s),
                "dhz_ffa_relu_bwd_add: pointers must be 16-byte aligned (a1=%p dr=%p dout=%p dpre1=%p s=%p)", (const void*)a1,
                (const void*)dr, (const void*)dout, (void*)dpre1, (void*)s);
    const size_t n4 = (size_t)n / 4;
    hipLaunchKernelGGL(ffa_relu_bwd_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a1, dr, dout, dpre1,
                       s, n4);
    DHZ_CHECK_LAUNCH("dhz_ffa_relu_bwd_add");
    return DHZ_OK;
}
