// K3 for 4 x 4 windows (16 tokens): the ProbSparse window-attention core (ATT:287-342), forward and backward, its dense twin
// (M0:428-492), and the window-parametrised (`_w`) entry points of the attention-side helpers (shift mask, bias gather, table gradient).
//
// A 16-token window-head is ONE 16 x 16 score tile, so one wave64 owns a window-head from its loads to its stores and a 256-thread
// workgroup runs four independent window-heads.  The waves of a workgroup share no data: every phase boundary is a wave-level
// ordering point (dhz_wave_sync), there is no workgroup barrier in this file, and waves without work simply leave.
// Persistent grid: wave gw = 4 blockIdx.x + w walks window-heads gw, gw + 4 gridDim.x, ...; the Q, K, V (and dO) rows of the next
// window-head are fetched into registers while the current one computes, as in ps_attn.hip.
//
// Contractions on v_mfma_f32_16x16x4_f32 (lane l: a = A[l & 15][l >> 4], b = B[l >> 4][l & 15], acc[j] = D[4 (l >> 4) + j][l & 15]):
//   S = Q K^T    one accumulator tile in d / 4 steps; the 15 sampled scores of a query are read out of S in LDS
//   O = P V      ALL 16 rows of P: the row of the one unselected query holds the constant 1/16, so its row of O is mean(V)
//                (ATT:168-172) - no compaction by rank, no padding, no scatter
// u = n_top(16) = 15 of 16 queries are selected.  bf16 storage: the staged fp32 values are the bf16 values; same fp32 products.
// No float atomic anywhere: a wave keeps the 16 x 16 bias-gradient sum of its window-heads in 4 registers per lane and stores it
// as its own partial; the table gradient is a fixed-order sum.  Deterministic mode needs no separate path.
#include "bf16_pipe.h"

namespace {

constexpr int NT = 16;     // tokens per window
constexpr int NU = 15;     // selected queries / sampled keys per query: n_top(16)
constexpr int SS = 20;     // row stride of the 16-wide score tiles (float4-aligned rows)

#ifndef PS16_FWD_WG
#define PS16_FWD_WG(d) ((d) == 64 ? 2 : 4)      // resident workgroups per CU, forward (LDS: 57.6 KB at d = 64, 33.1 KB at d = 32)
#endif
#ifndef PS16_BWD_WG
#define PS16_BWD_WG(d) ((d) == 64 ? 1 : 2)      // backward (79.9 KB at d = 64, 47.1 KB at d = 32)
#endif

__device__ __forceinline__ float q4_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    return fmaxf(v, __shfl_xor(v, 2));
}
__device__ __forceinline__ float q4_sum(float v) {
    v += __shfl_xor(v, 1);
    return v + __shfl_xor(v, 2);
}
// softmax of a 16-wide row held as 4 columns in each of 4 neighbouring lanes (v_exp_f32 / v_rcp_f32 as in ps_attn.hip)
__device__ __forceinline__ void softmax4(const float* x, float* p) {
    const float mx = q4_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    float e[4], sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { e[i] = __expf(x[i] - mx); sum += e[i]; }
    sum = __builtin_amdgcn_rcpf(q4_sum(sum));
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = e[i] * sum;
}
// the probabilities of row r, columns c0 .. c0 + 3, from the scaled scores x.  Every lane runs the shuffles (no divergence around them).
//   ProbSparse: p1 = softmax(x); p2 = softmax(p1 + bias + mask)  (ATT:195, 229, 251-258, 262); unselected row: p1 = 0, p2 = 1/16
//   dense:      p2 = softmax(x + bias + mask)  (M0:470-488); p1 is not used
// PAD: the padding word pw of the window (low 16 bits; bit j: token j is padding) adds -100 where query r AND key c0 + i are padding - summed
// with the shift-mask row first (exact), that sum added where the mask is added: the bits of a materialised shift + padding mask tensor
template <bool DENSE, bool PAD = false>
__device__ __forceinline__ void probs16(const float* x, const float* brow, const float* mrow, bool sel, float* p1, float* p2,
                                        uint64_t pw = 0, int r = 0, int c0 = 0) {
    float a[4];
    if (DENSE) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = x[i]; p1[i] = 0.f; }
    } else {
        softmax4(x, p1);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = p1[i];
    }
    if (brow) { const float4 b = *reinterpret_cast<const float4*>(brow); a[0] += b.x; a[1] += b.y; a[2] += b.z; a[3] += b.w; }
    if (PAD && pw != 0) {                                  // wave-uniform: one window per wave
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        if (mrow) { const float4 b = *reinterpret_cast<const float4*>(mrow); m[0] = b.x; m[1] = b.y; m[2] = b.z; m[3] = b.w; }
        const float pq = ((pw >> r) & 1ull) ? -100.0f : 0.f;
        const uint32_t kb = (uint32_t)((pw >> c0) & 0xfull);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += m[i] + (((kb >> i) & 1u) ? pq : 0.f);
    } else if (mrow) { const float4 b = *reinterpret_cast<const float4*>(mrow); a[0] += b.x; a[1] += b.y; a[2] += b.z; a[3] += b.w; }
    softmax4(a, p2);
    if (!DENSE && !sel) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { p1[i] = 0.f; p2[i] = 1.0f / NT; }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int D>
struct Fwd16 {
    static constexpr int DS = D + 4;
    float q[NT * DS];      // Q, later O
    float k[NT * DS];
    float v[NT * DS];
    float s[NT * SS];      // S -> P
    float m[NT];
    uint8_t rank[NT];
};

// PAD: the last argument carries the padding words (PadArg, common.h): pad.words[b] of the GLOBAL window b; the shift mask keeps b % nW.
template <int D, typename T, bool DENSE, bool PAD = false>
__global__ __launch_bounds__(256) void attn16_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                         int ld, const uint8_t* __restrict__ idx, const float* __restrict__ bias,
                                                         const float* __restrict__ mask, T* __restrict__ out, int ldo,
                                                         uint8_t* __restrict__ rank_out, int H, int nW, int nwh, float scale,
                                                         PadArg<PAD> pad) {
    constexpr int DS = D + 4, F = D / 4, NR = D / 16;      // float4 per row; staged float4 per lane and tensor
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    Fwd16<D>& sm = reinterpret_cast<Fwd16<D>*>(smem_raw)[w];
    const int i = lane & 15, g = lane >> 4;
    const int stride = gridDim.x * 4;
    int wh = blockIdx.x * 4 + w;
    if (wh >= nwh) return;                                 // an idle wave: nobody waits for it

    // the sampled keys of query lane >> 2 that this lane reads (samples lane & 3, + 4, ...): the same for every window-head
    int sidx[4];
    if (!DENSE) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int s = (lane & 3) + 4 * t;
            sidx[t] = s < NU ? (idx[(lane >> 2) * NU + s] & (NT - 1)) : -1;
        }
    }
    f32x4 pq[NR], pk[NR], pv[NR];
    auto prefetch = [&](int wh_) {
        const size_t tk0 = (size_t)(wh_ / H) * NT;
        const int hh = wh_ % H;
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane;
            const size_t gi = (tk0 + e / F) * ld + hh * D + (e % F) * 4;
            pq[p] = ld4v(q + gi);
            pk[p] = ld4v(k + gi);
            pv[p] = ld4v(v + gi);
        }
    };
    prefetch(wh);
#pragma unroll 1
    for (; wh < nwh; wh += stride) {
        const int b = wh / H, h = wh % H;
        const size_t tok0 = (size_t)b * NT;
        uint64_t pw = 0;
        if constexpr (PAD) pw = pad.words[b] & 0xffffull;
        dhz_wave_sync();                                       // the previous window-head's stores have read O / rank
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane, o = (e / F) * DS + (e % F) * 4;
            *reinterpret_cast<f32x4*>(&sm.q[o]) = pq[p];
            *reinterpret_cast<f32x4*>(&sm.k[o]) = pk[p];
            *reinterpret_cast<f32x4*>(&sm.v[o]) = pv[p];
        }
        if (wh + stride < nwh) prefetch(wh + stride);      // in flight during the rest of this window-head
        dhz_wave_sync();

        // ---- S = Q K^T
        {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = mfma16(sm.q[i * DS + 4 * s + g], sm.k[i * DS + 4 * s + g], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) sm.s[(4 * g + j) * SS + i] = acc[j];
        }
        dhz_wave_sync();

        if (!DENSE) {
            // ---- sparsity measure M[q] = max_s S[q, idx[q, s]] - sum_s S[q, idx[q, s]] / 16      (ATT:117), 4 lanes per query
            {
                const int qi = lane >> 2;
                float mx = -INFINITY, su = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (sidx[t] >= 0) {
                        const float val = sm.s[qi * SS + sidx[t]];
                        mx = fmaxf(mx, val);
                        su += val;
                    }
                }
                mx = q4_max(mx);
                su = q4_sum(su);
                if ((lane & 3) == 0) sm.m[qi] = mx - su * (1.0f / NT);
            }
            dhz_wave_sync();
            // ---- rank[q] = #{j : M[j] > M[q] or (M[j] == M[q] and j < q)}; the 15 lowest ranks are selected      (ATT:122)
            {
                const float m = sm.m[i];
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const float mj = sm.m[j];
                    cnt += (mj > m) || (mj == m && j < i);
                }
                if (lane < NT) sm.rank[lane] = cnt < NU ? (uint8_t)cnt : (uint8_t)255;
            }
            dhz_wave_sync();
        }

        // ---- P in place over S: lane = (row r, columns c0 .. c0 + 3)
        {
            const int r = lane >> 2, c0 = (lane & 3) * 4;
            const float4 s4 = *reinterpret_cast<const float4*>(&sm.s[r * SS + c0]);
            const float x[4] = {s4.x * scale, s4.y * scale, s4.z * scale, s4.w * scale};
            const float* brow = bias ? bias + ((size_t)h * NT + r) * NT + c0 : nullptr;
            const float* mrow = mask ? mask + ((size_t)(b % nW) * NT + r) * NT + c0 : nullptr;
            float p1[4], p2[4];
            probs16<DENSE, PAD>(x, brow, mrow, DENSE || sm.rank[r] != 255, p1, p2, pw, r, c0);
            *reinterpret_cast<float4*>(&sm.s[r * SS + c0]) = make_float4(p2[0], p2[1], p2[2], p2[3]);
        }
        dhz_wave_sync();

        // ---- O = P V over the dead Q tile
#pragma unroll
        for (int tc = 0; tc < D / 16; ++tc) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16(sm.s[i * SS + 4 * s + g], sm.v[(4 * s + g) * DS + 16 * tc + i], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) sm.q[(4 * g + j) * DS + 16 * tc + i] = acc[j];
        }
        dhz_wave_sync();
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane, row = e / F, c4 = e % F;
            st4(out + (tok0 + row) * ldo + h * D + c4 * 4, *reinterpret_cast<const float4*>(&sm.q[row * DS + c4 * 4]));
        }
        if (!DENSE && lane < NT / 4)
            reinterpret_cast<uint32_t*>(rank_out + (size_t)wh * NT)[lane] = reinterpret_cast<const uint32_t*>(sm.rank)[lane];
    }
}

// ------------------------------------------------------------------------------------------------ backward
template <int D>
struct Bwd16 {
    static constexpr int DS = D + 4;
    float q[NT * DS];      // Q ; later dQ
    float k[NT * DS];      // K ; later dK
    float v[NT * DS];      // V ; later dV
    float g[NT * DS];      // dO
    float s[NT * SS];      // S -> dP2 -> dS
    float p[NT * SS];      // P2
    uint8_t rank[NT];
};

// wave gw (< parts) owns head gw % H and the windows gw / H, + parts / H, ...; it stores the bias-gradient sum of its window-heads at
// dbias_part[gw] (4 registers per lane: row lane >> 2, columns 4 (lane & 3) ..)
// (PAD as in the forward; the padding term only enters the recomputation of P: no gradient flows to it)
template <int D, typename T, bool DENSE, bool HAS_BIAS, bool PAD = false>
__global__ __launch_bounds__(256) void attn16_bwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                         int ld, const float* __restrict__ bias, const float* __restrict__ mask,
                                                         const uint8_t* __restrict__ rank_in, const T* __restrict__ dout, int ldo,
                                                         T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dv, int ldg,
                                                         float* __restrict__ dbias_part, int B_, int H, int nW, int parts,
                                                         float scale, PadArg<PAD> pad) {
    constexpr int DS = D + 4, F = D / 4, NR = D / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    Bwd16<D>& sm = reinterpret_cast<Bwd16<D>*>(smem_raw)[w];
    const int i = lane & 15, g = lane >> 4;
    const int gw = blockIdx.x * 4 + w;
    if (gw >= parts) return;
    const int h = gw % H, bstep = parts / H;
    float accb[4] = {0.f, 0.f, 0.f, 0.f};

    f32x4 pq[NR], pk[NR], pv[NR], pg[NR];
    uint8_t prank = 0;
    auto prefetch = [&](int b) {
        const size_t tok0 = (size_t)b * NT;
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane;
            const size_t gi = (tok0 + e / F) * ld + h * D + (e % F) * 4;
            pq[p] = ld4v(q + gi);
            pk[p] = ld4v(k + gi);
            pv[p] = ld4v(v + gi);
            pg[p] = ld4v(dout + (tok0 + e / F) * ldo + h * D + (e % F) * 4);
        }
        if (!DENSE && lane < NT) prank = rank_in[((size_t)b * H + h) * NT + lane];
    };
    int b = gw / H;
    if (b < B_) prefetch(b);
#pragma unroll 1
    for (; b < B_; b += bstep) {
        const size_t tok0 = (size_t)b * NT;
        uint64_t pw = 0;
        if constexpr (PAD) pw = pad.words[b] & 0xffffull;
        dhz_wave_sync();                                       // the previous window-head's stores have read the staging tiles
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane, o = (e / F) * DS + (e % F) * 4;
            *reinterpret_cast<f32x4*>(&sm.q[o]) = pq[p];
            *reinterpret_cast<f32x4*>(&sm.k[o]) = pk[p];
            *reinterpret_cast<f32x4*>(&sm.v[o]) = pv[p];
            *reinterpret_cast<f32x4*>(&sm.g[o]) = pg[p];
        }
        if (!DENSE && lane < NT) sm.rank[lane] = prank;
        if (b + bstep < B_) prefetch(b + bstep);
        dhz_wave_sync();

        // ---- recompute S = Q K^T
        {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = mfma16(sm.q[i * DS + 4 * s + g], sm.k[i * DS + 4 * s + g], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) sm.s[(4 * g + j) * SS + i] = acc[j];
        }
        dhz_wave_sync();

        // ---- P1 (stays in registers: the same lane runs the softmax backward of these elements), P2 -> LDS
        const int r = lane >> 2, c0 = (lane & 3) * 4;
        const bool sel = DENSE || sm.rank[r] != 255;
        float p1[4], p2[4];
        {
            const float4 s4 = *reinterpret_cast<const float4*>(&sm.s[r * SS + c0]);
            const float x[4] = {s4.x * scale, s4.y * scale, s4.z * scale, s4.w * scale};
            const float* brow = bias ? bias + ((size_t)h * NT + r) * NT + c0 : nullptr;
            const float* mrow = mask ? mask + ((size_t)(b % nW) * NT + r) * NT + c0 : nullptr;
            probs16<DENSE, PAD>(x, brow, mrow, sel, p1, p2, pw, r, c0);
            *reinterpret_cast<float4*>(&sm.p[r * SS + c0]) = make_float4(p2[0], p2[1], p2[2], p2[3]);
        }
        dhz_wave_sync();

        // ---- dP2 = dO V^T (over S);  dV = P2^T dO (the 1/16 row of P2 carries the mean(V) path)
        f32x4 accv[D / 16];
        {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < D / 4; ++s) acc = mfma16(sm.g[i * DS + 4 * s + g], sm.v[i * DS + 4 * s + g], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) sm.s[(4 * g + j) * SS + i] = acc[j];
#pragma unroll
            for (int tc = 0; tc < D / 16; ++tc) {
                accv[tc] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s)      // A(n, r) = P2[r][n] ; B(r, e) = dO[r][16 tc + e]
                    accv[tc] = mfma16(sm.p[(4 * s + g) * SS + i], sm.g[(4 * s + g) * DS + 16 * tc + i], accv[tc]);
            }
        }
        dhz_wave_sync();                                       // V is dead: its tile takes dV

        // ---- both softmax backward steps; the bias gradient is dA
        {
#pragma unroll
            for (int tc = 0; tc < D / 16; ++tc)
#pragma unroll
                for (int j = 0; j < 4; ++j) sm.v[(4 * g + j) * DS + 16 * tc + i] = accv[tc][j];
            const float4 d4 = *reinterpret_cast<const float4*>(&sm.s[r * SS + c0]);
            const float dp[4] = {d4.x, d4.y, d4.z, d4.w};
            float dot2 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) dot2 += dp[e] * p2[e];
            dot2 = q4_sum(dot2);
            float da[4], ds[4], dot1 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) { da[e] = sel ? p2[e] * (dp[e] - dot2) : 0.f; dot1 += da[e] * p1[e]; }
            dot1 = q4_sum(dot1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ds[e] = DENSE ? da[e] * scale : p1[e] * (da[e] - dot1) * scale;
                if (HAS_BIAS) accb[e] += da[e];
            }
            *reinterpret_cast<float4*>(&sm.s[r * SS + c0]) = make_float4(ds[0], ds[1], ds[2], ds[3]);
        }
        dhz_wave_sync();

        // ---- dQ = dS K ; dK = dS^T Q
        f32x4 accq[D / 16], acck[D / 16];
#pragma unroll
        for (int tc = 0; tc < D / 16; ++tc) {
            accq[tc] = f32x4{0.f, 0.f, 0.f, 0.f};
            acck[tc] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                accq[tc] = mfma16(sm.s[i * SS + 4 * s + g], sm.k[(4 * s + g) * DS + 16 * tc + i], accq[tc]);
                acck[tc] = mfma16(sm.s[(4 * s + g) * SS + i], sm.q[(4 * s + g) * DS + 16 * tc + i], acck[tc]);
            }
        }
        dhz_wave_sync();                                       // all reads of Q / K done
#pragma unroll
        for (int tc = 0; tc < D / 16; ++tc)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sm.q[(4 * g + j) * DS + 16 * tc + i] = accq[tc][j];
                sm.k[(4 * g + j) * DS + 16 * tc + i] = acck[tc][j];
            }
        dhz_wave_sync();
#pragma unroll
        for (int p = 0; p < NR; ++p) {
            const int e = p * 64 + lane, row = e / F, c4 = e % F;
            const size_t go = (tok0 + row) * ldg + h * D + c4 * 4;
            st4(dq + go, *reinterpret_cast<const float4*>(&sm.q[row * DS + c4 * 4]));
            st4(dk + go, *reinterpret_cast<const float4*>(&sm.k[row * DS + c4 * 4]));
            st4(dv + go, *reinterpret_cast<const float4*>(&sm.v[row * DS + c4 * 4]));
        }
    }
    if (HAS_BIAS)
        *reinterpret_cast<float4*>(dbias_part + (size_t)gw * NT * NT + (lane >> 2) * NT + (lane & 3) * 4) =
            make_float4(accb[0], accb[1], accb[2], accb[3]);
}

// ------------------------------------------------------------------------------------------------ padding words
// bits[b] of window b = image (nW) + window row (nWw) + window column of the UNSHIFTED H x W map: bit i = mask[img, 0, y Himg / H, x Wimg / W] != 0
// for token i = (y % win) win + x % win - nearest-neighbour resampling at a whole ratio.  One lane per token; a wave ballots 64 tokens
// (one 8 x 8 window, or four 4 x 4 windows whose words are the 16-bit fields).
__global__ __launch_bounds__(256) void pad_window_bits_kernel(const float* __restrict__ mask, uint64_t* __restrict__ bits, int Himg, int Wimg,
                                                              int H, int W, int lw, long long ntok) {
    const int win = 1 << lw, N = win * win;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;      // token of the window-ordered list
    const bool valid = e < ntok;
    float m = 0.f;
    long long b = 0;
    if (valid) {
        b = e >> (2 * lw);
        const int tok = (int)(e & (N - 1));
        const int nWw = W >> lw, nWi = (H >> lw) * nWw;
        const long long img = b / nWi;
        const int wdx = (int)(b % nWi);
        const int y = ((wdx / nWw) << lw) + (tok >> lw), x = ((wdx % nWw) << lw) + (tok & (win - 1));
        m = mask[(size_t)img * Himg * Wimg + (size_t)(y * (Himg / H)) * Wimg + x * (Wimg / W)];
    }
    const uint64_t bal = __builtin_amdgcn_ballot_w64(valid && m != 0.f);
    const int lane = threadIdx.x & 63;
    if (valid && (lane & (N - 1)) == 0) bits[b] = lw == 3 ? bal : ((bal >> (lane & 48)) & 0xffffull);
}

// ------------------------------------------------------------------------------------------------ small helpers, window = 1 << lw
__global__ void bias_gather_w_kernel(const float* __restrict__ table, float* __restrict__ bias, int H, int lw) {
    const int win = 1 << lw, N = win * win;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // over H * N * N
    if (e >= H * N * N) return;
    const int h = e / (N * N), i = (e / N) % N, j = e % N;
    const int rel = ((i >> lw) - (j >> lw) + win - 1) * (2 * win - 1) + ((i & (win - 1)) - (j & (win - 1)) + win - 1);
    bias[e] = table[rel * H + h];
}

__global__ void shift_mask_w_kernel(float* __restrict__ mask, int Hres, int Wres, int shift, int lw) {
    const int win = 1 << lw, N = win * win;
    const int nWw = Wres >> lw;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = (Hres >> lw) * nWw * N * N;
    if (e >= total) return;
    const int wdx = e / (N * N), i = (e / N) % N, j = e % N;
    const int wh = wdx / nWw, ww = wdx % nWw;
    auto label = [&](int tok) {
        const int hh = wh * win + (tok >> lw), wc = ww * win + (tok & (win - 1));
        const int lh = hh < Hres - win ? 0 : (hh < Hres - shift ? 1 : 2);
        const int lc = wc < Wres - win ? 0 : (wc < Wres - shift ? 1 : 2);
        return lh * 3 + lc;
    };
    mask[e] = (label(i) != label(j)) ? -100.0f : 0.0f;
}

// 16-token table gradient, one 1024-thread workgroup per head: thread (z, e) sums element e = (i, j) over the partials z, z + 4, ... of
// its head in ascending order, the four z meet in LDS in fixed order, and thread t < 49 adds the (i, j) pairs of table row t in fixed
// order: the same bits from run to run in every mode
__global__ __launch_bounds__(1024) void bias_table_grad16_kernel(const float* __restrict__ part, int parts, float* __restrict__ dtable,
                                                                 int H, int accumulate) {
    __shared__ float tab[4][NT * NT];
    const int h = blockIdx.x, e = threadIdx.x & 255, z = threadIdx.x >> 8;
    float s0 = 0.f, s1 = 0.f;
    int p = h + H * z;
    for (; p + 4 * H < parts; p += 8 * H) {               // two loads in flight
        const float a = part[(size_t)p * NT * NT + e], c = part[(size_t)(p + 4 * H) * NT * NT + e];
        s0 += a; s1 += c;
    }
    if (p < parts) s0 += part[(size_t)p * NT * NT + e];
    tab[z][e] = s0 + s1;
    __syncthreads();
    if (threadIdx.x < 256) tab[0][e] = ((tab[0][e] + tab[1][e]) + tab[2][e]) + tab[3][e];
    __syncthreads();
    if (threadIdx.x < 49) {
        const int di = (int)threadIdx.x / 7 - 3, dj = (int)threadIdx.x % 7 - 3;
        float sum = 0.f;
        for (int jh = 0; jh < 4; ++jh) {
            const int ih = jh + di;
            if ((unsigned)ih >= 4u) continue;
            for (int jw = 0; jw < 4; ++jw) {
                const int iw = jw + dj;
                if ((unsigned)iw < 4u) sum += tab[0][(ih * 4 + iw) * NT + jh * 4 + jw];
            }
        }
        float* dst = dtable + threadIdx.x * H + h;
        *dst = accumulate ? *dst + sum : sum;
    }
}

int win_log2(int win) { return win == 4 ? 2 : (win == 8 ? 3 : -1); }

#define DHZ_REQUIRE_WIN(who, win) DHZ_REQUIRE(win_log2(win) > 0, "%s: window %d unsupported (4 or 8)", who, win)

template <int D, typename T, bool DENSE>
void launch_fwd16(hipStream_t s, const T* q, const T* k, const T* v, int ld, const uint8_t* idx, const float* bias, const float* mask,
                  T* out, int ldo, uint8_t* rank, int B_, int H, int nW, float scale, const uint64_t* pad) {
    const int nwh = B_ * H, wgs = (nwh + 3) / 4;
    const int resident = PS16_FWD_WG(D) * dhz_num_cus();
    const size_t smem = 4 * sizeof(Fwd16<D>);
    if constexpr (!DENSE) {
        if (pad) {
            dhz_allow_smem(&attn16_fwd_kernel<D, T, false, true>, smem);
            hipLaunchKernelGGL((attn16_fwd_kernel<D, T, false, true>), dim3(wgs < resident ? wgs : resident), dim3(256), smem, s, q, k, v, ld, idx,
                               bias, mask, out, ldo, rank, H, nW, nwh, scale, PadArg<true>{pad});
            return;
        }
    }
    dhz_allow_smem(&attn16_fwd_kernel<D, T, DENSE>, smem);
    hipLaunchKernelGGL((attn16_fwd_kernel<D, T, DENSE>), dim3(wgs < resident ? wgs : resident), dim3(256), smem, s, q, k, v, ld, idx, bias,
                       mask, out, ldo, rank, H, nW, nwh, scale, PadArg<false>{});
}

template <typename T, bool DENSE>
int attn16_fwd(const char* who, const T* q, const T* k, const T* v, int ld, const uint8_t* idx, const float* bias, const float* mask, T* out,
               int ldo, uint8_t* rank, int B_, int H, int nW, int d, float scale, void* stream, const uint64_t* pad = nullptr) {
    DHZ_REQUIRE(q && k && v && out && (DENSE || (idx && rank)), "%s: null pointer", who);
    DHZ_REQUIRE(B_ > 0 && H > 0, "%s: B_=%d H=%d", who, B_, H);
    DHZ_REQUIRE(d == 16 || d == 32 || d == 64, "%s: head_dim %d unsupported (16, 32 or 64)", who, d);
    DHZ_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && ld >= H * d && ldo >= H * d, "%s: bad ld %d/%d", who, ld, ldo);
    DHZ_REQUIRE(!mask || (nW > 0 && B_ % nW == 0), "%s: B_=%d not a multiple of nW=%d", who, B_, nW);
    hipStream_t s = (hipStream_t)stream;
    if (nW <= 0) nW = 1;
    if (d == 16) launch_fwd16<16, T, DENSE>(s, q, k, v, ld, idx, bias, mask, out, ldo, rank, B_, H, nW, scale, pad);
    else if (d == 32) launch_fwd16<32, T, DENSE>(s, q, k, v, ld, idx, bias, mask, out, ldo, rank, B_, H, nW, scale, pad);
    else launch_fwd16<64, T, DENSE>(s, q, k, v, ld, idx, bias, mask, out, ldo, rank, B_, H, nW, scale, pad);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

// partial bias-gradient tiles (= waves with work) of the 16-token backward kernels
int parts16(int B_, int H, int d) {
    if (B_ <= 0 || H <= 0) return 0;
    const int cap = 4 * PS16_BWD_WG(d) * dhz_part_cus();          // (deterministic mode: a function of the shape)
    int per_head = cap / H;
    if (per_head < 1) per_head = 1;
    if (per_head > B_) per_head = B_;
    return per_head * H;
}

template <int D, typename T, bool DENSE>
void launch_bwd16(hipStream_t s, const T* q, const T* k, const T* v, int ld, const float* bias, const float* mask, const uint8_t* rank,
                  const T* dout, int ldo, T* dq, T* dk, T* dv, int ldg, float* dbias_part, int B_, int H, int nW, float scale,
                  const uint64_t* pad) {
    const int parts = parts16(B_, H, D);
    const size_t smem = 4 * sizeof(Bwd16<D>);
    if constexpr (!DENSE) {
        if (pad && bias) {
            dhz_allow_smem(&attn16_bwd_kernel<D, T, false, true, true>, smem);
            hipLaunchKernelGGL((attn16_bwd_kernel<D, T, false, true, true>), dim3((parts + 3) / 4), dim3(256), smem, s, q, k, v, ld, bias, mask, rank,
                               dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, parts, scale, PadArg<true>{pad});
            return;
        }
        if (pad) {
            dhz_allow_smem(&attn16_bwd_kernel<D, T, false, false, true>, smem);
            hipLaunchKernelGGL((attn16_bwd_kernel<D, T, false, false, true>), dim3((parts + 3) / 4), dim3(256), smem, s, q, k, v, ld, bias, mask, rank,
                               dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, parts, scale, PadArg<true>{pad});
            return;
        }
    }
    if (bias) {
        dhz_allow_smem(&attn16_bwd_kernel<D, T, DENSE, true>, smem);
        hipLaunchKernelGGL((attn16_bwd_kernel<D, T, DENSE, true>), dim3((parts + 3) / 4), dim3(256), smem, s, q, k, v, ld, bias, mask, rank, dout,
                           ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, parts, scale, PadArg<false>{});
    } else {
        dhz_allow_smem(&attn16_bwd_kernel<D, T, DENSE, false>, smem);
        hipLaunchKernelGGL((attn16_bwd_kernel<D, T, DENSE, false>), dim3((parts + 3) / 4), dim3(256), smem, s, q, k, v, ld, bias, mask, rank, dout,
                           ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, parts, scale, PadArg<false>{});
    }
}

template <typename T, bool DENSE>
int attn16_bwd(const char* who, const T* q, const T* k, const T* v, int ld, const float* bias, const float* mask, const uint8_t* rank,
               const T* dout, int ldo, T* dq, T* dk, T* dv, int ldg, float* dbias_part, int B_, int H, int nW, int d, float scale,
               void* stream, const uint64_t* pad = nullptr) {
    DHZ_REQUIRE(q && k && v && dout && dq && dk && dv && (DENSE || rank), "%s: null pointer", who);
    DHZ_REQUIRE(B_ > 0 && H > 0, "%s: B_=%d H=%d", who, B_, H);
    DHZ_REQUIRE(d == 16 || d == 32 || d == 64, "%s: head_dim %d unsupported (16, 32 or 64)", who, d);
    DHZ_REQUIRE(!bias || dbias_part, "%s: bias given but dbias_part is NULL", who);
    DHZ_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && ldg % 4 == 0 && ld >= H * d && ldo >= H * d && ldg >= H * d, "%s: bad ld %d/%d/%d", who, ld,
                ldo, ldg);
    DHZ_REQUIRE(!mask || (nW > 0 && B_ % nW == 0), "%s: B_=%d not a multiple of nW=%d", who, B_, nW);
    hipStream_t s = (hipStream_t)stream;
    if (nW <= 0) nW = 1;
    if (d == 16) launch_bwd16<16, T, DENSE>(s, q, k, v, ld, bias, mask, rank, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, scale, pad);
    else if (d == 32) launch_bwd16<32, T, DENSE>(s, q, k, v, ld, bias, mask, rank, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, scale, pad);
    else launch_bwd16<64, T, DENSE>(s, q, k, v, ld, bias, mask, rank, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, scale, pad);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
// win = 8 runs the existing entry (the same kernel instance, the same bits); win = 4 the kernels above; anything else is refused.
extern "C" int dhz_ps_attn_fwd_w(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias,
                                 const float* mask, void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d, int win, int dtype,
                                 void* stream) {
    DHZ_REQUIRE_WIN("dhz_ps_attn_fwd_w", win);
    if (win == 8) return dhz_ps_attn_fwd_dt(q, k, v, ld, idx, bias, mask, out, ldo, rank, B_, H, nW, d, dtype, stream);
    const float scale = d > 0 ? 1.0f / sqrtf((float)d) : 0.f;
    if (dtype == DHZ_F32)
        return attn16_fwd<float, false>("dhz_ps_attn_fwd_w", (const float*)q, (const float*)k, (const float*)v, ld, idx, bias, mask, (float*)out,
                                        ldo, rank, B_, H, nW, d, scale, stream);
    if (dtype == DHZ_BF16)
        return attn16_fwd<bf16s, false>("dhz_ps_attn_fwd_w", (const bf16s*)q, (const bf16s*)k, (const bf16s*)v, ld, idx, bias, mask, (bf16s*)out,
                                        ldo, rank, B_, H, nW, d, scale, stream);
    dhz_set_error("dhz_ps_attn_fwd_w: unknown dtype %d", dtype);
    return DHZ_EINVAL;
}

extern "C" int dhz_ps_attn_bwd_parts_w(int B_, int H, int d, int win) {
    if (win == 8) return dhz_ps_attn_bwd_parts_d(B_, H, d);
    return win == 4 ? parts16(B_, H, d) : 0;
}

extern "C" int dhz_ps_attn_bwd_w(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask,
                                 const uint8_t* rank, const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg, float* dbias_part,
                                 int B_, int H, int nW, int d, int win, int dtype, void* stream) {
    DHZ_REQUIRE_WIN("dhz_ps_attn_bwd_w", win);
    if (win == 8) return dhz_ps_attn_bwd_dt(q, k, v, ld, bias, mask, rank, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, d, dtype, stream);
    const float scale = d > 0 ? 1.0f / sqrtf((float)d) : 0.f;
    if (dtype == DHZ_F32)
        return attn16_bwd<float, false>("dhz_ps_attn_bwd_w", (const float*)q, (const float*)k, (const float*)v, ld, bias, mask, rank,
                                        (const float*)dout, ldo, (float*)dq, (float*)dk, (float*)dv, ldg, dbias_part, B_, H, nW, d, scale, stream);
    if (dtype == DHZ_BF16)
        return attn16_bwd<bf16s, false>("dhz_ps_attn_bwd_w", (const bf16s*)q, (const bf16s*)k, (const bf16s*)v, ld, bias, mask, rank,
                                        (const bf16s*)dout, ldo, (bf16s*)dq, (bf16s*)dk, (bf16s*)dv, ldg, dbias_part, B_, H, nW, d, scale, stream);
    dhz_set_error("dhz_ps_attn_bwd_w: unknown dtype %d", dtype);
    return DHZ_EINVAL;
}

// padding-bit forms: pad[B_] uint64, bit i of word b = token i of GLOBAL window b is padding (4 x 4 windows: the low 16 bits); the shift
// mask keeps b % nW.  win = 8 runs dhz_ps_attn_fwd_dt_pad / dhz_ps_attn_bwd_dt_pad.
#define DHZ_REQUIRE_PAD(who)                                                                                       \
    DHZ_REQUIRE(pad, "%s: pad is NULL (the entry without _pad takes no padding words)", who);                      \
    DHZ_REQUIRE(nW > 0 && B_ % nW == 0, "%s: B_=%d is not a whole number of images of nW=%d windows", who, B_, nW)
extern "C" int dhz_ps_attn_fwd_w_pad(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias,
                                     const float* mask, const uint64_t* pad, void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d,
                                     int win, int dtype, void* stream) {
    DHZ_REQUIRE_WIN("dhz_ps_attn_fwd_w_pad", win);
    if (win == 8) return dhz_ps_attn_fwd_dt_pad(q, k, v, ld, idx, bias, mask, pad, out, ldo, rank, B_, H, nW, d, dtype, stream);
    DHZ_REQUIRE_PAD("dhz_ps_attn_fwd_w_pad");
    const float scale = d > 0 ? 1.0f / sqrtf((float)d) : 0.f;
    if (dtype == DHZ_F32)
        return attn16_fwd<float, false>("dhz_ps_attn_fwd_w_pad", (const float*)q, (const float*)k, (const float*)v, ld, idx, bias, mask, (float*)out,
                                        ldo, rank, B_, H, nW, d, scale, stream, pad);
    if (dtype == DHZ_BF16)
        return attn16_fwd<bf16s, false>("dhz_ps_attn_fwd_w_pad", (const bf16s*)q, (const bf16s*)k, (const bf16s*)v, ld, idx, bias, mask, (bf16s*)out,
                                        ldo, rank, B_, H, nW, d, scale, stream, pad);
    dhz_set_error("dhz_ps_attn_fwd_w_pad: unknown dtype %d", dtype);
    return DHZ_EINVAL;
}

extern "C" int dhz_ps_attn_bwd_w_pad(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask,
                                     const uint64_t* pad, const uint8_t* rank, const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg,
                                     float* dbias_part, int B_, int H, int nW, int d, int win, int dtype, void* stream) {
    DHZ_REQUIRE_WIN("dhz_ps_attn_bwd_w_pad", win);
    if (win == 8)
        return dhz_ps_attn_bwd_dt_pad(q, k, v, ld, bias, mask, pad, rank, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, d, dtype, stream);
    DHZ_REQUIRE_PAD("dhz_ps_attn_bwd_w_pad");
    const float scale = d > 0 ? 1.0f / sqrtf((float)d) : 0.f;
    if (dtype == DHZ_F32)
        return attn16_bwd<float, false>("dhz_ps_attn_bwd_w_pad", (const float*)q, (const float*)k, (const float*)v, ld, bias, mask, rank,
                                        (const float*)dout, ldo, (float*)dq, (float*)dk, (float*)dv, ldg, dbias_part, B_, H, nW, d, scale, stream, pad);
    if (dtype == DHZ_BF16)
        return attn16_bwd<bf16s, false>("dhz_ps_attn_bwd_w_pad", (const bf16s*)q, (const bf16s*)k, (const bf16s*)v, ld, bias, mask, rank,
                                        (const bf16s*)dout, ldo, (bf16s*)dq, (bf16s*)dk, (bf16s*)dv, ldg, dbias_part, B_, H, nW, d, scale, stream, pad);
    dhz_set_error("dhz_ps_attn_bwd_w_pad: unknown dtype %d", dtype);
    return DHZ_EINVAL;
}
#undef DHZ_REQUIRE_PAD

extern "C" int dhz_pad_window_bits(const float* mask, uint64_t* bits, int B, int Himg, int Wimg, int H, int W, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_pad_window_bits", win);
    DHZ_REQUIRE(mask && bits, "dhz_pad_window_bits: null pointer (mask, bits)");
    DHZ_REQUIRE(B > 0 && H > 0 && W > 0 && H % win == 0 && W % win == 0, "dhz_pad_window_bits: B=%d, map H x W = %d x %d is no multiple of win=%d", B,
                H, W, win);
    DHZ_REQUIRE(Himg > 0 && Wimg > 0 && Himg % H == 0 && Wimg % W == 0,
                "dhz_pad_window_bits: Himg x Wimg = %d x %d is no whole multiple of H x W = %d x %d (nearest resampling at a whole ratio only)", Himg,
                Wimg, H, W);
    const long long ntok = (long long)B * H * W;
    DHZ_REQUIRE((ntok + 255) / 256 < (1ll << 31), "dhz_pad_window_bits: B H W = %lld tokens exceed the grid", ntok);
    hipLaunchKernelGGL(pad_window_bits_kernel, dim3((unsigned)((ntok + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, bits, Himg, Wimg, H,
                       W, win_log2(win), ntok);
    DHZ_CHECK_LAUNCH("dhz_pad_window_bits");
    return DHZ_OK;
}

extern "C" int dhz_dense_attn_fwd_w(const float* q, const float* k, const float* v, int ld, const float* bias, const float* mask, float* out,
                                    int ldo, int B_, int H, int nW, int d, float scale, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_dense_attn_fwd_w", win);
    if (win == 8) return dhz_dense_attn_fwd(q, k, v, ld, bias, mask, out, ldo, B_, H, nW, d, scale, stream);
    return attn16_fwd<float, true>("dhz_dense_attn_fwd_w", q, k, v, ld, nullptr, bias, mask, out, ldo, nullptr, B_, H, nW, d, scale, stream);
}

extern "C" int dhz_dense_attn_bwd_w(const float* q, const float* k, const float* v, int ld, const float* bias, const float* mask,
                                    const float* dout, int ldo, float* dq, float* dk, float* dv, int ldg, float* dbias_part, int B_, int H,
                                    int nW, int d, float scale, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_dense_attn_bwd_w", win);
    if (win == 8) return dhz_dense_attn_bwd(q, k, v, ld, bias, mask, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW, d, scale, stream);
    return attn16_bwd<float, true>("dhz_dense_attn_bwd_w", q, k, v, ld, bias, mask, nullptr, dout, ldo, dq, dk, dv, ldg, dbias_part, B_, H, nW,
                                   d, scale, stream);
}

extern "C" int dhz_bias_gather_w(const float* table, float* bias, int H, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_bias_gather_w", win);
    if (win == 8) return dhz_bias_gather(table, bias, H, stream);
    DHZ_REQUIRE(table && bias && H > 0, "dhz_bias_gather_w: bad arguments");
    const int n = H * NT * NT;
    hipLaunchKernelGGL(bias_gather_w_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, table, bias, H, win_log2(win));
    DHZ_CHECK_LAUNCH("dhz_bias_gather_w");
    return DHZ_OK;
}

extern "C" int dhz_bias_table_grad_w(const float* dbias_part, int parts, float* dtable, int H, int accumulate, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_bias_table_grad_w", win);
    if (win == 8) return dhz_bias_table_grad(dbias_part, parts, dtable, H, accumulate, stream);
    DHZ_REQUIRE(dbias_part && dtable && H > 0 && parts > 0 && parts % H == 0, "dhz_bias_table_grad_w: bad arguments");
    hipLaunchKernelGGL(bias_table_grad16_kernel, dim3(H), dim3(1024), 0, (hipStream_t)stream, dbias_part, parts, dtable, H, accumulate);
    DHZ_CHECK_LAUNCH("dhz_bias_table_grad_w");
    return DHZ_OK;
}

extern "C" int dhz_shift_mask_w(float* mask, int Hres, int Wres, int shift, int win, void* stream) {
    DHZ_REQUIRE_WIN("dhz_shift_mask_w", win);
    if (win == 8) return dhz_shift_mask(mask, Hres, Wres, shift, stream);
    DHZ_REQUIRE(mask && Hres % win == 0 && Wres % win == 0 && Hres > win && Wres > win && shift > 0 && shift < win,
                "dhz_shift_mask_w: bad arguments %dx%d shift %d window %d", Hres, Wres, shift, win);
    const int n = (Hres / win) * (Wres / win) * NT * NT;
    hipLaunchKernelGGL(shift_mask_w_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, mask, Hres, Wres, shift, win_log2(win));
    DHZ_CHECK_LAUNCH("dhz_shift_mask_w");
    return DHZ_OK;
}
