// LeFF depthwise backward that forms dz itself: dz = dy . W2 is a thin product (contraction C, result 4C wide) whose output the kernel
// chain writes to HBM once and reads once - by leff_dwconv_bwd_kernel (csrc/elementwise.hip), which is HBM-bound with an idle matrix
// pipe.  This variant of that kernel (fp32 storage, 8 lanes per position, 32 channels x an 8 x 16 tile per workgroup, persistent over
// the tiles of one channel group) computes the tile's dz with its one-pixel halo on the bf16 matrix pipe while it stages dt:
//   - the 180 halo positions are padded to 12 MFMA tiles of 16 positions, three per wave; the 32 channels are two tiles of 16;
//   - the rows of dy (token order, clamped into the image like the staging loads) go from global memory straight into registers, 8
//     consecutive c per lane, and are cut there into three bf16 pieces (dhz_split8x3): no LDS image of them;
//   - the workgroup's 32 rows of the three planes of W2^T ([4C][C]: a channel's 8 consecutive c are 16 bytes) are fetched ONCE per
//     workgroup into LDS in fragment order (6 KB per 32 of C): the channel group never changes over a workgroup's life;
//   - six-term product, small terms first (lh hl mm hm mh hh), fp32 accumulation, v_mfma_f32_16x16x32_bf16 with the WEIGHT fragment as
//     the first operand: a lane then holds dz of 4 consecutive channels of one position - the float4 slot of the dt tile - so
//     dt = scale . dz . gelu'(t) is formed in registers from the lane's own tpre load and stored where the staging stored it; no
//     second pass over the tile, no extra barrier.
// Everything after the staging is leff_dwconv_bwd_kernel's: the position loop, the dw / db register sums, the two-round LDS reduction
// and the DET instance.
// LDS: 39.4 KB + 6 / 12 / 24 KB at C = 32 / 64 / 128: three workgroups per CU at C <= 64, two at C = 128.
// Grid numbering: the 4C / 32 channel groups of a tile all read the same rows of dy; workgroups are dealt round-robin to the 8 XCDs and
// are renumbered (as leff_dwconv_fwd_kernel does) so that a tile's channel groups share one XCD's L2.  DHZ_DWZ_PLAIN_ORDER in the
// environment keeps the plain order (diagnostics, tools/bench_leff_bwd_dz.py).
#include "bf16_pipe.h"
#include <stdlib.h>

namespace {
constexpr int TW = 16, TH = 8;                 // spatial tile (positions), as csrc/elementwise.hip
constexpr int HWID = TW + 2, HHGT = TH + 2;    // with halo
constexpr int CT = 32;                         // channels per workgroup
constexpr int NPOS = HHGT * HWID;              // 180 halo positions: 12 row tiles of 16, the last 12 rows idle

template <int KB, bool DET>                    // KB = C / 32
__global__ __launch_bounds__(256, KB == 4 ? 2 : 3) void leff_dwconv_bwd_dy_kernel(
    const float* __restrict__ dy, int ldy, const uint16_t* __restrict__ wt_hi, const uint16_t* __restrict__ wt_mid,
    const uint16_t* __restrict__ wt_lo, const float* __restrict__ u, const float* __restrict__ tpre, const float* __restrict__ w,
    float* __restrict__ du, float* __restrict__ dw, float* __restrict__ db, const float* __restrict__ dzscale, int B, int Hres,
    int Wres, int Ch, int tiles_x, int tiles_y, int wg_per_cg, int renumber) {
    constexpr int C = 32 * KB, LPP = 8;
    __shared__ __attribute__((aligned(16))) float ds[NPOS * CT];           // dt = scale dz gelu'(t) with halo
    __shared__ __attribute__((aligned(16))) float us[TH * TW * CT];        // u of the tile: each thread parks ITS OWN loads here
    __shared__ dhz_u32x4 wf[KB * 2 * 3 * 64];                              // W2^T fragments [k block][channel tile][piece][lane]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, i16 = lane & 15, g = lane >> 4;
    const int ncg = Ch / CT;
    const int lid = renumber ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int cg = lid % ncg;
    const int wslot = lid / ncg;
    const int c4 = t % LPP, ch0 = cg * CT + c4 * 4;
    for (int e = t; e < KB * 2 * 3 * 64; e += 256) {
        const int l = e & 63, f = e >> 6, pc = f % 3, ct = (f / 3) & 1, kb = f / 6;
        const uint16_t* pl = pc == 0 ? wt_hi : (pc == 1 ? wt_mid : wt_lo);
        wf[e] = *reinterpret_cast<const dhz_u32x4*>(pl + (size_t)(cg * CT + 16 * ct + (l & 15)) * C + 32 * kb + 8 * (l >> 4));
    }
    float wk[4][9], dwk[4][9], dbk[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) { wk[c][kk] = w[(ch0 + c) * 9 + kk]; dwk[c][kk] = 0.f; }
    const int ntiles = B * tiles_x * tiles_y;
    constexpr int NIT = TH * TW / 32;                                       // interior positions per thread
    for (int tile = wslot; tile < ntiles; tile += wg_per_cg) {
        const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, bimg = tile / (tiles_x * tiles_y);
        const int x0 = tx * TW - 1, y0 = ty * TH - 1;
        const size_t ib = (size_t)bimg * Hres * Wres;
        const float zsc = dzscale ? dzscale[bimg] : 1.f;     // per-image factor of dz (the DropPath scale)
        __syncthreads();                                     // (the first trip: wf is complete)
        // this thread's u values (interior positions; clamped addresses, masked at the store): in flight across the staging
        float4 uv[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int pos = (t / LPP) + 32 * it;
            const int yy = min(ty * TH + pos / TW, Hres - 1), xx = min(tx * TW + pos % TW, Wres - 1);
            uv[it] = ld4(u + (ib + (size_t)yy * Wres + xx) * Ch + ch0);
        }
        // staging of dt: wave wv owns halo positions 48 wv .. 48 wv + 47 (three MFMA tiles, one after the other: 8 accumulator registers at
        // a time), lane (i16, g) position i16 of each and channels 16 ct + 4 g .. + 3 of both channel tiles.  gelu'(t) of those slots and
        // the dy row are requested first, then the product, then dt goes to its slot.
        constexpr int TA[6] = {2, 0, 1, 0, 1, 0}, TB[6] = {0, 2, 1, 1, 0, 0};          // (token piece, weight piece): lh hl mm hm mh hh
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {                            // (not unrolled: the loads of all three tiles hoisted cost spills)
            const int pos = 16 * (3 * wv + a) + i16;
            const int pc = pos < NPOS ? pos : NPOS - 1;
            const int yy = y0 + pc / HWID, xx = x0 + pc % HWID;
            const bool ok = pos < NPOS && yy >= 0 && yy < Hres && xx >= 0 && xx < Wres;
            const int yc = min(max(yy, 0), Hres - 1), xc = min(max(xx, 0), Wres - 1);
            const size_t tok = ib + (size_t)yc * Wres + xc;
            const float* dyrow = dy + tok * ldy + 8 * g;
            f32x4 r[KB][2];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                r[kb][0] = ld4v(dyrow + 32 * kb);
                r[kb][1] = ld4v(dyrow + 32 * kb + 4);
            }
            float4 rt[2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) rt[ct] = ld4(tpre + tok * Ch + cg * CT + 16 * ct + 4 * g);      // tpre holds gelu'(t)
            if (a == 0) {                                        // u is here by now (requested first): park it, free its registers
#pragma unroll
                for (int it = 0; it < NIT; ++it) *reinterpret_cast<float4*>(&us[((t / LPP) + 32 * it) * CT + c4 * 4]) = uv[it];
            }
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            // C = 32 keeps its 6 weight fragments in registers across tiles (the compiler hoists the LDS reads); beyond that they would
            // take 48 / 96 registers: the fragment index is made opaque so that they are read where they are used
            int wl = lane;
            if (KB > 1) asm volatile("" : "+v"(wl));
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                dhz_u32x4 p[3];
                dhz_split8x3(r[kb][0], r[kb][1], p[0], p[1], p[2]);
#pragma unroll
                for (int term = 0; term < 6; ++term)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        acc[ct] = dhz_mfma_bf16(wf[((kb * 2 + ct) * 3 + TB[term]) * 64 + wl], p[TA[term]], acc[ct]);
            }
            if (pos < NPOS) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    float4 dv = make_float4(0, 0, 0, 0);
                    if (ok) dv = make_float4(zsc * acc[ct][0] * rt[ct].x, zsc * acc[ct][1] * rt[ct].y, zsc * acc[ct][2] * rt[ct].z,
                                             zsc * acc[ct][3] * rt[ct].w);
                    *reinterpret_cast<float4*>(&ds[pos * CT + 16 * ct + 4 * g]) = dv;
                }
            }
        }
        __syncthreads();
        // the position loop is NOT unrolled (see leff_dwconv_bwd_kernel)
#pragma unroll 1
        for (int it = 0; it < NIT; ++it) {
            const int pos = (t / LPP) + 32 * it;
            const int py = pos / TW, px = pos % TW;
            const int yy = ty * TH + py, xx = tx * TW + px;
            if (yy >= Hres || xx >= Wres) continue;
            const size_t o = (ib + (size_t)yy * Wres + xx) * Ch + ch0;
            const float4 uc = *reinterpret_cast<const float4*>(&us[pos * CT + c4 * 4]);
            f32x4 gv, pv;                                                // gelu(u), gelu'(u) of this position
            gelu_both4(f32x4{uc.x, uc.y, uc.z, uc.w}, gv, pv);
            float4 dg = make_float4(0, 0, 0, 0);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float4 dn = *reinterpret_cast<const float4*>(&ds[((py + 2 - ky) * HWID + px + 2 - kx) * CT + c4 * 4]);
                    dg.x += wk[0][ky * 3 + kx] * dn.x; dg.y += wk[1][ky * 3 + kx] * dn.y;
                    dg.z += wk[2][ky * 3 + kx] * dn.z; dg.w += wk[3][ky * 3 + kx] * dn.w;
                    if (ky == 1 && kx == 1) { dbk[0] += dn.x; dbk[1] += dn.y; dbk[2] += dn.z; dbk[3] += dn.w; }
                    dwk[0][ky * 3 + kx] += gv[0] * dn.x; dwk[1][ky * 3 + kx] += gv[1] * dn.y;
                    dwk[2][ky * 3 + kx] += gv[2] * dn.z; dwk[3][ky * 3 + kx] += gv[3] * dn.w;
                }
            st4(du + o, make_float4(dg.x * pv[0], dg.y * pv[1], dg.z * pv[2], dg.w * pv[3]));
        }
    }
    // reduce the 32 position-slots (t / LPP) that share a channel quad: five quantities per round through the dead dt tile
    const int ps = t / LPP;
    float* red5 = ds;
    static_assert(NPOS * CT >= 5 * 32 * CT, "reduction scratch must fit the dt tile");
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int kk = 5 * half + q;
#pragma unroll
            for (int c = 0; c < 4; ++c) red5[(q * 32 + ps) * CT + c4 * 4 + c] = (kk < 9) ? dwk[c][kk] : dbk[c];
        }
        __syncthreads();
        if (t < 5 * CT) {
            const int q = t / CT, c = t % CT, kk = 5 * half + q;
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < 32; ++p) sum += red5[(q * 32 + p) * CT + c];
            const size_t det_off = DET ? (size_t)wslot * 10 * Ch : 0;
            if (kk < 9) dhz_accum<DET>(dw + det_off + (cg * CT + c) * 9 + kk, sum);
            else dhz_accum<DET>(db + det_off + cg * CT + c, sum);
        }
    }
}

template <bool DET>
void launch(int C, int grid, hipStream_t s, const float* dy, int ldy, const uint16_t* hi, const uint16_t* mid, const uint16_t* lo,
            const float* u, const float* tpre, const float* wd, float* du, float* dw, float* db, const float* dz_scale, int B, int Hres,
            int Wres, int Ch, int tiles_x, int tiles_y, int wg_per_cg, int renumber) {
#define DWZ(KB_) hipLaunchKernelGGL((leff_dwconv_bwd_dy_kernel<KB_, DET>), dim3(grid), dim3(256), 0, s, dy, ldy, hi, mid, lo, u, tpre, wd, du, \
                                    dw, db, dz_scale, B, Hres, Wres, Ch, tiles_x, tiles_y, wg_per_cg, renumber)
    if (C == 32) DWZ(1); else if (C == 64) DWZ(2); else DWZ(4);
#undef DWZ
}
}  // namespace

extern "C" int dhz_leff_dwconv_bwd_dy(const float* dy, int ldy, const void* w2t_hi, const void* w2t_mid, const void* w2t_lo,
                                      const float* u, const float* tpre, const float* wd, float* du, float* dw, float* db,
                                      const float* dz_scale, int B, int Hres, int Wres, int C, int Ch, void* stream) {
    const char* who = "dhz_leff_dwconv_bwd_dy";
    DHZ_REQUIRE(dy && w2t_hi && w2t_mid && w2t_lo && u && tpre && wd && du && dw && db, "%s: null pointer", who);
    DHZ_REQUIRE(C == 32 || C == 64 || C == 128, "%s: C=%d must be 32, 64 or 128", who, C);
    DHZ_REQUIRE(B > 0 && Hres > 0 && Wres > 0 && Ch > 0 && Ch % CT == 0, "%s: Ch=%d must be a multiple of %d", who, Ch, CT);
    DHZ_REQUIRE(ldy % 4 == 0 && ldy >= C, "%s: ldy=%d must be a multiple of 4 and at least C=%d", who, ldy, C);
    DHZ_REQUIRE(!(((uintptr_t)dy | (uintptr_t)w2t_hi | (uintptr_t)w2t_mid | (uintptr_t)w2t_lo | (uintptr_t)u | (uintptr_t)tpre |
                   (uintptr_t)du) & 15), "%s: dy, the planes, u, tpre and du must be 16-byte aligned", who);
    const int tiles_x = (Wres + TW - 1) / TW, tiles_y = (Hres + TH - 1) / TH;
    const int ntiles = B * tiles_x * tiles_y, ncg = Ch / CT;
    int wg_per_cg = (C == 128 ? 2 : 3) * dhz_part_cus() / ncg;    // one resident round, persistent over tiles
    if (wg_per_cg < 1) wg_per_cg = 1;
    if (wg_per_cg > ntiles) wg_per_cg = ntiles;
    const int grid = wg_per_cg * ncg;
    static const bool plain = getenv("DHZ_DWZ_PLAIN_ORDER") != nullptr;
    const int renumber = !plain && grid % 8 == 0;
    const uint16_t *hi = (const uint16_t*)w2t_hi, *mid = (const uint16_t*)w2t_mid, *lo = (const uint16_t*)w2t_lo;
    if (dhz_det()) {                     // one item per workgroup slot, as dhz_leff_dwconv_bwd_scaled_dt
        float* ws = dhz_det_ws(who, wg_per_cg, 10L * Ch);
        if (!ws) return DHZ_EINVAL;
        launch<true>(C, grid, (hipStream_t)stream, dy, ldy, hi, mid, lo, u, tpre, wd, du, ws, ws + 9L * Ch, dz_scale, B, Hres, Wres, Ch,
                     tiles_x, tiles_y, wg_per_cg, renumber);
        DHZ_CHECK_LAUNCH(who);
        DetSegs segs{};
        segs.n = 2;
        segs.off[0] = 0; segs.len[0] = 9L * Ch; segs.dst[0] = dw;
        segs.off[1] = 9L * Ch; segs.len[1] = Ch; segs.dst[1] = db;
        return dhz_det_reduce(who, ws, wg_per_cg, 10L * Ch, segs, (hipStream_t)stream);
    }
    launch<false>(C, grid, (hipStream_t)stream, dy, ldy, hi, mid, lo, u, tpre, wd, du, dw, db, dz_scale, B, Hres, Wres, Ch, tiles_x, tiles_y,
                  wg_per_cg, renumber);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}
