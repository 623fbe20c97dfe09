// K11w - weight and bias gradient of a dense 3x3 / stride 1 / pad 1 convolution on the channel-blocked layout of the Winograd kernels
// (x[b][c/8][h][w][c%8], csrc/winograd_conv.hip): what autograd runs for nn.Conv2d(C, K, 3, padding=1) of the UNet baseline's ConvBlock
// (M1:28-40) - aten::convolution_backward's weight / bias outputs - without a repacking pass between forward, backward-data and this.
//
//   dW[k][c][r][s] = sum_{b,h,w} dy[b][k][h][w] * x[b][c][h+r-1][w+s-1]        db[k] = sum_{b,h,w} dy[b][k][h][w]
//
// Nine implicit GEMMs (one per tap) with a tiny result (Kout x Cin) and a contraction over every position B*H*W, so the contraction is
// what gets split.  The cut:
//   chunk  = 64 output positions: 4 rows x 16 columns of one image (H, W multiples of 16), or one whole 8 x 8 image; the `_any` entries
//            take every other map too, as ceil(H / 4) x ceil(W / 16) chunks per image whose positions outside the map are zeros in LDS
//            (never loaded), so that they add zero to dW and db;
//   slab   = a run of consecutive chunks; `slabs` of them, min(ceil(512 / tiles), chunks / 4) - a function of the shapes alone;
//   tile   = 32 output channels x 32 input channels (all nine taps);
//   item   = (slab, tile): one workgroup accumulates the tile over the slab's chunks in fp32 on v_mfma_f32_16x16x4_f32 and STORES it to
//            slot `slab` of the workspace ([slabs][Kout*Cin*9 + Kout], the layout of dW followed by db).
// A persistent grid (4 workgroups per CU) walks the items; which workgroup computes an item changes no bit of it.  A second kernel sums
// the slots in ascending slab order, one owner thread per element, and writes dW / db.  No atomics anywhere: the result is the same from
// run to run, under any CU reservation and with the deterministic mode on or off (the mode only chooses whose workspace is used).
//
// A workgroup = 4 waves; wave w owns the 16 x 16 sub-tile (k half w & 1, c half w >> 1) for all nine taps: 9 accumulators of 4 VGPRs.
// Per chunk the workgroup stages dy [64 px][32 k] and the x patch [(4+2) x (16+2) px][32 c] in LDS, pixel-major with 48 floats per pixel
// (32 channels + 16 pad: the four pixels x 16 channels a wave reads in one ds_read_b32 fall into 64 distinct banks).  Patch pixels outside
// the map are zeros written to LDS; they are never loaded.  The next chunk's global loads are issued before the 144 MFMAs of this one.
#include <limits.h>
#include "common.h"

namespace {

constexpr int TKC = 32;            // tile side, both channel axes
constexpr int NPOS = 64;           // positions per chunk
constexpr int PS = 48;             // LDS floats per pixel
constexpr int MIN_CHUNKS = 4;      // chunks per slab at least (where the problem has that many)
constexpr int TARGET_ITEMS = 512;  // items aimed at: two workgroups per CU of a 256-CU device
constexpr int WG_PER_CU = 4;
constexpr int NTHR = 256;

enum { MODE_M16 = 0, MODE_Q8 = 1, MODE_RAGGED = 2 };   // kernel instances: whole 4 x 16 chunks; one 8 x 8 image per chunk; 4 x 16 chunks cut by the map's edge

struct Cut {
    bool ok;
    int mode;
    int nchunks, tiles, slabs;
    long wlen, slot;               // floats of dW; floats of one workspace slot (dW + db)
};

// any: the `_any` entries (every H, W >= 1); otherwise multiples of 16, or 8 x 8
Cut make_cut(int B, int H, int W, int Cin, int Kout, bool any) {
    Cut c{};
    c.mode = H == 8 && W == 8 ? MODE_Q8 : (H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 ? MODE_M16 : MODE_RAGGED);
    c.ok = B >= 1 && Cin >= TKC && Kout >= TKC && Cin <= 512 && Kout <= 512 && Cin % TKC == 0 && Kout % TKC == 0 &&
           (c.mode != MODE_RAGGED || (any && H >= 1 && W >= 1));
    if (!c.ok) return c;
    const long nch = c.mode == MODE_Q8 ? (long)B : (long)B * ((H + 3) / 4) * ((W + 15) / 16);
    if (nch > INT_MAX / NPOS) { c.ok = false; return c; }         // B*H*W fits an int
    c.nchunks = (int)nch;
    c.tiles = (Kout / TKC) * (Cin / TKC);
    const int want = (TARGET_ITEMS + c.tiles - 1) / c.tiles;
    const int cap = c.nchunks / MIN_CHUNKS > 1 ? c.nchunks / MIN_CHUNKS : 1;
    c.slabs = want < cap ? want : cap;
    c.wlen = (long)Kout * Cin * 9;
    c.slot = c.wlen + Kout;
    return c;
}

template <int MODE>
__global__ __launch_bounds__(NTHR) void conv3x3_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ ws, int H, int W, int Cin, int Kout, int nchunks,
                                                             int slabs, long slot, int with_db) {
    constexpr bool Q8 = MODE == MODE_Q8;
    constexpr int CH = Q8 ? 8 : 4, CW = Q8 ? 8 : 16;            // chunk rows x columns
    constexpr int PW = CW + 2, NPATCH = (CH + 2) * PW;           // patch: 6 x 18 = 108 px, or 10 x 10 = 100 px
    constexpr int NX = (NPATCH * 8 + NTHR - 1) / NTHR;           // float4 patch slots per thread (4)
    __shared__ __attribute__((aligned(16))) float dyl[NPOS * PS];
    __shared__ __attribute__((aligned(16))) float xl[NPATCH * PS];
    __shared__ float red[8 * TKC];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int ktw = w & 1, ctw = w >> 1;
    const int CT = Cin / TKC, tiles = (Kout / TKC) * CT;
    const int items = slabs * tiles;
    const size_t plane = (size_t)H * W * 8;
    const int bxn = Q8 ? 1 : (W + 15) / 16, cpi = Q8 ? 1 : ((H + 3) / 4) * bxn;     // chunks per image row group / per image

    // per-thread staging slots, fixed for the whole kernel: float4 e = t + 256 i of the dy chunk -> (pixel, channel group, half),
    // of the patch -> (patch pixel, channel group, half; group >= 4: no such slot).  Recomputed where used: constants of t.
#define DY_SLOT(i) const int e_ = t + NTHR * (i), hf = e_ & 1, pix = (e_ >> 1) & 63, cg = e_ >> 7
#define X_SLOT(i) const int e_ = t + NTHR * (i), hf = e_ & 1, cg = (e_ >> 1) / NPATCH, pp = (e_ >> 1) % NPATCH

    for (int item = blockIdx.x; item < items; item += gridDim.x) {
        const int slab = item / tiles, tile = item % tiles;
        const int kt = tile / CT, ct = tile % CT;
        const int q0 = (int)((long)slab * nchunks / slabs), q1 = (int)((long)(slab + 1) * nchunks / slabs);
        const bool do_db = with_db && ct == 0;

        f32x4 acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        float dbacc = 0.f;

        f32x4 rdy[2], rx[NX];
        auto gload = [&](int q) {
            const int b = q / cpi, rem = q % cpi;
            const int y0 = Q8 ? 0 : (rem / bxn) * 4, x0 = Q8 ? 0 : (rem % bxn) * 16;
            const float* dyb = dy + ((size_t)b * (Kout / 8) + kt * 4) * plane;
            const float* xb = x + ((size_t)b * (Cin / 8) + ct * 4) * plane;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                DY_SLOT(i);
                const int py = pix / CW, px = pix % CW;
                if (MODE == MODE_RAGGED) {                                                       // behind the map's edge: zeros, never read
                    rdy[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (y0 + py < H && x0 + px < W) rdy[i] = ld4v(dyb + cg * plane + ((size_t)(y0 + py) * W + x0 + px) * 8 + hf * 4);
                } else {
                    rdy[i] = ld4v(dyb + cg * plane + ((size_t)(y0 + py) * W + x0 + px) * 8 + hf * 4);
                }
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                X_SLOT(i);
                const int iy = y0 - 1 + pp / PW, ix = x0 - 1 + pp % PW;
                const bool in = cg < 4 && iy >= 0 && iy < H && ix >= 0 && ix < W;           // the halo outside the map is never read
                rx[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (in) rx[i] = ld4v(xb + cg * plane + ((size_t)iy * W + ix) * 8 + hf * 4);
            }
        };
        gload(q0);
        for (int q = q0; q < q1; ++q) {
            __syncthreads();                                      // the previous chunk's reads are done
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                DY_SLOT(i);
                st4v(dyl + pix * PS + cg * 8 + hf * 4, rdy[i]);
            }
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                X_SLOT(i);
                if (cg < 4) st4v(xl + pp * PS + cg * 8 + hf * 4, rx[i]);
            }
            __syncthreads();
            if (q + 1 < q1) gload(q + 1);                         // in flight during the MFMAs
            const float* ap = dyl + g * PS + ktw * 16 + i16;
            const float* bp = xl + g * PS + ctw * 16 + i16;
#pragma unroll
            for (int s = 0; s < NPOS / 4; ++s) {                  // lane group g contracts position p = 4 s + g
                const int py = (4 * s) / CW, px = (4 * s) % CW;   // p's row and (less g) column: CW % 4 == 0
                const float a = ap[4 * s * PS];
                const float* b0 = bp + (py * PW + px) * PS;
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[r * 3 + c] = mfma16(a, b0[(r * PW + c) * PS], acc[r * 3 + c]);
            }
            if (do_db) {                                          // thread = (channel t & 31, positions t >> 5 + 8 j), fixed order
                const float* dp = dyl + (t >> 5) * PS + (t & 31);
#pragma unroll
                for (int j = 0; j < 8; ++j) dbacc += dp[8 * j * PS];
            }
        }
        // the tile's partial -> slot `slab`, in the layout of dW: acc[tap][j] = D[k = 4 g + j][c = i16]
        float* o = ws + (size_t)slab * slot;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kt * TKC + ktw * 16 + 4 * g + j, c = ct * TKC + ctw * 16 + i16;
            float* d = o + ((size_t)k * Cin + c) * 9;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) d[tap] = acc[tap][j];
        }
        if (do_db) {
            red[t] = dbacc;
            __syncthreads();
            if (t < TKC) {
                float sum = 0.f;
#pragma unroll
                for (int p = 0; p < 8; ++p) sum += red[p * TKC + t];
                o[(size_t)Kout * Cin * 9 + kt * TKC + t] = sum;
            }
        }
    }
}

#undef DY_SLOT
#undef X_SLOT

// second pass: element e of [dW | db] = sum of the slots in ascending slab order, written (not accumulated)
__global__ __launch_bounds__(256) void conv3x3_wgrad_reduce_kernel(const float* __restrict__ ws, int slabs, long slot, long wlen,
                                                                   long total, float* __restrict__ dw, float* __restrict__ db) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float* p = ws + e;
    float sum = 0.f;
    int i = 0;
    for (; i + 4 <= slabs; i += 4) {                              // four loads in flight, added in slab order
        const float a = p[(long)i * slot], b = p[(long)(i + 1) * slot], c = p[(long)(i + 2) * slot], d = p[(long)(i + 3) * slot];
        sum += a; sum += b; sum += c; sum += d;
    }
    for (; i < slabs; ++i) sum += p[(long)i * slot];
    if (e < wlen) dw[e] = sum;
    else db[e - wlen] = sum;
}

// Layout changes between the token layout [B][HW][C] (row stride ld floats) and the channel-blocked layout [B][C/8][HW][8], with the two
// elementwise factors of a ConvBlock (M1:28-40) folded in, so that neither is a pass of its own: towards the blocked layout the
// LeakyReLU derivative (1 or 0.01 by the sign of the saved activation `mask`, blocked) on a gradient; towards tokens the block's
// `+ conv11(x)` (`addend`, tokens).  One thread = 4 channels of one pixel; the token side is read / written in whole rows.
__global__ __launch_bounds__(256) void tokens_to_blocked_kernel(const float* __restrict__ tok, int ld, const float* __restrict__ mask,
                                                                float* __restrict__ blk, int HW, int C, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int C4 = C / 4, q = (int)(e % C4);
    const size_t row = e / C4;
    const size_t b = row / HW, p = row % HW;
    const size_t o = ((b * (C / 8) + (q >> 1)) * HW + p) * 8 + (q & 1) * 4;
    f32x4 v = ld4v(tok + row * ld + 4 * q);
    if (mask) {
        const f32x4 m = ld4v(mask + o);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = m[i] > 0.f ? v[i] : 0.01f * v[i];
    }
    st4v(blk + o, v);
}

__global__ __launch_bounds__(256) void blocked_to_tokens_kernel(const float* __restrict__ blk, const float* __restrict__ addend, int ld_add,
                                                                float* __restrict__ tok, int ld, int HW, int C, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int C4 = C / 4, q = (int)(e % C4);
    const size_t row = e / C4;
    const size_t b = row / HW, p = row % HW;
    f32x4 v = ld4v(blk + ((b * (C / 8) + (q >> 1)) * HW + p) * 8 + (q & 1) * 4);
    if (addend) v += ld4v(addend + row * ld_add + 4 * q);
    st4v(tok + row * ld + 4 * q, v);
}

int wgrad(const char* who, bool any, const float* x, const float* dy, float* dw, float* db, float* ws, size_t ws_bytes, int B, int H, int W,
          int Cin, int Kout, void* stream) {
    DHZ_REQUIRE(x && dy && dw, "%s: null pointer (x=%p dy=%p dw=%p)", who, (const void*)x, (const void*)dy, (void*)dw);
    const Cut c = make_cut(B, H, W, Cin, Kout, any);
    DHZ_REQUIRE(c.ok, "%s: unsupported shape B=%d H=%d W=%d Cin=%d Kout=%d (channels in 32s up to 512; maps %s)", who, B, H, W, Cin, Kout,
                any ? "of H, W >= 1" : "in 16s, or 8 x 8");
    const size_t need = (size_t)c.slabs * (size_t)c.slot * sizeof(float);
    if (dhz_det()) {                                              // the mode's workspace; the kernels are the same
        ws = dhz_det_ws(who, c.slabs, c.slot);
        if (!ws) return DHZ_EINVAL;
    } else {
        DHZ_REQUIRE(ws, "%s: null workspace (%zu bytes needed: dhz_conv3x3_wgrad_workspace_bytes%s)", who, need, any ? "_any" : "");
        DHZ_REQUIRE(ws_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    }
    hipStream_t s = (hipStream_t)stream;
    const int items = c.slabs * c.tiles;
    const int cap = WG_PER_CU * dhz_num_cus();
    const int grid = items < cap ? items : cap;
    if (c.mode == MODE_Q8)
        hipLaunchKernelGGL((conv3x3_wgrad_kernel<MODE_Q8>), dim3(grid), dim3(NTHR), 0, s, x, dy, ws, H, W, Cin, Kout, c.nchunks, c.slabs,
                           c.slot, db != nullptr);
    else if (c.mode == MODE_M16)
        hipLaunchKernelGGL((conv3x3_wgrad_kernel<MODE_M16>), dim3(grid), dim3(NTHR), 0, s, x, dy, ws, H, W, Cin, Kout, c.nchunks, c.slabs,
                           c.slot, db != nullptr);
    else
        hipLaunchKernelGGL((conv3x3_wgrad_kernel<MODE_RAGGED>), dim3(grid), dim3(NTHR), 0, s, x, dy, ws, H, W, Cin, Kout, c.nchunks,
                           c.slabs, c.slot, db != nullptr);
    DHZ_CHECK_LAUNCH(who);
    const long total = c.wlen + (db ? Kout : 0);
    hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws, c.slabs, c.slot, c.wlen,
                       total, dw, db);
    DHZ_CHECK_LAUNCH(any ? "dhz_conv3x3_wgrad_any (reduction)" : "dhz_conv3x3_wgrad (reduction)");
    return DHZ_OK;
}

}  // namespace

extern "C" size_t dhz_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Kout) {
    const Cut c = make_cut(B, H, W, Cin, Kout, false);
    return c.ok ? (size_t)c.slabs * (size_t)c.slot * sizeof(float) : 0;
}
extern "C" size_t dhz_conv3x3_wgrad_workspace_bytes_any(int B, int H, int W, int Cin, int Kout) {
    const Cut c = make_cut(B, H, W, Cin, Kout, true);
    return c.ok ? (size_t)c.slabs * (size_t)c.slot * sizeof(float) : 0;
}

extern "C" int dhz_conv3x3_wgrad_parts(int B, int H, int W, int Cin, int Kout) {
    const Cut c = make_cut(B, H, W, Cin, Kout, false);
    return c.ok ? c.slabs : 0;
}
extern "C" int dhz_conv3x3_wgrad_parts_any(int B, int H, int W, int Cin, int Kout) {
    const Cut c = make_cut(B, H, W, Cin, Kout, true);
    return c.ok ? c.slabs : 0;
}

extern "C" int dhz_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, size_t ws_bytes, int B, int H,
                                 int W, int Cin, int Kout, void* stream) {
    return wgrad("dhz_conv3x3_wgrad", false, x, dy, dw, db, ws, ws_bytes, B, H, W, Cin, Kout, stream);
}
extern "C" int dhz_conv3x3_wgrad_any(const float* x, const float* dy, float* dw, float* db, float* ws, size_t ws_bytes, int B, int H,
                                     int W, int Cin, int Kout, void* stream) {
    return wgrad("dhz_conv3x3_wgrad_any", true, x, dy, dw, db, ws, ws_bytes, B, H, W, Cin, Kout, stream);
}

extern "C" int dhz_tokens_to_blocked8(const float* tok, int ld, const float* leaky_mask, float* blk, int B, int HW, int C, void* stream) {
    DHZ_REQUIRE(tok && blk, "dhz_tokens_to_blocked8: null pointer");
    DHZ_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 4 == 0, "dhz_tokens_to_blocked8: B=%d HW=%d C=%d ld=%d", B, HW, C, ld);
    DHZ_REQUIRE((((uintptr_t)tok | (uintptr_t)blk | (uintptr_t)leaky_mask) & 15) == 0, "dhz_tokens_to_blocked8: pointers must be 16-byte aligned");
    const size_t total = (size_t)B * HW * (C / 4);
    hipLaunchKernelGGL(tokens_to_blocked_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok, ld,
                       leaky_mask, blk, HW, C, total);
    DHZ_CHECK_LAUNCH("dhz_tokens_to_blocked8");
    return DHZ_OK;
}

extern "C" int dhz_blocked8_to_tokens(const float* blk, const float* addend, int ld_add, float* tok, int ld, int B, int HW, int C,
                                      void* stream) {
    DHZ_REQUIRE(tok && blk, "dhz_blocked8_to_tokens: null pointer");
    DHZ_REQUIRE(B > 0 && HW > 0 && C > 0 && C % 8 == 0 && ld >= C && ld % 4 == 0 && (!addend || (ld_add >= C && ld_add % 4 == 0)),
                "dhz_blocked8_to_tokens: B=%d HW=%d C=%d ld=%d ld_add=%d", B, HW, C, ld, ld_add);
    DHZ_REQUIRE((((uintptr_t)tok | (uintptr_t)blk | (uintptr_t)addend) & 15) == 0, "dhz_blocked8_to_tokens: pointers must be 16-byte aligned");
    const size_t total = (size_t)B * HW * (C / 4);
    hipLaunchKernelGGL(blocked_to_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, blk, addend,
                       ld_add, tok, ld, HW, C, total);
    DHZ_CHECK_LAUNCH("dhz_blocked8_to_tokens");
    return DHZ_OK;
}
