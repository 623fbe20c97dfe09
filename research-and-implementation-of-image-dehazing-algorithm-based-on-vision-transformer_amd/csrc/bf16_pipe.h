// The bf16 matrix pipe and LDS-DMA primitives of the gfx950 kernels, one definition each: v_mfma_f32_16x16x32_bf16 wrappers, the fp32 ->
// bf16-piece splits of the six-term product, the 16-byte global -> LDS DMA request, the LDS image swizzles and transpose reads, and the
// small wave-level helpers the attention kernels share.
//
// Six-term arithmetic (csrc/split6_gemm.hip): an fp32 value is cut by TRUNCATION into three bf16 pieces (a bf16 is
// the top 16 bits of the fp32 pattern, so each piece takes the next eight significant bits of what is left: hi + mid + lo == x exactly,
// x - hi and r - mid are exact); a product is hh + (hm + mh) + (hl + lh + mm), small terms first.
//
// Where a helper exists in two textual forms, hipcc compiles the two to different code (other scheduling and register allocation of the
// kernels around them): both are kept, under distinct names, with the instruction form each one yields and its users.
#pragma once
#include "common.h"

typedef __bf16 dhz_bf16x8 __attribute__((ext_vector_type(8)));
typedef short dhz_s16x4 __attribute__((ext_vector_type(4)));
typedef short dhz_s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t dhz_u32x4 __attribute__((ext_vector_type(4)));
typedef float dhz_f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void dhz_lds_void;
typedef const __attribute__((address_space(1))) void dhz_glb_void;

// v_mfma_f32_16x16x32_bf16: D[16x16] += A[16x32] . B[32x16].  Lane (i = lane & 15, g = lane >> 4) holds the 8 bf16 k = 8 g .. 8 g + 7 of
// row (A) / column (B) i; acc[j] = D[4 g + j][i].  Operands as eight shorts (fragments read from LDS) or as four packed pairs (split output).
__device__ __forceinline__ f32x4 dhz_mfma_bf16(dhz_s16x8 a, dhz_s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dhz_bf16x8, a), __builtin_bit_cast(dhz_bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 dhz_mfma_bf16(dhz_u32x4 a, dhz_u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dhz_bf16x8, a), __builtin_bit_cast(dhz_bf16x8, b), c, 0, 0, 0);
}

// global_load_lds_dwordx4: 16 bytes per lane, global -> LDS with no VGPR, no VALU and no ds_write.  The LDS address is wave-uniform (M0) +
// 16 * lane, the global address is per lane (a bank swizzle is carried by the per-lane SOURCE address).
__device__ __forceinline__ void dhz_dma16(const float* g, float* l) {
    __builtin_amdgcn_global_load_lds((dhz_glb_void*)g, (dhz_lds_void*)l, 16, 0, 0);
}
__device__ __forceinline__ void dhz_dma16(const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((dhz_glb_void*)g, (dhz_lds_void*)l, 16, 0, 0);
}

// ---- fp32 -> bf16 pieces
__device__ __forceinline__ uint32_t dhz_pack_top(float x1, float x0) {              // (x1 & 0xffff0000) | (x0 >> 16): one v_perm_b32
    return __builtin_amdgcn_perm(__float_as_uint(x1), __float_as_uint(x0), 0x07060302u);
}
// Between two bf16 MFMAs of a wave the first two plain vector instructions cost nothing and further ones 4 cycles each, a PACKED fp32
// instruction 7 - 17 cycles of matrix-pipe time (tools/ubench/interleave.hip).  Loops that multiply on the bf16 matrix pipe while they
// split therefore issue their fp32 arithmetic per lane, through inline asm (left as C, hipcc's SLP vectoriser re-packs it).
__device__ __forceinline__ float dhz_sub_np(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float dhz_mul_np(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// two fp32 values -> one packed pair per piece
__device__ __forceinline__ void dhz_split2x3(float x0, float x1, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    const float r0 = x0 - __uint_as_float(__float_as_uint(x0) & 0xffff0000u), r1 = x1 - __uint_as_float(__float_as_uint(x1) & 0xffff0000u);
    const float q0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), q1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    hi = dhz_pack_top(x1, x0);
    mid = dhz_pack_top(r1, r0);
    lo = dhz_pack_top(q1, q0);
}
// Eight fp32 values (a lane's 8 consecutive k) -> the three MFMA operands, four forms:
// dhz_split8x3, array form: plain C subtractions, the compiler packs them where it likes (csrc/leff_fused.hip, csrc/leff_dwconv_dz.hip)
__device__ __forceinline__ void dhz_split8x3(const f32x4 a, const f32x4 b, dhz_u32x4& hi, dhz_u32x4& mid, dhz_u32x4& lo) {
    uint32_t h[4], m[4], l[4];
    dhz_split2x3(a[0], a[1], h[0], m[0], l[0]);
    dhz_split2x3(a[2], a[3], h[1], m[1], l[1]);
    dhz_split2x3(b[0], b[1], h[2], m[2], l[2]);
    dhz_split2x3(b[2], b[3], h[3], m[3], l[3]);
    hi = dhz_u32x4{h[0], h[1], h[2], h[3]};
    mid = dhz_u32x4{m[0], m[1], m[2], m[3]};
    lo = dhz_u32x4{l[0], l[1], l[2], l[3]};
}
// dhz_split8x3, pointer form: the same C arithmetic on eight values that already lie in an array (csrc/fused_attn.hip)
__device__ __forceinline__ void dhz_split8x3(const float* x, dhz_u32x4& hi, dhz_u32x4& mid, dhz_u32x4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x0 = x[2 * i], x1 = x[2 * i + 1];
        const float r0 = x0 - __uint_as_float(__float_as_uint(x0) & 0xffff0000u), r1 = x1 - __uint_as_float(__float_as_uint(x1) & 0xffff0000u);
        const float q0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), q1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
        hi[i] = dhz_pack_top(x1, x0);
        mid[i] = dhz_pack_top(r1, r0);
        lo[i] = dhz_pack_top(q1, q0);
    }
}
// dhz_split8x3_pk: one PACKED subtraction (v_pk_add_f32) per level and pair - two masks, one subtraction per level, one v_perm_b32 per
// piece: 4.5 VALU instructions per element.  For splits outside an MFMA stream (csrc/linear_split.hip)
__device__ __forceinline__ dhz_f32x2 dhz_top16(dhz_f32x2 v) {
    return dhz_f32x2{__uint_as_float(__float_as_uint(v[0]) & 0xffff0000u), __uint_as_float(__float_as_uint(v[1]) & 0xffff0000u)};
}
__device__ __forceinline__ void dhz_split8x3_pk(const f32x4 a, const f32x4 b, dhz_u32x4& hi, dhz_u32x4& mid, dhz_u32x4& lo) {
    const dhz_f32x2 x[4] = {{a[0], a[1]}, {a[2], a[3]}, {b[0], b[1]}, {b[2], b[3]}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const dhz_f32x2 r1 = x[i] - dhz_top16(x[i]);
        const dhz_f32x2 r2 = r1 - dhz_top16(r1);
        hi[i] = dhz_pack_top(x[i][1], x[i][0]);
        mid[i] = dhz_pack_top(r1[1], r1[0]);
        lo[i] = dhz_pack_top(r2[1], r2[0]);
    }
}
// dhz_split8x3_np: per-lane v_sub_f32 (dhz_sub_np) - 11 instructions per pair of elements instead of 9, none of them packed.  For splits
// INSIDE an MFMA stream (csrc/split6_gemm.hip, csrc/linear_split.hip)
__device__ __forceinline__ void dhz_split8x3_np(const f32x4 a, const f32x4 b, dhz_u32x4& hi, dhz_u32x4& mid, dhz_u32x4& lo) {
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x0 = x[2 * i], x1 = x[2 * i + 1];
        const float r0 = dhz_sub_np(x0, __uint_as_float(__float_as_uint(x0) & 0xffff0000u)), r1 = dhz_sub_np(x1, __uint_as_float(__float_as_uint(x1) & 0xffff0000u));
        const float q0 = dhz_sub_np(r0, __uint_as_float(__float_as_uint(r0) & 0xffff0000u)), q1 = dhz_sub_np(r1, __uint_as_float(__float_as_uint(r1) & 0xffff0000u));
        hi[i] = dhz_pack_top(x1, x0);
        mid[i] = dhz_pack_top(r1, r0);
        lo[i] = dhz_pack_top(q1, q0);
    }
}
// The two-piece split of the three-term experiment (csrc/linear_split.hip): ROUNDED bf16 heads (v_cvt_pk_bf16_f32) and the rounded bf16 of
// what the heads leave; x = hi + lo + r, |r| <= 2^-17 |x|
__device__ __forceinline__ void dhz_split8(const f32x4 a, const f32x4 b, dhz_u32x4& hi, dhz_u32x4& lo) {
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    uint32_t h[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = f32_to_bf16(x[i]);
        l[i] = f32_to_bf16(x[i] - __uint_as_float(h[i] << 16));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = h[2 * i] | (h[2 * i + 1] << 16);
        lo[i] = l[2 * i] | (l[2 * i + 1] << 16);
    }
}

// ---- LDS images
// 64-byte-row bf16 images ([row][32 k]): byte offset of 16-byte chunk ch (0..3) of row `row`; the four chunks of a row are XOR-ed with
// {0, 2, 3, 1}[(row >> 2) & 3] - a lane group's ds_read_b128 of rows i16, chunk g is conflict-free
__device__ __forceinline__ int dhz_swz64(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
__device__ __forceinline__ int dhz_off64(int row, int ch) { return row * 64 + 16 * (ch ^ dhz_swz64(row)); }
// Contraction-major (transposed) images: [contraction row][F features] bf16.  Byte offset of 16-byte chunk ch of row `row`: F >= 128
// (256 / 512-byte rows) XORs the low four chunk bits with ((row & 3) << 2) | ((row >> 2) & 3), F = 64 (128-byte rows) with
// (row & 2) | ((row & 8) >> 1) -> conflict-free transpose reads
template <int F>
__device__ __forceinline__ int dhz_swz_tr(int row) {
    if (F >= 128) return ((row & 3) << 2) | ((row >> 2) & 3);
    return (row & 2) | ((row & 8) >> 1);
}
template <int F>
__device__ __forceinline__ int dhz_off_tr(int row, int ch) { return row * (2 * F) + 16 * (ch ^ dhz_swz_tr<F>(row)); }
// fragment (8 contraction rows r0 .. r0 + 7 of feature column 16 cb + (lane & 15)) from such an image by the hardware transpose read
// ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group addresses row r0 + q, columns 4 p .. 4 p + 3 of a 4 x 16 block and receives column
// (lane & 15), rows r0 .. r0 + 3
template <int F>
__device__ __forceinline__ dhz_s16x8 dhz_tr_frag(const unsigned char* img, int r0, int cb, int lane) {
    const int m = lane & 15, q = m >> 2, p = m & 3;
    typedef dhz_s16x4 __attribute__((address_space(3))) * lds_ptr;
    const dhz_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + dhz_off_tr<F>(r0 + q, 2 * cb + (p >> 1)) + 8 * (p & 1)));
    const dhz_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(img + dhz_off_tr<F>(r0 + 4 + q, 2 * cb + (p >> 1)) + 8 * (p & 1)));
    return dhz_s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- wave-level helpers
// max / sum over the 8 lanes that share a softmax row (csrc/ps_attn.hip, csrc/fused_attn_bwd.hip)
__device__ __forceinline__ float dhz_row8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    v = fmaxf(v, __shfl_xor(v, 2));
    return fmaxf(v, __shfl_xor(v, 4));
}
__device__ __forceinline__ float dhz_row8_sum(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v + __shfl_xor(v, 4);
}
// phase boundary inside ONE wave (csrc/winograd_conv.hip, csrc/ps_attn16.hip)
__device__ __forceinline__ void dhz_wave_sync() {
    // LDS operations of one wave execute in order; only the compiler must not move accesses across phase boundaries
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
