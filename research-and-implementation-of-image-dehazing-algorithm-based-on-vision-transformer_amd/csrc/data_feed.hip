// F2 - the training feed of dataset.py:17-77 on the device: for each batch item (patch id, r, c, augmentation k) gather the
// ps x ps crop of the uint8 HWC patch pair held in HBM, apply one of the 8 rotate/flip maps of
// utils/dataset_utils.py:6-40 and emit float32 CHW in [0,1] (value / 255, the same IEEE division load_img performs).
// HBM-bound and tiny (2 x n x 3 x ps^2 floats out); one thread per output pixel, stores coalesced along the row.
// The *_mix_* kernels blend MixUp's partner item into the same store (My_train.py from epoch 6 on); gather_mix_pair_kernel does the
// same for float32 tensors that are already resident.
#include <stdint.h>
#include "common.h"

namespace {

__global__ void crop_augment_pair_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy,
                                         const int* __restrict__ table, float* __restrict__ out_gt,
                                         float* __restrict__ out_hazy, int n, int Hs, int Ws, int ps) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)ps * ps;
    if (e >= (size_t)n * per) return;
    const int item = (int)(e / per);
    const int pix = (int)(e % per);
    const int i = pix / ps, j = pix % ps, m = ps - 1;
    const int id = table[item * 4 + 0], r = table[item * 4 + 1], c = table[item * 4 + 2], k = table[item * 4 + 3] & 7;
    int si, sj;                                     // source position inside the crop for output (i, j)
    switch (k) {
        case 0: si = i;     sj = j;     break;      // identity
        case 1: si = m - j; sj = i;     break;      // rot90(k=1, dims=[-1,-2])
        case 2: si = m - i; sj = m - j; break;      // rot90(k=2)
        case 3: si = j;     sj = m - i; break;      // rot90(k=3)
        case 4: si = m - i; sj = j;     break;      // flip(-2)
        case 5: si = m - j; sj = m - i; break;      // rot90(k=1).flip(-2)
        case 6: si = i;     sj = m - j; break;      // rot90(k=2).flip(-2)
        default: si = j;    sj = i;     break;      // rot90(k=3).flip(-2)
    }
    const size_t src = (((size_t)id * Hs + r + si) * Ws + c + sj) * 3;
    const size_t dst = (size_t)item * 3 * per + pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out_gt[dst + ch * per] = (float)gt[src + ch] / 255.f;
        out_hazy[dst + ch * per] = (float)hazy[src + ch] / 255.f;
    }
}

// The same feed for an h x w crop (whole images: h = Hs, w = Ws).  On h != w only the four maps that keep the shape exist - identity,
// rot180, the two flips: k & 6 -; on h == w all eight, position for position the kernel above.
__global__ void crop_augment_pair_rect_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy,
                                              const int* __restrict__ table, float* __restrict__ out_gt,
                                              float* __restrict__ out_hazy, int n, int Hs, int Ws, int h, int w) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)h * w;
    if (e >= (size_t)n * per) return;
    const int item = (int)(e / per);
    const int pix = (int)(e % per);
    const int i = pix / w, j = pix % w, mi = h - 1, mj = w - 1;
    const int id = table[item * 4 + 0], r = table[item * 4 + 1], c = table[item * 4 + 2];
    const int k = table[item * 4 + 3] & (h == w ? 7 : 6);
    int si, sj;                                     // source position inside the crop for output (i, j)
    switch (k) {
        case 0: si = i;      sj = j;      break;    // identity
        case 1: si = mi - j; sj = i;      break;    // rot90(k=1, dims=[-1,-2])        (square crops only, mi == mj)
        case 2: si = mi - i; sj = mj - j; break;    // rot90(k=2)
        case 3: si = j;      sj = mj - i; break;    // rot90(k=3)                      (square)
        case 4: si = mi - i; sj = j;      break;    // flip(-2)
        case 5: si = mi - j; sj = mj - i; break;    // rot90(k=1).flip(-2)             (square)
        case 6: si = i;      sj = mj - j; break;    // rot90(k=2).flip(-2)
        default: si = j;     sj = i;      break;    // rot90(k=3).flip(-2)             (square)
    }
    const size_t src = (((size_t)id * Hs + r + si) * Ws + c + sj) * 3;
    const size_t dst = (size_t)item * 3 * per + pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out_gt[dst + ch * per] = (float)gt[src + ch] / 255.f;
        out_hazy[dst + ch * per] = (float)hazy[src + ch] / 255.f;
    }
}

// The feed of FFA_model/data_utils.py:51-81 for images that each have their own size (RESIDE, I-HAZE, O-HAZE): the two stores are byte pools,
// every image HWC at its own offset, and the geometry comes per item from desc instead of per launch.  One block works on one item
// (blockIdx.x / bpi), so the descriptor row and the map k are wave-uniform: the row is read once per wave through the constant path and
// the switch does not diverge; the pixel index needs 32-bit divisions only.  Loads and stores per pixel are those of the rect kernel.
struct Norm6 { float mean[3], std[3]; };

template <bool NORM>
__global__ void __launch_bounds__(256) crop_augment_pair_ragged_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy,
                                                                       const long long* __restrict__ desc, float* __restrict__ out_gt,
                                                                       float* __restrict__ out_hazy, Norm6 nm, int bpi, int h, int w) {
    const int item = (int)(blockIdx.x / (unsigned)bpi);
    const int pix = (int)(blockIdx.x - (unsigned)item * (unsigned)bpi) * 256 + (int)threadIdx.x;
    const int per = h * w;
    if (pix >= per) return;
    const long long* d = desc + (size_t)item * DHZ_RAGGED_DESC_WORDS;
    const long long hazy_org = d[0], hazy_stride = d[1], gt_org = d[2], gt_stride = d[3];
    const int k = (int)d[4] & (h == w ? 7 : 6);
    const int i = pix / w, j = pix - i * w, mi = h - 1, mj = w - 1;
    int si, sj;                                     // source position inside the crop for output (i, j): the rect kernel's table
    switch (k) {
        case 0: si = i;      sj = j;      break;
        case 1: si = mi - j; sj = i;      break;
        case 2: si = mi - i; sj = mj - j; break;
        case 3: si = j;      sj = mj - i; break;
        case 4: si = mi - i; sj = j;      break;
        case 5: si = mi - j; sj = mj - i; break;
        case 6: si = i;      sj = mj - j; break;
        default: si = j;     sj = i;      break;
    }
    const uint8_t* pg = gt + (size_t)(gt_org + (long long)si * gt_stride + sj) * 3;
    const uint8_t* ph = hazy + (size_t)(hazy_org + (long long)si * hazy_stride + sj) * 3;
    const size_t dst = (size_t)item * 3 * (size_t)per + (size_t)pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out_gt[dst + (size_t)ch * per] = (float)pg[ch] / 255.f;
        const float v = (float)ph[ch] / 255.f;
        out_hazy[dst + (size_t)ch * per] = NORM ? (v - nm.mean[ch]) / nm.std[ch] : v;
    }
}

// ---- MixUp (utils/dataset_utils.py:39-45) inside the feed: out[t] = lam[t] * A[t] + (1 - lam[t]) * A[partner[t]], A[.] what the kernels
// above write.  partner and the bit pattern of lam ride in the table rows.  ATen evaluates the formula as four fp32 operations - 1 - lam,
// two products, one sum - so contraction is off in mix_of (hipcc contracts to FMA by default, and __fmul_rn / __fadd_rn are plain
// operators in this toolchain's headers): the four operations below are rounded one by one and reproduce ATen bit for bit.
__device__ __forceinline__ float mix_of(float lam, float a, float b) {
#pragma clang fp contract(off)
    const float oml = 1.f - lam;
    const float pa = lam * a;
    const float pb = oml * b;
    return pa + pb;
}

// source position inside an h x w crop for output (i, j) under map k: the table of crop_augment_pair_rect_kernel
__device__ __forceinline__ void map_of(int k, int i, int j, int mi, int mj, int& si, int& sj) {
    switch (k) {
        case 0: si = i;      sj = j;      break;
        case 1: si = mi - j; sj = i;      break;
        case 2: si = mi - i; sj = mj - j; break;
        case 3: si = j;      sj = mj - i; break;
        case 4: si = mi - i; sj = j;      break;
        case 5: si = mi - j; sj = mj - i; break;
        case 6: si = i;      sj = mj - j; break;
        default: si = j;     sj = i;      break;
    }
}

// crop_augment_pair_rect_kernel with a second crop blended into the same store: six more byte loads per pixel, no extra pass
__global__ void crop_augment_mix_pair_rect_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy,
                                                  const int* __restrict__ table, float* __restrict__ out_gt,
                                                  float* __restrict__ out_hazy, int n, int Hs, int Ws, int h, int w) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)h * w;
    if (e >= (size_t)n * per) return;
    const int item = (int)(e / per);
    const int pix = (int)(e % per);
    const int i = pix / w, j = pix % w, mi = h - 1, mj = w - 1, km = h == w ? 7 : 6;
    const int* ta = table + item * DHZ_MIX_TABLE_WORDS;
    const int* tb = table + ta[4] * DHZ_MIX_TABLE_WORDS;          // the partner's row (0 <= partner < n: the caller's promise)
    const float lam = __int_as_float(ta[5]);
    int si, sj;
    map_of(ta[3] & km, i, j, mi, mj, si, sj);
    const size_t sa = (((size_t)ta[0] * Hs + ta[1] + si) * Ws + ta[2] + sj) * 3;
    map_of(tb[3] & km, i, j, mi, mj, si, sj);
    const size_t sb = (((size_t)tb[0] * Hs + tb[1] + si) * Ws + tb[2] + sj) * 3;
    const size_t dst = (size_t)item * 3 * per + pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out_gt[dst + ch * per] = mix_of(lam, (float)gt[sa + ch] / 255.f, (float)gt[sb + ch] / 255.f);
        out_hazy[dst + ch * per] = mix_of(lam, (float)hazy[sa + ch] / 255.f, (float)hazy[sb + ch] / 255.f);
    }
}

// crop_augment_pair_ragged_kernel with the partner's crop blended in.  One block per item still, so both descriptor rows - the item's
// and its partner's - and both maps are wave-uniform.  The hazy value is normalised first and mixed second, the order of the two passes.
template <bool NORM>
__global__ void __launch_bounds__(256) crop_augment_mix_pair_ragged_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy,
                                                                           const long long* __restrict__ desc, float* __restrict__ out_gt,
                                                                           float* __restrict__ out_hazy, Norm6 nm, int bpi, int h, int w) {
    const int item = (int)(blockIdx.x / (unsigned)bpi);
    const int pix = (int)(blockIdx.x - (unsigned)item * (unsigned)bpi) * 256 + (int)threadIdx.x;
    const int per = h * w;
    if (pix >= per) return;
    const long long* da = desc + (size_t)item * DHZ_RAGGED_MIX_DESC_WORDS;
    const long long* db = desc + (size_t)da[5] * DHZ_RAGGED_MIX_DESC_WORDS;          // the partner's row
    const float lam = __int_as_float((int)da[6]);                                      // (the low 32 bits)
    const int i = pix / w, j = pix - i * w, mi = h - 1, mj = w - 1, km = h == w ? 7 : 6;
    int si, sj;
    map_of((int)da[4] & km, i, j, mi, mj, si, sj);
    const uint8_t* pha = hazy + (size_t)(da[0] + (long long)si * da[1] + sj) * 3;
    const uint8_t* pga = gt + (size_t)(da[2] + (long long)si * da[3] + sj) * 3;
    map_of((int)db[4] & km, i, j, mi, mj, si, sj);
    const uint8_t* phb = hazy + (size_t)(db[0] + (long long)si * db[1] + sj) * 3;
    const uint8_t* pgb = gt + (size_t)(db[2] + (long long)si * db[3] + sj) * 3;
    const size_t dst = (size_t)item * 3 * (size_t)per + (size_t)pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        out_gt[dst + (size_t)ch * per] = mix_of(lam, (float)pga[ch] / 255.f, (float)pgb[ch] / 255.f);
        const float va = (float)pha[ch] / 255.f, vb = (float)phb[ch] / 255.f;
        out_hazy[dst + (size_t)ch * per] = NORM ? mix_of(lam, (va - nm.mean[ch]) / nm.std[ch], (vb - nm.mean[ch]) / nm.std[ch])
                                                : mix_of(lam, va, vb);
    }
}

// Resident fp32 tensors [N, per_item]: out[t] = src[sel[t]], or with MIX lam * src[sel[t]] + (1 - lam) * src[sel[partner[t]]], for the
// clear and the hazy tensor in one launch.  One block works on one item (rows wave-uniform); V = float4 where per_item % 4 == 0 and the
// four pointers are 16-byte aligned, else float.  `count` = per_item in units of V.
template <typename V, bool MIX>
__global__ void __launch_bounds__(256) gather_mix_pair_kernel(const V* __restrict__ gt, const V* __restrict__ hazy,
                                                              const long long* __restrict__ table, V* __restrict__ out_gt,
                                                              V* __restrict__ out_hazy, int bpi, long long count) {
    const int item = (int)(blockIdx.x / (unsigned)bpi);
    const long long at = (long long)(blockIdx.x - (unsigned)item * (unsigned)bpi) * 256 + threadIdx.x;
    if (at >= count) return;
    const long long* ta = table + (size_t)item * DHZ_GATHER_MIX_TABLE_WORDS;
    const size_t sa = (size_t)ta[0] * (size_t)count + (size_t)at, dst = (size_t)item * (size_t)count + (size_t)at;
    if (!MIX) {
        out_gt[dst] = gt[sa];
        out_hazy[dst] = hazy[sa];
        return;
    }
    const size_t sb = (size_t)table[(size_t)ta[1] * DHZ_GATHER_MIX_TABLE_WORDS] * (size_t)count + (size_t)at;
    const float lam = __int_as_float((int)ta[2]);
    const V ga = gt[sa], gb = gt[sb], ha = hazy[sa], hb = hazy[sb];
    V og, oh;
    if constexpr (sizeof(V) == 16) {
        og = make_float4(mix_of(lam, ga.x, gb.x), mix_of(lam, ga.y, gb.y), mix_of(lam, ga.z, gb.z), mix_of(lam, ga.w, gb.w));
        oh = make_float4(mix_of(lam, ha.x, hb.x), mix_of(lam, ha.y, hb.y), mix_of(lam, ha.z, hb.z), mix_of(lam, ha.w, hb.w));
    } else {
        og = mix_of(lam, ga, gb);
        oh = mix_of(lam, ha, hb);
    }
    out_gt[dst] = og;
    out_hazy[dst] = oh;
}

template <typename V>
void launch_gather_mix(const float* gt, const float* hazy, const int64_t* table, float* out_gt, float* out_hazy, int n, int bpi,
                       long long count, int mix, hipStream_t stream) {
    const dim3 grid((unsigned)((long long)n * bpi));
    if (mix)
        hipLaunchKernelGGL((gather_mix_pair_kernel<V, true>), grid, dim3(256), 0, stream, (const V*)gt, (const V*)hazy,
                           (const long long*)table, (V*)out_gt, (V*)out_hazy, bpi, count);
    else
        hipLaunchKernelGGL((gather_mix_pair_kernel<V, false>), grid, dim3(256), 0, stream, (const V*)gt, (const V*)hazy,
                           (const long long*)table, (V*)out_gt, (V*)out_hazy, bpi, count);
}

}  // namespace

extern "C" int dhz_crop_augment_mix_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                                              int n, int Hs, int Ws, int h, int w, void* stream) {
    DHZ_REQUIRE(gt && hazy && table && out_gt && out_hazy, "dhz_crop_augment_mix_pair_rect: null pointer");
    DHZ_REQUIRE(n > 0 && h > 0 && w > 0 && h <= Hs && w <= Ws, "dhz_crop_augment_mix_pair_rect: bad sizes n=%d h=%d w=%d H=%d W=%d", n, h, w, Hs, Ws);
    DHZ_REQUIRE((long long)n * h * w < (1ll << 31), "dhz_crop_augment_mix_pair_rect: batch too large n=%d h=%d w=%d", n, h, w);
    const size_t total = (size_t)n * h * w;
    hipLaunchKernelGGL(crop_augment_mix_pair_rect_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt,
                       hazy, table, out_gt, out_hazy, n, Hs, Ws, h, w);
    DHZ_CHECK_LAUNCH("dhz_crop_augment_mix_pair_rect");
    return DHZ_OK;
}

extern "C" int dhz_crop_augment_mix_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt,
                                                float* out_hazy, const float* norm, int n, int h, int w, void* stream) {
    DHZ_REQUIRE(gt_pool && hazy_pool && desc && out_gt && out_hazy, "dhz_crop_augment_mix_pair_ragged: null pointer");
    DHZ_REQUIRE(n > 0 && h > 0 && w > 0, "dhz_crop_augment_mix_pair_ragged: bad sizes n=%d h=%d w=%d", n, h, w);
    DHZ_REQUIRE((long long)n * h * w < (1ll << 31), "dhz_crop_augment_mix_pair_ragged: batch too large n=%d h=%d w=%d", n, h, w);
    const int bpi = (h * w + 255) / 256;            // blocks per item
    DHZ_REQUIRE((long long)n * bpi < (1ll << 31), "dhz_crop_augment_mix_pair_ragged: batch too large n=%d h=%d w=%d", n, h, w);
    const dim3 grid((unsigned)((long long)n * bpi));
    Norm6 nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    if (norm) {
        for (int ch = 0; ch < 3; ++ch) { nm.mean[ch] = norm[ch]; nm.std[ch] = norm[3 + ch]; }
        hipLaunchKernelGGL(crop_augment_mix_pair_ragged_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, gt_pool, hazy_pool,
                           (const long long*)desc, out_gt, out_hazy, nm, bpi, h, w);
    } else {
        hipLaunchKernelGGL(crop_augment_mix_pair_ragged_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, gt_pool, hazy_pool,
                           (const long long*)desc, out_gt, out_hazy, nm, bpi, h, w);
    }
    DHZ_CHECK_LAUNCH("dhz_crop_augment_mix_pair_ragged");
    return DHZ_OK;
}

extern "C" int dhz_gather_mix_pair(const float* gt, const float* hazy, const int64_t* table, float* out_gt, float* out_hazy, int n,
                                   int64_t per_item, int mix, void* stream) {
    DHZ_REQUIRE(gt && hazy && table && out_gt && out_hazy, "dhz_gather_mix_pair: null pointer");
    DHZ_REQUIRE(n > 0 && per_item > 0, "dhz_gather_mix_pair: bad sizes n=%d per_item=%lld", n, (long long)per_item);
    DHZ_REQUIRE((long long)n * per_item < (1ll << 31), "dhz_gather_mix_pair: batch too large n=%d per_item=%lld", n, (long long)per_item);
    const bool vec = per_item % 4 == 0 && (((uintptr_t)gt | (uintptr_t)hazy | (uintptr_t)out_gt | (uintptr_t)out_hazy) & 15) == 0;
    const long long count = vec ? per_item / 4 : per_item;
    const int bpi = (int)((count + 255) / 256);     // blocks per item
    if (vec)
        launch_gather_mix<float4>(gt, hazy, table, out_gt, out_hazy, n, bpi, count, mix, (hipStream_t)stream);
    else
        launch_gather_mix<float>(gt, hazy, table, out_gt, out_hazy, n, bpi, count, mix, (hipStream_t)stream);
    DHZ_CHECK_LAUNCH("dhz_gather_mix_pair");
    return DHZ_OK;
}

extern "C" int dhz_crop_augment_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt,
                                            float* out_hazy, const float* norm, int n, int h, int w, void* stream) {
    DHZ_REQUIRE(gt_pool && hazy_pool && desc && out_gt && out_hazy, "dhz_crop_augment_pair_ragged: null pointer");
    DHZ_REQUIRE(n > 0 && h > 0 && w > 0, "dhz_crop_augment_pair_ragged: bad sizes n=%d h=%d w=%d", n, h, w);
    DHZ_REQUIRE((long long)n * h * w < (1ll << 31), "dhz_crop_augment_pair_ragged: batch too large n=%d h=%d w=%d", n, h, w);
    const int bpi = (h * w + 255) / 256;            // blocks per item
    DHZ_REQUIRE((long long)n * bpi < (1ll << 31), "dhz_crop_augment_pair_ragged: batch too large n=%d h=%d w=%d", n, h, w);
    const dim3 grid((unsigned)((long long)n * bpi));
    Norm6 nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    if (norm) {
        for (int ch = 0; ch < 3; ++ch) { nm.mean[ch] = norm[ch]; nm.std[ch] = norm[3 + ch]; }
        hipLaunchKernelGGL(crop_augment_pair_ragged_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, gt_pool, hazy_pool,
                           (const long long*)desc, out_gt, out_hazy, nm, bpi, h, w);
    } else {
        hipLaunchKernelGGL(crop_augment_pair_ragged_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, gt_pool, hazy_pool,
                           (const long long*)desc, out_gt, out_hazy, nm, bpi, h, w);
    }
    DHZ_CHECK_LAUNCH("dhz_crop_augment_pair_ragged");
    return DHZ_OK;
}

extern "C" int dhz_crop_augment_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                                          int n, int Hs, int Ws, int h, int w, void* stream) {
    DHZ_REQUIRE(gt && hazy && table && out_gt && out_hazy, "dhz_crop_augment_pair_rect: null pointer");
    DHZ_REQUIRE(n > 0 && h > 0 && w > 0 && h <= Hs && w <= Ws, "dhz_crop_augment_pair_rect: bad sizes n=%d h=%d w=%d H=%d W=%d", n, h, w, Hs, Ws);
    DHZ_REQUIRE((long long)n * h * w < (1ll << 31), "dhz_crop_augment_pair_rect: batch too large n=%d h=%d w=%d", n, h, w);
    const size_t total = (size_t)n * h * w;
    hipLaunchKernelGGL(crop_augment_pair_rect_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt,
                       hazy, table, out_gt, out_hazy, n, Hs, Ws, h, w);
    DHZ_CHECK_LAUNCH("dhz_crop_augment_pair_rect");
    return DHZ_OK;
}

extern "C" int dhz_crop_augment_pair(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt,
                                     float* out_hazy, int n, int Hs, int Ws, int ps, void* stream) {
    DHZ_REQUIRE(gt && hazy && table && out_gt && out_hazy, "dhz_crop_augment_pair: null pointer");
    DHZ_REQUIRE(n > 0 && ps > 0 && ps <= Hs && ps <= Ws, "dhz_crop_augment_pair: bad sizes n=%d ps=%d H=%d W=%d", n, ps, Hs, Ws);
    const size_t total = (size_t)n * ps * ps;
    hipLaunchKernelGGL(crop_augment_pair_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt,
                       hazy, table, out_gt, out_hazy, n, Hs, Ws, ps);
    DHZ_CHECK_LAUNCH("dhz_crop_augment_pair");
    return DHZ_OK;
}
