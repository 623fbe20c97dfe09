// F2 - the training feed of dataset.py:17-77 on the device: for each batch item (patch id, r, c, augmentation k) gather the
// ps x ps crop of the uint8 HWC patch pair held in HBM, apply one of the 8 rotate/flip maps of
// utils/dataset_utils.py:6-40 and emit float32 CHW in [0,1] (value / 255, the same IEEE division load_img performs).
// HBM-bound and tiny (2 x n x 3 x ps^2 floats out); one thread per output pixel, stores coalesced along the row.
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

}  // namespace

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
