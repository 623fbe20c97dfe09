// F2 - the training feed on the device (dataset.py:17-77, FFA_model/data_utils.py:51-81): for each batch item gather an h x w crop of the uint8 HWC
// image pair held in HBM, apply one of the 8 rotate/flip maps of utils/dataset_utils.py:6-40 and emit float32 CHW in [0,1] (value / 255,
// the same IEEE division load_img performs).  HBM-bound and tiny (2 x n x 3 x h x w floats out); one thread per output pixel, stores
// coalesced along the row.  ONE kernel template, feed_kernel, serves the five crop entries: they differ in where an item's geometry comes
// from (TableGeom / DescGeom) and in whether MixUp's partner item is blended into the same store (My_train.py from epoch 6 on);
// gather_mix_pair_kernel does the latter for float32 tensors that are already resident.
#include <stdint.h>
#include "common.h"

namespace {

struct Norm6 { float mean[3], std[3]; };

// What the kernel needs of one batch item: pixel origin of the crop and row stride in pixels, in gt and in hazy; the map k; MixUp's partner
// item and the bit pattern of its fp32 lam (read only by the MIX instances).
struct Item { long long gt_org, gt_stride, hazy_org, hazy_stride; int k, partner, lam_bits; };

// uint8 [N,Hs,Ws,3] stores, rows of 4 int (id, r, c, k) or, MIX, DHZ_MIX_TABLE_WORDS int (id, r, c, k, partner, lam bits)
struct TableGeom {
    static constexpr bool STORE = true;
    const int* rows;
    int Hs, Ws;
    template <bool MIX>
    __device__ __forceinline__ Item row(int t) const {
        const int* r = rows + (size_t)t * (MIX ? DHZ_MIX_TABLE_WORDS : 4);
        const long long org = ((long long)r[0] * Hs + r[1]) * Ws + r[2];
        return {org, Ws, org, Ws, r[3], MIX ? r[4] : 0, MIX ? r[5] : 0};
    }
};

// byte pools of images that each have their own size, every image HWC at its own offset: rows of DHZ_RAGGED_DESC_WORDS int64 (hazy origin,
// hazy stride, gt origin, gt stride, k) or, MIX, DHZ_RAGGED_MIX_DESC_WORDS (the same, partner, lam bits in the low 32 bits)
struct DescGeom {
    static constexpr bool STORE = false;
    const long long* rows;
    template <bool MIX>
    __device__ __forceinline__ Item row(int t) const {
        const long long* d = rows + (size_t)t * (MIX ? DHZ_RAGGED_MIX_DESC_WORDS : DHZ_RAGGED_DESC_WORDS);
        return {d[2], d[3], d[0], d[1], (int)d[4], MIX ? (int)d[5] : 0, MIX ? (int)d[6] : 0};
    }
};

// MixUp (utils/dataset_utils.py:39-45): lam * a + (1 - lam) * b.  ATen evaluates the formula as four fp32 operations - 1 - lam, two
// products, one sum - so contraction is off here (hipcc contracts to FMA by default, and __fmul_rn / __fadd_rn are plain operators in this
// toolchain's headers): the four operations below are rounded one by one and reproduce ATen bit for bit.
__device__ __forceinline__ float mix_of(float lam, float a, float b) {
#pragma clang fp contract(off)
    const float oml = 1.f - lam;
    const float pa = lam * a;
    const float pb = oml * b;
    return pa + pb;
}

// source position inside an h x w crop (mi = h - 1, mj = w - 1) for output (i, j) under map k; the odd maps exist on square crops only
__device__ __forceinline__ void map_of(int k, int i, int j, int mi, int mj, int& si, int& sj) {
    switch (k) {
        case 0: si = i;      sj = j;      break;    // identity
        case 1: si = mi - j; sj = i;      break;    // rot90(k=1, dims=[-1,-2])
        case 2: si = mi - i; sj = mj - j; break;    // rot90(k=2)
        case 3: si = j;      sj = mj - i; break;    // rot90(k=3)
        case 4: si = mi - i; sj = j;      break;    // flip(-2)
        case 5: si = mi - j; sj = mj - i; break;    // rot90(k=1).flip(-2)
        case 6: si = i;      sj = mj - j; break;    // rot90(k=2).flip(-2)
        default: si = j;     sj = i;      break;    // rot90(k=3).flip(-2)
    }
}

// The three bytes of an item's pixel under output (i, j), in gt and in hazy.  Addresses are formed in 64 bits: a pool may exceed 4 GiB.
struct Pixel { const uint8_t *gt, *hazy; };
__device__ __forceinline__ Pixel pixel_of(const uint8_t* gt, const uint8_t* hazy, const Item& it, int km, int i, int j, int mi, int mj) {
    int si, sj;
    map_of(it.k & km, i, j, mi, mj, si, sj);
    return {gt + (size_t)(it.gt_org + (long long)si * it.gt_stride + sj) * 3,
            hazy + (size_t)(it.hazy_org + (long long)si * it.hazy_stride + sj) * 3};
}

template <bool NORM>
__device__ __forceinline__ float hazy_of(uint8_t byte, const Norm6& nm, int ch) {
    const float v = (float)byte / 255.f;
    return NORM ? (v - nm.mean[ch]) / nm.std[ch] : v;
}

// One block works on one item (blockIdx.x / bpi), so the item's row, its partner's row and both maps are wave-uniform: the rows are read
// once per wave through the constant path, the switch does not diverge and the pixel index needs 32-bit divisions only.  On h != w only
// the four maps that keep the shape exist (k & 6: identity, rot180, the two flips), on h == w all eight.  NORM: the hazy value becomes
// (v - mean) / std, normalised first and mixed second, the order of the two passes it replaces; out_gt is never normalised.
template <typename Geom, bool MIX, bool NORM>
__global__ void __launch_bounds__(256) feed_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ hazy, Geom geom,
                                                   float* __restrict__ out_gt, float* __restrict__ out_hazy, Norm6 nm, int bpi, int h, int w) {
    const unsigned item = blockIdx.x / (unsigned)bpi;
    const unsigned at = (blockIdx.x - item * (unsigned)bpi) * 256u + threadIdx.x;
    const int per = h * w;
    if (at >= (unsigned)per) return;
    const Item a = geom.template row<MIX>((int)item);      // (before the division below: the compiler then issues the row's loads ahead of it)
    const int pix = (int)at, i = pix / w, j = pix - i * w, mi = h - 1, mj = w - 1, km = h == w ? 7 : 6;
    const Pixel pa = pixel_of(gt, hazy, a, km, i, j, mi, mj);
    Pixel pb = pa;
    if (MIX) pb = pixel_of(gt, hazy, geom.template row<MIX>(a.partner), km, i, j, mi, mj);       // (0 <= partner < n: the caller's promise)
    const float lam = __int_as_float(a.lam_bits);
    const size_t dst = (size_t)item * 3 * (size_t)per + (size_t)pix;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float g = (float)pa.gt[ch] / 255.f, v = hazy_of<NORM>(pa.hazy[ch], nm, ch);
        out_gt[dst + (size_t)ch * per] = MIX ? mix_of(lam, g, (float)pb.gt[ch] / 255.f) : g;
        out_hazy[dst + (size_t)ch * per] = MIX ? mix_of(lam, v, hazy_of<NORM>(pb.hazy[ch], nm, ch)) : v;
    }
}

// The host side of the five crop entries: refusals in the entry's name, Norm6 from the host pointer, the instance, the launch.  Only the
// instances an entry reaches exist: the table entries take no normalisation.
template <typename Geom>
int launch_feed(const char* entry, const uint8_t* gt, const uint8_t* hazy, Geom geom, float* out_gt, float* out_hazy, const float* norm,
                bool mix, int n, int h, int w, void* stream) {
    DHZ_REQUIRE(gt && hazy && geom.rows && out_gt && out_hazy, "%s: null pointer", entry);
    if constexpr (Geom::STORE)                      // the crop must fit the Hs x Ws store; a pool's entry cannot see the images' sizes
        DHZ_REQUIRE(n > 0 && h > 0 && w > 0 && h <= geom.Hs && w <= geom.Ws, "%s: bad sizes n=%d h=%d w=%d H=%d W=%d", entry, n, h, w, geom.Hs,
                    geom.Ws);
    else
        DHZ_REQUIRE(n > 0 && h > 0 && w > 0, "%s: bad sizes n=%d h=%d w=%d", entry, n, h, w);
    DHZ_REQUIRE((long long)n * h * w < (1ll << 31), "%s: batch too large n=%d h=%d w=%d", entry, n, h, w);
    const int bpi = (int)(((long long)h * w + 255) / 256);          // blocks per item
    DHZ_REQUIRE((long long)n * bpi < (1ll << 31), "%s: batch too large n=%d h=%d w=%d", entry, n, h, w);
    constexpr bool NORMS = !Geom::STORE;
    Norm6 nm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    if (NORMS && norm)
        for (int ch = 0; ch < 3; ++ch) { nm.mean[ch] = norm[ch]; nm.std[ch] = norm[3 + ch]; }
    const auto kernel = NORMS && norm ? (mix ? feed_kernel<Geom, true, NORMS> : feed_kernel<Geom, false, NORMS>)
                                      : (mix ? feed_kernel<Geom, true, false> : feed_kernel<Geom, false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)n * bpi)), dim3(256), 0, (hipStream_t)stream, gt, hazy, geom, out_gt, out_hazy, nm,
                       bpi, h, w);
    DHZ_CHECK_LAUNCH(entry);
    return DHZ_OK;
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

extern "C" int dhz_crop_augment_pair(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt,
                                     float* out_hazy, int n, int Hs, int Ws, int ps, void* stream) {
    return launch_feed("dhz_crop_augment_pair", gt, hazy, TableGeom{table, Hs, Ws}, out_gt, out_hazy, nullptr, false, n, ps, ps, stream);
}

extern "C" int dhz_crop_augment_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                                          int n, int Hs, int Ws, int h, int w, void* stream) {
    return launch_feed("dhz_crop_augment_pair_rect", gt, hazy, TableGeom{table, Hs, Ws}, out_gt, out_hazy, nullptr, false, n, h, w, stream);
}

extern "C" int dhz_crop_augment_mix_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                                              int n, int Hs, int Ws, int h, int w, void* stream) {
    return launch_feed("dhz_crop_augment_mix_pair_rect", gt, hazy, TableGeom{table, Hs, Ws}, out_gt, out_hazy, nullptr, true, n, h, w, stream);
}

extern "C" int dhz_crop_augment_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt,
                                            float* out_hazy, const float* norm, int n, int h, int w, void* stream) {
    return launch_feed("dhz_crop_augment_pair_ragged", gt_pool, hazy_pool, DescGeom{(const long long*)desc}, out_gt, out_hazy, norm, false,
                       n, h, w, stream);
}

extern "C" int dhz_crop_augment_mix_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt,
                                                float* out_hazy, const float* norm, int n, int h, int w, void* stream) {
    return launch_feed("dhz_crop_augment_mix_pair_ragged", gt_pool, hazy_pool, DescGeom{(const long long*)desc}, out_gt, out_hazy, norm, true,
                       n, h, w, stream);
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
