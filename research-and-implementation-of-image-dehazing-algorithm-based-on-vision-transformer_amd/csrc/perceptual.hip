// K11d: the squared-error feature taps of FFA-Net's perceptual loss (FFA_model/models/PerceptualLoss.py:24-31: F.mse_loss between the
// VGG16 features of the dehazed image and of the ground truth at relu1_2, relu2_2, relu3_3), and the pooling backward of a map that is
// a tap as well.  Streaming kernels: one float4 per lane and pass, grid-stride; the forward reads two maps, the backward reads two
// and writes one.
#include "common.h"

namespace {

inline int grid_for(int64_t work_items, int cap) {
    int64_t g = (work_items + 255) / 256;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

template <bool DET>          // deterministic mode: the workgroup stores its sum at sum[blockIdx.x] (the workspace)
__global__ __launch_bounds__(256) void mse_pair_fwd_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                           float* __restrict__ sum, int64_t n4) {
    __shared__ float part[4];
    float s = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const float4 av = reinterpret_cast<const float4*>(a)[e];
        const float4 gv = reinterpret_cast<const float4*>(g)[e];
        const float dx = av.x - gv.x, dy = av.y - gv.y, dz = av.z - gv.z, dw = av.w - gv.w;
        s += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) dhz_accum<DET>(sum + (DET ? blockIdx.x : 0), (part[0] + part[1]) + (part[2] + part[3]));
}

template <bool MASK>         // MASK: a is a post-ReLU map and da the gradient below that ReLU (zero where a <= 0)
__global__ __launch_bounds__(256) void mse_pair_bwd_kernel(const float* __restrict__ a, const float* __restrict__ g,
                                                           const float* __restrict__ gmean, float scale, float* __restrict__ da,
                                                           int64_t n4) {
    const float c = gmean[0] * scale;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        const float4 av = reinterpret_cast<const float4*>(a)[e];
        const float4 gv = reinterpret_cast<const float4*>(g)[e];
        float4 r = make_float4(c * (av.x - gv.x), c * (av.y - gv.y), c * (av.z - gv.z), c * (av.w - gv.w));
        if (MASK) {
            r.x = av.x > 0.f ? r.x : 0.f; r.y = av.y > 0.f ? r.y : 0.f;
            r.z = av.z > 0.f ? r.z : 0.f; r.w = av.w > 0.f ? r.w : 0.f;
        }
        reinterpret_cast<float4*>(da)[e] = r;
    }
}

// maxpool2x2_blocked_bwd_kernel (csrc/winograd_conv.hip) for a post-ReLU map that is a loss tap too: besides the pooled gradient, routed
// to the first maximum of each window, every position receives the tap's own gradient `add`; both pass the ReLU below (act > 0).
// One thread = 4 channels of one pooled pixel = four float4 of the un-pooled map.
__global__ __launch_bounds__(256) void maxpool2x2_blocked_bwd_add_kernel(const float4* __restrict__ gy, const float4* __restrict__ act,
                                                                         const float4* __restrict__ add, float4* __restrict__ gx,
                                                                         size_t total, int Ho, int Wo) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;     // over [n][ho][wo][2 halves]
    if (e >= total) return;
    const int hf = e & 1;
    const size_t p = e >> 1;
    const int wo = p % Wo;
    const size_t r = p / Wo;
    const int ho = r % Ho;
    const size_t n = r / Ho;
    const int W = 2 * Wo;
    const size_t o = ((n * (2 * Ho) + 2 * ho) * W + 2 * wo) * 2 + hf;
    const float4 a = act[o], b = act[o + 2], c = act[o + 2 * W], d = act[o + 2 * W + 2];
    const float4 ta = add[o], tb = add[o + 2], tc = add[o + 2 * W], td = add[o + 2 * W + 2];
    const float4 g = gy[e];
    float4 ra, rb, rc, rd;
#define ROUTE(f)                                                                              \
    {                                                                                         \
        const float m = fmaxf(fmaxf(a.f, b.f), fmaxf(c.f, d.f));                              \
        const float gv = m > 0.f ? g.f : 0.f;                                                 \
        const bool ia = a.f == m, ib = !ia && b.f == m, ic = !ia && !ib && c.f == m;          \
        ra.f = (ia ? gv : 0.f) + (a.f > 0.f ? ta.f : 0.f);                                    \
        rb.f = (ib ? gv : 0.f) + (b.f > 0.f ? tb.f : 0.f);                                    \
        rc.f = (ic ? gv : 0.f) + (c.f > 0.f ? tc.f : 0.f);                                    \
        rd.f = ((!ia && !ib && !ic) ? gv : 0.f) + (d.f > 0.f ? td.f : 0.f);                   \
    }
    ROUTE(x) ROUTE(y) ROUTE(z) ROUTE(w)
#undef ROUTE
    gx[o] = ra; gx[o + 2] = rb; gx[o + 2 * W] = rc; gx[o + 2 * W + 2] = rd;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int dhz_mse_pair_fwd(const float* a, const float* g, float* sum, int64_t count, void* stream) {
    DHZ_REQUIRE(a && g && sum, "dhz_mse_pair_fwd: null pointer");
    DHZ_REQUIRE(count > 0 && count % 4 == 0, "dhz_mse_pair_fwd: bad arguments (count must be a positive multiple of 4)");
    DHZ_REQUIRE(aligned16(a) && aligned16(g), "dhz_mse_pair_fwd: a and g must be 16-byte aligned");
    // three workgroups per CU; the deterministic cut uses the constant 256 (dhz_part_cus), so a reservation moves no bit
    const int grid = grid_for(count / 4, 3 * dhz_part_cus());
    if (dhz_det()) {                                      // one item per workgroup
        float* ws = dhz_det_ws("dhz_mse_pair_fwd", grid, 1);
        if (!ws) return DHZ_EINVAL;
        hipLaunchKernelGGL(mse_pair_fwd_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, g, ws, count / 4);
        DHZ_CHECK_LAUNCH("dhz_mse_pair_fwd");
        DetSegs segs{};
        segs.n = 1; segs.off[0] = 0; segs.len[0] = 1; segs.dst[0] = sum;
        return dhz_det_reduce("dhz_mse_pair_fwd", ws, grid, 1, segs, (hipStream_t)stream);
    }
    hipLaunchKernelGGL(mse_pair_fwd_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, g, sum, count / 4);
    DHZ_CHECK_LAUNCH("dhz_mse_pair_fwd");
    return DHZ_OK;
}

extern "C" int dhz_mse_pair_bwd(const float* a, const float* g, const float* gmean, float* da, int64_t count, int relu_mask,
                                void* stream) {
    DHZ_REQUIRE(a && g && gmean && da, "dhz_mse_pair_bwd: null pointer");
    DHZ_REQUIRE(count > 0 && count % 4 == 0, "dhz_mse_pair_bwd: bad arguments (count must be a positive multiple of 4)");
    DHZ_REQUIRE(aligned16(a) && aligned16(g) && aligned16(da), "dhz_mse_pair_bwd: a, g and da must be 16-byte aligned");
    const int grid = grid_for(count / 4, 8 * dhz_num_cus());
    const float scale = (float)(2.0 / (double)count);
    if (relu_mask)
        hipLaunchKernelGGL(mse_pair_bwd_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, g, gmean, scale, da, count / 4);
    else
        hipLaunchKernelGGL(mse_pair_bwd_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, g, gmean, scale, da, count / 4);
    DHZ_CHECK_LAUNCH("dhz_mse_pair_bwd");
    return DHZ_OK;
}

extern "C" int dhz_maxpool2x2_blocked_bwd_add(const float* gy, const float* act, const float* addend, float* gx, int N, int H, int W,
                                              void* stream) {
    DHZ_REQUIRE(gy && act && addend && gx, "dhz_maxpool2x2_blocked_bwd_add: null pointer");
    DHZ_REQUIRE(N > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "dhz_maxpool2x2_blocked_bwd_add: bad arguments (H, W even)");
    DHZ_REQUIRE(aligned16(gy) && aligned16(act) && aligned16(addend) && aligned16(gx),
                "dhz_maxpool2x2_blocked_bwd_add: the maps must be 16-byte aligned");
    const size_t total = (size_t)N * (H / 2) * (W / 2) * 2;
    hipLaunchKernelGGL(maxpool2x2_blocked_bwd_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(gy), reinterpret_cast<const float4*>(act),
                       reinterpret_cast<const float4*>(addend), reinterpret_cast<float4*>(gx), total, H / 2, W / 2);
    DHZ_CHECK_LAUNCH("dhz_maxpool2x2_blocked_bwd_add");
    return DHZ_OK;
}
