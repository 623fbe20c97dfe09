// Second stage of the deterministic mode (dhz_set_deterministic, include/dehaze_hip.h): the accumulating kernels' DET instances have
// stored the partial of work item i at ws[i * slot + ...] with plain stores; here ONE thread owns an output element, sums its `items`
// partials in ascending item order and adds the sum to the target - the "caller zeroes, kernel accumulates" contract is kept, and two
// calls that share a target add in stream order.  No atomics: the sum is a function of the inputs and of the (shape-only) cut alone.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void det_reduce_kernel(const float* __restrict__ ws, int items, long slot, DetSegs segs, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    int s = 0;
    long r = e;
    while (r >= segs.len[s]) r -= segs.len[s++];          // at most 8 segments
    const float* p = ws + segs.off[s] + r;
    float sum = 0.f;
    int i = 0;
    for (; i + 4 <= items; i += 4) {                      // four loads in flight, added in item order
        const float a = p[(long)i * slot], b = p[(long)(i + 1) * slot], c = p[(long)(i + 2) * slot], d = p[(long)(i + 3) * slot];
        sum += a; sum += b; sum += c; sum += d;
    }
    for (; i < items; ++i) sum += p[(long)i * slot];
    segs.dst[s][r] += sum;
}

}  // namespace

int dhz_det_reduce(const char* who, const float* ws, int items, long slot, const DetSegs& segs, hipStream_t s) {
    long total = 0;
    DHZ_REQUIRE(segs.n >= 1 && segs.n <= DHZ_DET_MAXSEG && items >= 1, "%s: deterministic reduction of %d segments, %d items", who, segs.n, items);
    for (int i = 0; i < segs.n; ++i) {
        DHZ_REQUIRE(segs.dst[i] && segs.len[i] > 0 && segs.off[i] >= 0 && segs.off[i] + segs.len[i] <= slot,
                    "%s: deterministic reduction: segment %d (offset %ld, %ld floats) outside the slot of %ld", who, i, segs.off[i], segs.len[i], slot);
        total += segs.len[i];
    }
    hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws, items, slot, segs, total);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}
