// Backward of a token-major Linear y = x W^T + b as ONE pass over the incoming gradient: dx = dy W, dW += dy^T x and db += sum dy from one
// read of dy [T, N] and x [T, K] and one split of each into the three bf16 pieces of the six-term product (csrc/bf16_pipe.h).  Replaces the
// pair dhz_linear_fwd_split6 (on the planes of W^T) + dhz_linear_wgrad_split where dy is the wide tensor of the block: LeFF linear1
// (N = 4C) and the packed Q / K / V projection (N = 3C) at C = 32 / 64.
//
// Persistent 512-thread workgroups, one per CU, each over a contiguous slab of 32-token stages with two stage buffers in LDS, as
// wgrad_split6_kernel (csrc/linear_split.hip): raw rows go global -> registers two stages ahead (every thread the same share), are split
// once and written as piece images [32 tokens][64 features] (dy: N / 64 of them side by side, then one of x; K = 32 fills half of its
// image).  A wave takes from the images of a stage
//   (a) its N/4 x K/2 share of the dW tile by transposed fragment reads (contraction over the 32 tokens), accumulators in registers over
//       the whole slab, and
//   (b) one 16 x 16 block of the stage's dx [32, K] by plain row reads of the same dy images (contraction over N), against the W^T
//       fragments of its 16 output columns, which it loads ONCE from the planes into registers.  At K = 32 there are four such blocks:
//       waves w and w + 4 each take half of the contraction and the upper one hands its part over through LDS.
// The dx block of stage s is stored behind the barrier of stage s, beside the work of stage s + 1.  At the end the dW tile goes through
// LDS to full-line fp32 atomics and db comes from the fp32 values each thread staged.
//
// Budget at N x K = 256 x 64: 48 KB of HBM traffic per stage and CU against 96 MFMAs per wave (two waves per SIMD): HBM-bound by design,
// the matrix pipe under half load.  Measured (profiles/r09_linear_bwd_pair.txt): 3.7 - 4.0 TB/s of dy + x + dx on 128 x 128 maps.
// Resources (-Rpass-analysis=kernel-resource-usage): 134 / 251 / 228 VGPRs at 128 x 32 / 256 x 64 / 192 x 64, no scratch, 80 / 120 / 96 KB
// of LDS.  Not available in deterministic mode (fp32 atomics): the entry refuses, ops.linear_bwd_pair runs the two launches there.
#include <type_traits>
#include <utility>
#include "bf16_pipe.h"

namespace {

constexpr int MAXMAT = 4;
constexpr int ST = 32;                  // tokens per stage
constexpr int NT = 512;                 // threads per workgroup
constexpr int IMG = ST * 64 * 2;        // one piece image: 32 tokens x 64 features, bf16

struct PairOut {
    float* dw[MAXMAT];
    float* db[MAXMAT];
    int nper;
};

template <int N, int K>
struct PairCfg {
    static constexpr int NS = N / 64;                               // dy images per piece
    static constexpr int PIECE = (NS + 1) * IMG, STAGE = 3 * PIECE;
    static constexpr int KSPLIT = 8 / (2 * (K / 16));               // waves that share one dx block (1 or 2)
    static constexpr int PART = KSPLIT == 2 ? 2 * 4 * 64 * 16 : 0;  // handed-over dx parts: [stage parity][block][lane] f32x4
    static constexpr size_t SMEM = 2 * (size_t)STAGE + PART;
    static_assert((size_t)N * K * 4 <= 2 * (size_t)STAGE && (size_t)ST * N * 4 <= 2 * (size_t)STAGE, "the epilogue reuses the stage buffers");
};

// f(integral_constant<int, 0>) ... f(integral_constant<int, n - 1>): a loop whose index is a constant inside the body
template <class F, int... I>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
// which of `np` pieces of the split rides behind group gi of `ng` MFMA groups (spread evenly; -1: none)
constexpr int piece_of(int gi, int ng, int np) {
    for (int p = 0; p < np; ++p)
        if (p * ng / np == gi) return p;
    return -1;
}

template <int N, int K>
__global__ __launch_bounds__(NT) void linear_bwd_pair_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x, int ldx,
                                                             const uint16_t* __restrict__ wt_hi, const uint16_t* __restrict__ wt_mid,
                                                             const uint16_t* __restrict__ wt_lo, float* __restrict__ dx, int T,
                                                             PairOut out) {
    using C = PairCfg<N, K>;
    constexpr int NS = C::NS, PIECE = C::PIECE, STAGE = C::STAGE, KSPLIT = C::KSPLIT;
    constexpr int QPR = N / 4, QA = ST * QPR / NT;                            // quads (4 values) of a dy stage: per row, per thread
    constexpr int XE = ST * K / NT;                                           // values of an x stage per thread (4 or 2)
    constexpr bool SAMECOL = NT % QPR == 0;                                   // a thread's quads all lie in one column group
    constexpr int NDB = SAMECOL ? 1 : QA;
    constexpr int WB = K / 32;                                                // dW: 4 waves across N (NS row blocks each), 2 across K
    constexpr int KS = N / 32 / KSPLIT;                                       // dx: contraction steps of a wave
    static_assert(QA * NT == ST * QPR && (XE == 4 || XE == 2), "a stage is a whole number of quads per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int wn = w & 3, wk = w >> 2;
    const int tb = w & 1, cb = KSPLIT == 2 ? (w >> 1) & 1 : w >> 1, half = KSPLIT == 2 ? w >> 2 : 0;     // dx block (tokens, columns), contraction half
    const int nst = T / ST;
    const int st0 = (int)((long long)nst * blockIdx.x / gridDim.x), st1 = (int)((long long)nst * (blockIdx.x + 1) / gridDim.x);

    // W^T fragments of the wave's 16 dx columns: plane row 16 cb + i16, the 8 contraction values 32 ks + 8 g ..
    dhz_u32x4 wf[3][KS];
    {
        const uint16_t* const pl[3] = {wt_hi, wt_mid, wt_lo};
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int s = 0; s < KS; ++s)
                wf[pc][s] = *reinterpret_cast<const dhz_u32x4*>(pl[pc] + (size_t)(16 * cb + i16) * N + 32 * (half * KS + s) + 8 * g);
    }
    f32x4 acc[NS][WB];
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < WB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc[NDB][4];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) dbacc[i][c] = 0.f;

    // this thread's share of a stage, the same for every thread (the split and the LDS writes then form ONE block of straight-line code
    // between the MFMAs): QA quads of dy, XE values of x.  LDS byte offset inside a piece, global byte offset inside a stage (32 bits)
    f32x4 ra[QA], rx = f32x4{0.f, 0.f, 0.f, 0.f};
    int a_off[QA];
    unsigned pa[QA];
#pragma unroll
    for (int i = 0; i < QA; ++i) {
        const int q = t + NT * i, row = q / QPR, c4 = q % QPR, ch = c4 >> 1;
        a_off[i] = (ch >> 3) * IMG + dhz_off_tr<64>(row, ch & 7) + 8 * (c4 & 1);
        pa[i] = (unsigned)((row * ldy + 4 * c4) * 4);
    }
    const int xrow = (t * XE) / K, xcol = (t * XE) % K;
    const int x_off = NS * IMG + dhz_off_tr<64>(xrow, xcol >> 3) + 2 * (xcol & 7);
    const unsigned px = (unsigned)((xrow * ldx + xcol) * 4);
    auto gload = [&](int st) {
        const size_t tok0 = (size_t)st * ST;
        const char* const da = reinterpret_cast<const char*>(dy) + tok0 * ldy * 4;
        const char* const xa = reinterpret_cast<const char*>(x) + tok0 * ldx * 4;
#pragma unroll
        for (int i = 0; i < QA; ++i) ra[i] = *reinterpret_cast<const f32x4*>(da + pa[i]);
        if constexpr (XE == 4) rx = *reinterpret_cast<const f32x4*>(xa + px);
        else {
            const dhz_f32x2 v = *reinterpret_cast<const dhz_f32x2*>(xa + px);
            rx[0] = v[0]; rx[1] = v[1];
        }
    };
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    // piece p < QA: quad p of dy; piece QA: the values of x
    auto swrite_piece = [&](int buf, auto p_) {
        constexpr int p = decltype(p_)::value;
        unsigned char* const S = smem + buf * STAGE;
        dhz_u32x4 hi, mid, lo;
        if constexpr (p < QA) {
            dhz_split8x3_np(ra[p], ra[p], hi, mid, lo);                       // (the second half is the first again: dropped by the compiler)
            *reinterpret_cast<u32x2*>(S + a_off[p]) = u32x2{hi[0], hi[1]};
            *reinterpret_cast<u32x2*>(S + PIECE + a_off[p]) = u32x2{mid[0], mid[1]};
            *reinterpret_cast<u32x2*>(S + 2 * PIECE + a_off[p]) = u32x2{lo[0], lo[1]};
#pragma unroll
            for (int c = 0; c < 4; ++c) dbacc[SAMECOL ? 0 : p][c] += ra[p][c];
        } else {
            dhz_split8x3_np(rx, rx, hi, mid, lo);
            if constexpr (XE == 4) {
                *reinterpret_cast<u32x2*>(S + x_off) = u32x2{hi[0], hi[1]};
                *reinterpret_cast<u32x2*>(S + PIECE + x_off) = u32x2{mid[0], mid[1]};
                *reinterpret_cast<u32x2*>(S + 2 * PIECE + x_off) = u32x2{lo[0], lo[1]};
            } else {
                *reinterpret_cast<uint32_t*>(S + x_off) = hi[0];
                *reinterpret_cast<uint32_t*>(S + PIECE + x_off) = mid[0];
                *reinterpret_cast<uint32_t*>(S + 2 * PIECE + x_off) = lo[0];
            }
        }
    };
    auto swrite = [&](int buf) { static_for(std::make_integer_sequence<int, QA + 1>{}, [&](auto p_) { swrite_piece(buf, p_); }); };
    // the dx block of the previous stage: stored (K = 32: by the lower wave of a pair, with the upper one's part) behind that stage's barrier
    f32x4 dprev = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4* const part = reinterpret_cast<f32x4*>(smem + 2 * STAGE);
    auto drain = [&](int st) {
        if (KSPLIT == 2) {
            if (half) return;
            dprev += part[((st & 1) * 4 + (w & 3)) * 64 + lane];
        }
        *reinterpret_cast<f32x4*>(dx + ((size_t)st * ST + 16 * tb + i16) * K + 16 * cb + 4 * g) = dprev;
    };

    if (st0 < st1) {
        gload(st0);
        swrite(st0 & 1);
        if (st0 + 1 < st1) gload(st0 + 1);
    }
    __syncthreads();
    constexpr int TA[6] = {2, 0, 1, 1, 0, 0}, TB[6] = {0, 2, 1, 0, 1, 0};      // (dy piece, other piece): lh hl mm mh hm hh
    // one stage; MORE: another stage of the slab follows, whose split and LDS writes ride between this one's MFMAs
    auto stage = [&](int st, auto more) {
        constexpr bool MORE = decltype(more)::value;
        const int buf = st & 1;
        const unsigned char* const S = smem + buf * STAGE;
        if (st > st0) drain(st - 1);
        // NS groups of MFMAs for (a) dW - group a: rows 16 (wn NS + a) .., columns 16 (wk WB + b) .. - then KS groups for (b) the dx^T
        // block D[column 4 g + j][token i16] = sum_n W^T[column][n] dy[token][n], one contraction step each.  The fragments of a group
        // are read one group ahead; behind each group's MFMAs rides one piece of the split and the LDS writes of stage st + 1 (the
        // other buffer: its readers passed the barrier at the end of stage st - 1), up to three vector instructions / LDS writes per
        // MFMA (a bf16 MFMA holds the vector issue for 8 of its 16 cycles: csrc/linear_split.hip).  Short groups that alternate
        // between the matrix pipe and the vector unit also let the two waves of a SIMD dovetail.
        constexpr int NG = NS + KS;
        dhz_s16x8 bf[3][WB], fr[2][3];
        f32x4 dacc = f32x4{0.f, 0.f, 0.f, 0.f};
        auto frags = [&](auto gi_, dhz_s16x8(&f)[3]) {
            constexpr int gi = decltype(gi_)::value;
            if constexpr (gi < NS) {
                const int nb = wn * NS + gi;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc) f[pc] = dhz_tr_frag<64>(S + pc * PIECE + (nb >> 2) * IMG, 8 * g, nb & 3, lane);
            } else {
                const int ks = half * KS + gi - NS;
#pragma unroll
                for (int pc = 0; pc < 3; ++pc)
                    f[pc] = *reinterpret_cast<const dhz_s16x8*>(S + pc * PIECE + (ks >> 1) * IMG + dhz_off_tr<64>(16 * tb + i16, (ks & 1) * 4 + g));
            }
        };
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int b = 0; b < WB; ++b) bf[pc][b] = dhz_tr_frag<64>(S + pc * PIECE + NS * IMG, 8 * g, wk * WB + b, lane);
        frags(std::integral_constant<int, 0>{}, fr[0]);
        static_for(std::make_integer_sequence<int, NG>{}, [&](auto gi_) {
            constexpr int gi = decltype(gi_)::value;
            constexpr int NM = gi < NS ? 6 * WB : 6;
            if constexpr (gi + 1 < NG) frags(std::integral_constant<int, gi + 1>{}, fr[(gi + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (gi < NS) {
#pragma unroll
                for (int term = 0; term < 6; ++term)
#pragma unroll
                    for (int b = 0; b < WB; ++b) acc[gi][b] = dhz_mfma_bf16(fr[gi & 1][TA[term]], bf[TB[term]][b], acc[gi][b]);
            } else {
#pragma unroll
                for (int term = 0; term < 6; ++term)
                    dacc = dhz_mfma_bf16(__builtin_bit_cast(dhz_s16x8, wf[TB[term]][gi - NS]), fr[gi & 1][TA[term]], dacc);
            }
            constexpr int p = piece_of(gi, NG, QA + 1);
            if constexpr (MORE && p >= 0) swrite_piece(buf ^ 1, std::integral_constant<int, p>{});
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x202, 3, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if (KSPLIT == 2 && half) part[(buf * 4 + (w & 3)) * 64 + lane] = dacc;
        else dprev = dacc;
        if (st + 2 < st1) gload(st + 2);
        // raw barrier: a __syncthreads() would also drain vmcnt, i.e. wait for the loads just issued
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    for (int st = st0; st + 1 < st1; ++st) stage(st, std::true_type{});
    if (st0 < st1) stage(st1 - 1, std::false_type{});
    if (st0 < st1) drain(st1 - 1);
    // ---- epilogue: tile -> LDS (row-major N x K fp32) -> full-line fp32 atomics; the stage buffers are free behind the last barrier
    float* const Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int a = 0; a < NS; ++a)
#pragma unroll
        for (int b = 0; b < WB; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) Cs[((wn * NS + a) * 16 + 4 * g + j) * K + (wk * WB + b) * 16 + i16] = acc[a][b][j];
    __syncthreads();
    for (int e = t; e < N * K; e += NT) {
        const int n = e / K, mat = n / out.nper;
        atomicAdd(out.dw[mat] + (size_t)(n - mat * out.nper) * K + e % K, Cs[e]);
    }
    bool do_db = false;
#pragma unroll
    for (int m = 0; m < MAXMAT; ++m) do_db = do_db || out.db[m] != nullptr;
    if (do_db) {
        __syncthreads();
        float* const red = reinterpret_cast<float*>(smem);                 // [rows of quads][N]
        constexpr int ROWS = SAMECOL ? NT / QPR : ST;
#pragma unroll
        for (int i = 0; i < NDB; ++i) {
            const int q = t + NT * i;
            *reinterpret_cast<f32x4*>(red + (q / QPR) * N + 4 * (q % QPR)) = f32x4{dbacc[i][0], dbacc[i][1], dbacc[i][2], dbacc[i][3]};
        }
        __syncthreads();
        if (t < N) {
            float tot = 0.f;
            for (int r = 0; r < ROWS; ++r) tot += red[r * N + t];
            const int mat = t / out.nper;
            if (out.db[mat]) atomicAdd(out.db[mat] + t - mat * out.nper, tot);
        }
    }
}

// one workgroup per CU of the current setting, never more than there are stages
int pair_grid(int T) {
    const int nst = T / ST, cus = dhz_num_cus();
    return cus < nst ? cus : nst;
}

bool pair_shape(int N, int K) { return (N == 128 && K == 32) || (N == 256 && K == 64) || (N == 192 && K == 64); }

template <int N, int K>
void launch(int grid, hipStream_t s, const float* dy, int ldy, const float* x, int ldx, const uint16_t* hi, const uint16_t* mid,
            const uint16_t* lo, float* dx, int T, const PairOut& out) {
    constexpr size_t smem = PairCfg<N, K>::SMEM;
    dhz_allow_smem(&linear_bwd_pair_kernel<N, K>, smem);
    hipLaunchKernelGGL((linear_bwd_pair_kernel<N, K>), dim3(grid), dim3(NT), smem, s, dy, ldy, x, ldx, hi, mid, lo, dx, T, out);
}

}  // namespace

extern "C" int dhz_linear_bwd_pair_grid(int T, int N, int K) {
    if (T <= 0 || T % ST || !pair_shape(N, K)) return 0;
    return pair_grid(T);
}

extern "C" int dhz_linear_bwd_pair(const float* dy, int ldy, const float* x, int ldx, const void* wt_hi, const void* wt_mid,
                                   const void* wt_lo, float* dx, int T, int nmat, int nper, int K, float* const* dw, float* const* db,
                                   void* stream) {
    const char* who = "dhz_linear_bwd_pair";
    DHZ_REQUIRE(!dhz_det(), "%s: accumulates with fp32 atomics: not available in deterministic mode (run dhz_linear_fwd_split6 on the "
                            "planes of W^T and dhz_linear_wgrad_split)", who);
    DHZ_REQUIRE(dy && x && wt_hi && wt_mid && wt_lo && dx && dw, "%s: null pointer", who);
    DHZ_REQUIRE(nmat >= 1 && nmat <= MAXMAT, "%s: nmat=%d must be 1..%d", who, nmat, MAXMAT);
    DHZ_REQUIRE(T > 0 && T % ST == 0, "%s: T=%d must be a positive multiple of %d", who, T, ST);
    DHZ_REQUIRE(nper > 0 && nper % 16 == 0 && pair_shape(nmat * nper, K),
                "%s: N=%d (nmat=%d x nper=%d) K=%d: instances are N x K = 128 x 32, 256 x 64 and 192 x 64", who, nmat * nper, nmat, nper, K);
    const int N = nmat * nper;
    DHZ_REQUIRE(ldy % 4 == 0 && ldy >= N, "%s: ldy=%d must be a multiple of 4 and at least N=%d", who, ldy, N);
    DHZ_REQUIRE(ldx % 4 == 0 && ldx >= K, "%s: ldx=%d must be a multiple of 4 and at least K=%d", who, ldx, K);
    DHZ_REQUIRE(!(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)wt_hi | (uintptr_t)wt_mid | (uintptr_t)wt_lo | (uintptr_t)dx) & 15),
                "%s: dy, x, the planes and dx must be 16-byte aligned", who);
    PairOut out = {};
    for (int i = 0; i < nmat; ++i) {
        DHZ_REQUIRE(dw[i], "%s: null dw[%d]", who, i);
        out.dw[i] = dw[i];
        out.db[i] = db ? db[i] : nullptr;
    }
    out.nper = nper;
    const int grid = pair_grid(T);
    hipStream_t s = (hipStream_t)stream;
    const uint16_t *hi = (const uint16_t*)wt_hi, *mid = (const uint16_t*)wt_mid, *lo = (const uint16_t*)wt_lo;
    if (N == 128) launch<128, 32>(grid, s, dy, ldy, x, ldx, hi, mid, lo, dx, T, out);
    else if (N == 256) launch<256, 64>(grid, s, dy, ldy, x, ldx, hi, mid, lo, dx, T, out);
    else launch<192, 64>(grid, s, dy, ldy, x, ldx, hi, mid, lo, dx, T, out);
    DHZ_CHECK_LAUNCH(who);
    return DHZ_OK;
}
