/*
 * dehaze_hip.h - C-ABI of the MI355X (gfx950) kernels behind the Uformer_ProbSparse training path.
 *
 * The reference (xin-fight/...Image-Dehazing...Vision-Transformer) is pure Python/PyTorch: it has no
 * FFI layer of its own, so every entry point below replaces a *sequence of ATen ops* in the reference;
 * the file:line each one replaces is cited (M1 = Uformer_ProbSparse/My_model_1.py, M0 = My_model.py,
 * ATT = Uformer_ProbSparse/ProbSparse/attn.py, TR = My_train.py).  The reference-side binding a
 * maintainer would add is a ctypes stub - see INTEGRATION.md.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, an explicit hipStream_t passed as void*; no torch types.
 *   - the caller owns every buffer (allocate through the framework's caching allocator); no entry
 *     point allocates, frees or synchronises; all work is enqueued on `stream`.
 *   - return 0 on success, a negative DHZ_E* code otherwise; dhz_last_error() gives the message of
 *     the last failure on the calling thread.
 *   - all floating-point tensors are fp32, contiguous unless a leading dimension `ld*` is given.
 *   - re-entrant across streams/devices; no hidden global state.
 */
#ifndef DEHAZE_HIP_H
#define DEHAZE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHZ_OK 0
#define DHZ_EINVAL (-22)  /* bad argument (shape / null pointer / unsupported head_dim) */
#define DHZ_ELAUNCH (-5)  /* hipLaunchKernel reported an error */

/* Storage type of token tensors for the dhz_*_dt entry points (BASELINE config 4: bf16 activations in HBM, fp32 arithmetic
 * and accumulation inside every kernel, fp32 parameters / statistics / parameter gradients). */
#define DHZ_F32 0
#define DHZ_BF16 1

#define DHZ_NTOK 64 /* tokens per 8x8 window */
#define DHZ_NTOP 25 /* u = U_part = 5*ceil(ln 64)  (ATT:310-315) */

int dhz_abi_version(void);
const char* dhz_last_error(void);
/* 16 hex digits: content hash of the sources (every .hip file under csrc/, common.h, this header) the loaded library was built from.  The PMC
 * passes stamp it into profiles/pmc_traffic.json; bench.py reports `roofline.traffic` only when the stamp matches. */
const char* dhz_build_id(void);
/* Compute units the persistent grids of this library leave free (default 0 = none).  One process per GPU with the gradient exchange
 * overlapping the backward pass (replaces nn.DataParallel, My_train.py:97): RCCL's collective kernels need CUs beside grids that are sized
 * "resident workgroups per CU x CUs"; dhz_set_reserved_cus(k) sizes every such grid for (CUs - k).  Results do not depend on it.
 * dhz_grid_cus() = the CU count the grids are sized for (physical - reserved). */
int dhz_set_reserved_cus(int k);
int dhz_get_reserved_cus(void);
int dhz_grid_cus(void);
/* Deterministic mode (process-global like the reservation; default 0 = off: nothing changes).  With it on, every entry that ACCUMULATES a
 * parameter gradient or a loss sum - the token-Linear / convolution / depthwise / input-projection weight gradients, LayerNorm dgamma / dbeta,
 * the relative-position table gradient, the Charbonnier and L1-pair sums - runs a second instance of its kernel: work item i (token slab, tile
 * slot, workgroup) STORES its partial in slot i of the workspace, and one reduction kernel (csrc/det_reduce.hip) sums the slots in ascending
 * order, one owner thread per element, and adds the sum to the target.  No fp32 atomic, global or LDS, contributes; the cut into items is a
 * function of the problem shape alone (slab counts and tile choices otherwise derived from the CU count use the constant 256; the size of a
 * persistent grid whose workgroups walk the tiles still follows the CU count: it moves no bit), so results are bit-identical from
 * run to run, under any dhz_set_reserved_cus and on any device.  "Caller zeroes, kernel accumulates" holds in both modes.
 * Scope: fp32 storage, one process.  The bf16-storage accumulating entries (dhz_linear_wgrad_bf16, dhz_l1_pair_fwd_bf16, the DHZ_BF16 forms of
 * the LayerNorm / depthwise / thin-convolution / input-projection backward) and dhz_fused_window_attn_bwd return DHZ_EINVAL while the mode is
 * on (the Python side routes C = 32 attention to its backward chain).
 * dhz_set_det_workspace: device memory the mode may use (16-byte aligned; NULL, 0 takes it away); used in stream order, so all calls that
 * accumulate must be on ONE stream.  An entry that needs more than `bytes` returns DHZ_EINVAL and names the bytes it needs - never a
 * fall-back to atomics. */
int dhz_set_deterministic(int on);
int dhz_get_deterministic(void);
int dhz_set_det_workspace(float* ws, size_t bytes);

/* ---------------------------------------------------------------------------------------------
 * K3  ProbSparse window attention core.   Replaces ProbAttention.forward  ATT:287-342
 *     (_prob_QK ATT:71-152, _get_initial_context ATT:154-176, _update_context ATT:178-281).
 *
 * q,k,v : [B_, 64, H, d] fp32 with token stride `ld` floats (element (b,n,h,e) at
 *         ((b*64+n)*ld + h*d + e)); ld = H*d for separate projections, 3*H*d for a packed QKV.
 * idx   : [64, 25] uint8 sampled key ids, shared by all windows/heads (ATT:91).
 * bias  : [H, 64, 64] relative-position bias (M1:408-410) or NULL (options.is_relative_position_bias
 *         False, ATT:227-232).   mask: [nW, 64, 64] (0 / -100) or NULL; window id = b mod nW.
 * out   : [B_, 64, H, d], token stride ldo.
 * rank  : [B_, H, 64] uint8 - for each query its position (0..24, by descending sparsity measure M)
 *         in the top-u set, 255 if not selected.  Saved for backward.
 * d must be 32 or 64.
 */
int dhz_ps_attn_fwd(const float* q, const float* k, const float* v, int ld, const uint8_t* idx,
                    const float* bias, const float* mask, float* out, int ldo, uint8_t* rank,
                    int B_, int H, int nW, int d, void* stream);

/* Backward of the above (autograd of ATT:287-342; gradient flows through steps 6-12 only).
 * dout: [B_,64,H,d] stride ldo.  dq,dk,dv: [B_,64,H,d] stride ldg (every element written).
 * dbias_part: workspace [dhz_ps_attn_bwd_parts_d(B_,H,d), 64, 64] fp32 (written, not accumulated) or
 *             NULL when bias == NULL.  Row p holds the partial bias gradient of head (p % H);
 *             reduce with dhz_bias_table_grad.
 */
int dhz_ps_attn_bwd_parts(int B_, int H);            /* dhz_dense_attn_bwd */
int dhz_ps_attn_bwd_parts_d(int B_, int H, int d);   /* dhz_ps_attn_bwd: its persistent workgroups (two per CU) */
int dhz_ps_attn_bwd(const float* q, const float* k, const float* v, int ld, const float* bias,
                    const float* mask, const uint8_t* rank, const float* dout, int ldo, float* dq,
                    float* dk, float* dv, int ldg, float* dbias_part, int B_, int H, int nW, int d,
                    void* stream);

/* K1+K2+K3+K4  Fused attention branch of a LeWin block, forward, for C = 32, 64, 128 (head_dim 32):
 *     out = x + drop_scale[b] * out_projection(ProbAttention(Q,K,V = projections(window(roll(norm1(x))))))
 *     Replaces M1:839-872 + ATT:385-461 in one kernel (one workgroup per 8x8 window, per-head QKV GEMM and
 *     the out-projection on the fp32 matrix pipe around the LDS-resident ProbSparse core).
 * dhz_fused_attn_prepack: reorders the four [C,C] projection weights into MFMA B-fragment order
 *     (wqkv_p: 3*C*C floats, wo_p: C*C floats); call whenever the weights change.
 * x,out: [B, Hres*Wres, C] tokens.  bqkv = [bq|bk|bv] (3C), bo (C).  idx [64,25] uint8.  bias [H,64,64] or
 *     NULL.  mask [nW,64,64] (shifted blocks) or NULL.  drop_scale [B] or NULL (DropPath keep/keep_prob).
 * Training mode - all five save pointers non-NULL, window-ordered rows r = (b*nW + w)*64 + token:
 *     xn_save [T,C] (LayerNorm output), qkv_save [T,3C], ctx_save [T,C], stats_save [B*HW,2] (mean, rstd by
 *     source token), rank_save [B*nW, H, 64] - exactly what dhz_ps_attn_bwd / dhz_linear_wgrad /
 *     dhz_ln_partition_bwd consume.  Inference mode: pass NULL for all five. */
int dhz_fused_attn_prepack(const float* wq, const float* wk, const float* wv, const float* wo,
                           float* wqkv_p, float* wo_p, int C, void* stream);
/* ... for n <= 16 blocks in ONE launch (host arrays of device pointers; C[i] in {32, 64, 128}).  Same values as n calls of
 * dhz_fused_attn_prepack. */
int dhz_fused_attn_prepack_multi(const float* const* wq, const float* const* wk, const float* const* wv, const float* const* wo,
                                 float* const* wqkv_p, float* const* wo_p, const int* C, int n, void* stream);
int dhz_fused_window_attn_fwd(const float* x, const float* gamma, const float* beta, const float* wqkv_p,
                              const float* bqkv, const float* wo_p, const float* bo, const uint8_t* idx,
                              const float* bias, const float* mask, const float* drop_scale, float* out,
                              float* xn_save, float* qkv_save, float* ctx_save, float* stats_save,
                              uint8_t* rank_save, int B, int Hres, int Wres, int C, int shift,
                              void* stream);
/* The same kernel with the Q / K / V product of every head on the bf16 matrix pipe in the six-term form of dhz_linear_fwd_split6 (three bf16
 * truncation pieces per operand value, products hh hm mh hl lh mm, dropped terms <= 2^-24 relative, fp32 accumulation: fp32-class results).
 * So is the out-projection (its planes in the S tile while P V runs).  wqkv6_p: the planes of the four weights in the kernel's fragment order
 * (dhz_fused_attn_prepack6: (C/32) ((C/64) 36 + (C/16) 3) KiB of bf16), brought ONCE per workgroup and head by LDS-DMA into tiles that are dead
 * at that point - not once per wave through L1.  Every other argument as dhz_fused_window_attn_fwd (wo_p is not read).  C = 64. */
int dhz_fused_window_attn_fwd6(const float* x, const float* gamma, const float* beta, const void* wqkv6_p, const float* bqkv,
                               const float* wo_p, const float* bo, const uint8_t* idx, const float* bias, const float* mask,
                               const float* drop_scale, float* out, float* xn_save, float* qkv_save, float* ctx_save, float* stats_save,
                               uint8_t* rank_save, int B, int Hres, int Wres, int C, int shift, void* stream);
/* The inference form (no save buffers) of either kernel with the PADDING MASK of any-size evaluation as one 64-bit word per window:
 *     pad[B nW] from dhz_pad_window_bits, bit j of word b = token j of window b (image-major, then window row, window column of the ROLLED
 *     map, M1:791-800) is padding.  Replaces, per block,
 *          m  = F.interpolate(mask, (H, W)); am = window_partition(m)              ([B nW, 64])
 *          am = (am[:, :, None] * am[:, None, :]).masked_fill(!= 0, -100)          ([B nW, 64, 64] fp32: 16 KiB per window)
 *          attn_mask = am + shift_mask                                             (batch 1 only: [B nW, ..] + [nW, ..])
 *     and the unfused kernel chain that a [B nW, 64, 64] mask forced.  The kernel adds (shift-mask term + padding term) where it adds the
 *     shift mask; a word of 0 skips the term.  six_term != 0: wqkv_p holds dhz_fused_attn_prepack6's planes (dhz_fused_window_attn_fwd6),
 *     else dhz_fused_attn_prepack's fragments.  mask stays the [nW, 64, 64] shift mask (NULL iff shift == 0); pad is valid at any shift. */
int dhz_fused_window_attn_fwd_pad(int six_term, const float* x, const float* gamma, const float* beta, const void* wqkv_p, const float* bqkv,
                                  const float* wo_p, const float* bo, const uint8_t* idx, const float* bias, const float* mask,
                                  const uint64_t* pad, const float* drop_scale, float* out, int B, int Hres, int Wres, int C, int shift,
                                  void* stream);
int dhz_fused_attn_prepack6(const float* wq, const float* wk, const float* wv, const float* wo, void* wqkv6_p, int C, void* stream);
/* ... for n <= 16 blocks in ONE launch (host arrays of device pointers). */
int dhz_fused_attn_prepack6_multi(const float* const* wq, const float* const* wk, const float* const* wv, const float* const* wo,
                                  void* const* wqkv6_p, const int* C, int n, void* stream);

/* Fused BACKWARD of the same branch at C = 32 (one head): given d(out) it recomputes LayerNorm, Q/K/V, the selected scores, both
 *     softmaxes and P V per window from x and the 64 selection ranks the forward saved (rank_save of dhz_fused_window_attn_fwd
 *     called with rank_save ALONE), and produces dx (shortcut included) and every parameter gradient on chip.  Replaces, per block,
 *     the autograd chain of M1:839-872: dhz_reverse_residual_bwd, two backward-data GEMMs, three weight-gradient launches,
 *     dhz_ps_attn_bwd, dhz_ln_partition_bwd.
 *     wqkv_p: the forward's prepack (dhz_fused_attn_prepack); wt [4096]: dhz_fused_attn_bwd_prepack(wq, wk, wv, wo).
 *     ACCUMULATED with fp32 atomics (caller zeroes): dwq, dwk, dwv, dwo [32, 32]; dbq, dbk, dbv, dbo [32] (each may be NULL);
 *     dgamma, dbeta [32].  dbias_part [dhz_fused_attn_bwd_parts(nwin)][64][64] (written, not accumulated) iff bias != NULL:
 *     reduce with dhz_bias_table_grad.  dx [B, Hres*Wres, 32] is written. */
int dhz_fused_attn_bwd_parts(int nwin);
int dhz_fused_attn_bwd_prepack(const float* wq, const float* wk, const float* wv, const float* wo, float* wt, int C, void* stream);
int dhz_fused_window_attn_bwd(const float* x, const float* dout, const float* gamma, const float* beta, const float* wqkv_p,
                              const float* bqkv, const float* wt, const float* bias, const float* mask, const float* drop_scale,
                              const uint8_t* rank, float* dx, float* dwq, float* dwk, float* dwv, float* dbq, float* dbk,
                              float* dbv, float* dwo, float* dbo, float* dgamma, float* dbeta, float* dbias_part, int B, int Hres,
                              int Wres, int C, int shift, void* stream);

/* K3-dense  Dense window attention of the My_model.Uformer twin.  Replaces WindowAttention.forward
 *     M0:428-492:  out = softmax(scale * q k^T + bias[h] + mask[b % nW]) v   per (window, head).
 *     Same layouts as dhz_ps_attn_fwd (q,k,v [B_,64,H,d] with token stride ld; bias [H,64,64] or NULL;
 *     mask [nW,64,64] or NULL).  Nothing is saved: the backward recomputes the probabilities.
 *     dbias_part: [dhz_ps_attn_bwd_parts(B_,H), 64, 64] partials, reduced by dhz_bias_table_grad. */
int dhz_dense_attn_fwd(const float* q, const float* k, const float* v, int ld, const float* bias,
                       const float* mask, float* out, int ldo, int B_, int H, int nW, int d,
                       float scale, void* stream);
int dhz_dense_attn_bwd(const float* q, const float* k, const float* v, int ld, const float* bias,
                       const float* mask, const float* dout, int ldo, float* dq, float* dk, float* dv,
                       int ldg, float* dbias_part, int B_, int H, int nW, int d, float scale,
                       void* stream);

/* K7  relative-position bias:  bias[h,i,j] = table[rel_index(i,j), h]   (M1:408-410, win = 8).
 * table: [225, H].  bias: [H,64,64]. */
int dhz_bias_gather(const float* table, float* bias, int H, void* stream);
/* ... for every block of one model forward in ONE launch (host arrays of n <= 32 device pointers / head counts; entry i: biases[i][H_i,64,64]
 * from tables[i][225,H_i]).  Same values as n calls of dhz_bias_gather. */
int dhz_bias_gather_multi(const float* const* tables, float* const* biases, const int* heads, int n, void* stream);
/* dtable[t,h] (+)= sum_p sum_{(i,j): rel_index(i,j)=t} dbias_part[p,i,j] over parts p with p%H==h.
 * dtable: [225,H], overwritten when accumulate == 0. */
int dhz_bias_table_grad(const float* dbias_part, int parts, float* dtable, int H, int accumulate,
                        void* stream);
/* ... for n <= 32 blocks in ONE launch, ACCUMULATING into dtable[i] (host arrays; the accumulate = 1 form of dhz_bias_table_grad per entry). */
int dhz_bias_table_grad_multi(const float* const* dbias_part, const int* parts, float* const* dtable, const int* heads, int n, void* stream);

/* K9  InputProj: Conv2d(3, E, 3x3, padding 1) + LeakyReLU(slope) from the NCHW image into the token layout, M1:659-682
 *     (replaces aten::convolution + aten::leaky_relu_ + the NCHW -> token copy), E = 32 or 64.
 *     dhz_input_proj_fwd: img [B,3,H,W], w [E,3,3,3], bias [E] -> y [B, H*W, E].
 *     dhz_input_proj_bwd: dy, y (the forward output: the LeakyReLU mask is its sign) -> dw [E,3,3,3], db [E] ACCUMULATED (fp32
 *     atomics, caller zeroes).  The image needs no gradient on this path (M1:1169). */
int dhz_input_proj_fwd(const float* img, const float* w, const float* bias, float* y, int B, int H, int W, int E, float slope,
                       void* stream);
int dhz_input_proj_bwd(const float* dy, const float* y, const float* img, float* dw, float* db, int B, int H, int W, int E,
                       float slope, void* stream);
/* the same with the token tensors (y, dy) stored as `dtype` (DHZ_F32 / DHZ_BF16; image, weights and gradients fp32) */
int dhz_input_proj_fwd_dt(const float* img, const float* w, const float* bias, void* y, int B, int H, int W, int E, float slope,
                          int dtype, void* stream);
int dhz_input_proj_bwd_dt(const void* dy, const void* y, const float* img, float* dw, float* db, int B, int H, int W, int E,
                          float slope, int dtype, void* stream);

/* K8  Downsample: Conv2d(Cin, Cout, kernel 4, stride 2, padding 1) on the token layout, M1:606-622, as implicit GEMMs on the fp32
 *     matrix pipe (no im2col matrix: a tap of an output pixel is one contiguous run of Cin floats of a token).
 *     x [B, H*W, Cin] -> y [B, (H/2)*(W/2), Cout].  wp = weight.permute(0,2,3,1) as [Cout, 16*Cin] (taps-major, channels
 *     contiguous), wq = weight.permute(2,3,0,1) as [16*Cout, Cin]; H, W even; Cin, Cout multiples of 32.
 *     dhz_conv4s2_fwd  : replaces aten::convolution (MIOpen implicit GEMM)             bias [Cout] or NULL
 *     dhz_conv4s2_dgrad: dx [B, H*W, Cin] from dy [B, (H/2)*(W/2), Cout] (every element written; four parity-class GEMMs)
 *     dhz_conv4s2_wgrad: dwp [Cout, 16*Cin] += dy^T xcol, db [Cout] += column sums (ACCUMULATED, fp32 atomics; db may be NULL);
 *                        the output map sizes must be powers of two (training patch sizes 128 / 256). */
int dhz_conv4s2_fwd(const float* x, const float* wp, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                    void* stream);
int dhz_conv4s2_dgrad(const float* dy, const float* wq, float* dx, int B, int H, int W, int Cin, int Cout, void* stream);
int dhz_conv4s2_wgrad(const float* dy, const float* x, float* dwp, float* db, int B, int H, int W, int Cin, int Cout,
                      void* stream);
/*     dhz_conv4s2_tile: which tile instance <WM, WN> (32 WM rows x 32 WN columns per workgroup) the entry above runs for this shape
 *     under the current dhz_set_reserved_cus / dhz_set_deterministic state, as 10 WM + WN.  mode 1 = forward, 2 = backward-data
 *     (all four parity launches share it), 3 = weight gradient (a function of Cin, Cout alone).  0 for a shape the entry refuses.
 *     Host-side only; the dispatch asks the same function, so the answer is what is launched. */
int dhz_conv4s2_tile(int mode, int B, int H, int W, int Cin, int Cout);
/* K8 on the bf16 matrix pipe, six-term (csrc/split6_gemm.hip: the plane kernels of the token Linears with a gathered activation operand;
 *     same x / y / dy / dx as above, fp32, the arithmetic and error class of dhz_linear_fwd_split6).
 *     dhz_conv4s2_prepack6: from weight [Cout, Cin, 4, 4] the truncation-split bf16 planes (hi | mid | lo, 16 Cin Cout elements each, 96 Cin Cout
 *                        bytes per set) of weight.permute(0,2,3,1) [Cout][(ky, kx, ci)] -> fwd_planes and of weight.permute(1,2,3,0)
 *                        [Cin][(ky, kx, co)] -> bwd_planes, bit-identical to dhz_split3_planes of those tensors; one launch; either set may be
 *                        NULL.  Cin, Cout multiples of 32.
 *     dhz_conv4s2_fwd6 : y = conv(x) + bias (bias may be NULL).  H, W even, Cin a multiple of 32, Cout a multiple of 64 and <= 2048.
 *     dhz_conv4s2_dgrad6: dx, every element written exactly once, ONE launch over (parity class, row tile, column tile).  H, W even,
 *                        Cin, Cout multiples of 32, Cin <= 2048.
 *     dhz_conv4s2_tile6: the tile of mode 1 = dhz_conv4s2_fwd6, 2 = dhz_conv4s2_dgrad6 under the current dhz_set_reserved_cus /
 *                        dhz_set_deterministic state, as dhz_linear_split6_tile writes it: 44 = 128 x 128, 42 = 128 x 64, 41 = 128 x 32
 *                        (backward-data only); 0 for a shape the entry refuses.  Backward-data chooses from the rows of all four classes. */
int dhz_conv4s2_prepack6(const float* weight, void* fwd_planes, void* bwd_planes, int Cin, int Cout, void* stream);
int dhz_conv4s2_fwd6(const float* x, const void* fwd_planes, const float* bias, float* y, int B, int H, int W, int Cin, int Cout,
                     void* stream);
int dhz_conv4s2_dgrad6(const float* dy, const void* bwd_planes, float* dx, int B, int H, int W, int Cin, int Cout, void* stream);
int dhz_conv4s2_tile6(int mode, int B, int H, int W, int Cin, int Cout);

/* K8 in bf16 (BASELINE config 4): the same convolution as three token-Linear GEMMs on the bf16 matrix pipe (dhz_linear_fwd_bf16 /
 *     _dgrad_bf16 / _wgrad_bf16 with wp [Cout, 16*Cin]) over an explicit tap-major patch matrix; in the token layout a tap of an
 *     output pixel is one contiguous run of Cin bf16, so both helpers are 16-byte-per-lane streaming copies.  Replaces
 *     aten::convolution / convolution_backward under autocast (MIOpen igemm / CK grouped-conv kernels).
 *     dhz_im2col_k4s2_bf16: x bf16 [B, H*W, Cin] -> col bf16 [B*(H/2)*(W/2), 16*Cin], col[.][(ky, kx, ci)] = x[2ho+ky-1, 2wo+kx-1, ci]
 *     dhz_col2im_k4s2_bf16: dx bf16 [B, H*W, Cin] = for every input pixel the fp32 sum of the 4 dcol entries that read it.
 *     H, W even; Cin a multiple of 8; 16-byte aligned buffers. */
int dhz_im2col_k4s2_bf16(const void* x, void* col, int B, int H, int W, int Cin, void* stream);
int dhz_col2im_k4s2_bf16(const void* dcol, void* dx, int B, int H, int W, int Cin, void* stream);

/* K5 fused  The whole LeFF branch of a LeWin block for C = 32, 64, 128 (hidden width 4C), forward, in one kernel:
 *     out = x + drop_scale[b] * linear2(gelu(dwconv3x3(gelu(linear1(norm2(x))))))          replaces M1:873 + M1:496-534
 *     (LayerNorm, both Linears on the fp32 matrix pipe around an LDS-resident 8x16-pixel tile + halo, both GELUs, the
 *     depthwise 3x3 convolution, bias adds, DropPath scale and the residual - the 4C-wide hidden tensors never travel
 *     to HBM except as the saves below).
 * x, out: [B, Hres*Wres, C] tokens; gamma, beta [C]; w1 [4C, C], b1 [4C]; wd [4C, 3, 3] (Conv2d groups = 4C), bd [4C];
 * w2 [C, 4C], b2 [C]; drop_scale [B] or NULL.  Hres % 8 == 0, Wres % 16 == 0.
 * Training mode - the five save pointers all non-NULL (else all NULL): xn_save [T, C] (norm2 output), stats_save [T, 2]
 * (mean, rstd), u_save [T, 4C] (linear1 output before GELU), tp_save [T, 4C] (gelu'(t), t = dwconv output + bd),
 * z_save [T, 4C] (gelu(t), the input of linear2) - what dhz_leff_dwconv_bwd and dhz_linear_wgrad consume. */
int dhz_leff_fused_fwd(const float* x, const float* gamma, const float* beta, const float* w1, const float* b1,
                       const float* wd, const float* bd, const float* w2, const float* b2, const float* drop_scale,
                       float* out, float* xn_save, float* stats_save, float* u_save, float* tp_save, float* z_save,
                       int B, int Hres, int Wres, int C, void* stream);
/* The same kernel with its two weight products (linear1, linear2) as six-term products on the bf16 matrix pipe (the arithmetic of
 * dhz_linear_fwd_split6: fp32-class results): w6 = the planes of both weights in the kernel's MFMA fragment order (dhz_leff_prepack6:
 * 24 C^2 bf16), read by every wave straight from L1 / L2; the LayerNorm output and z live in LDS as bf16 piece images.  C = 32, 64. */
int dhz_leff_fused_fwd6(const float* x, const float* gamma, const float* beta, const void* w6, const float* b1, const float* wd,
                        const float* bd, const float* b2, const float* drop_scale, float* out, float* xn_save, float* stats_save,
                        float* u_save, float* tp_save, float* z_save, int B, int Hres, int Wres, int C, void* stream);
int dhz_leff_prepack6(const float* w1, const float* w2, void* w6, int C, void* stream);

/* K2/K4/K5  forward and backward-data GEMMs of every token-major nn.Linear on the path (query/key/value/out
 *     projections ATT:420-422,454-458; LeFF linear1/linear2 M1:487-492,508,529; the 2x2/stride-2 transposed convolution
 *     of Upsample M1:633-648 in its token-Linear form), on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32):
 *     dhz_linear_fwd  : y[T,N]  = x[T,K] . w[N,K]^T + bias[N]       replaces aten::addmm / F.linear   (bias may be NULL)
 *     dhz_linear_dgrad: dx[T,K] = dy[T,N] . w[N,K]                   replaces the aten::mm of Linear's backward
 *     x / y / dy / dx are token-major with row strides ldx / ldy (floats, multiples of 4; packed QKV buffers pass 3C);
 *     w is contiguous [N,K].  N % 32 == 0, K % 32 == 0, any T >= 1; all pointers 16-byte aligned. */
int dhz_linear_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int T, int N, int K,
                   void* stream);
int dhz_linear_dgrad(const float* dy, int ldy, const float* w, float* dx, int ldx, int T, int N, int K, void* stream);
/*     dhz_linear_tile: which tile instance <WM, WN> the two entries above run for `rows` tokens and `out_features` output columns
 *     (N of the forward, K of the backward-data) under the current dhz_set_reserved_cus / dhz_set_deterministic state, as
 *     10 WM + WN; the last row tile is ragged where rows % (32 WM) != 0.  0 for a shape the entries refuse and for a width that
 *     takes the narrow kernel (a multiple of 16 but not of 32).  Host-side only; the dispatch asks the same function. */
int dhz_linear_tile(int rows, int out_features);

/* EXPERIMENT, off by default (dehaze_hip.ops.SPLIT_BF16 / bench.py --split-bf16; BASELINE configs[1] never takes it): the same two
 *     GEMMs with fp32 operands and results in HBM but the products on the bf16 matrix pipe, each operand split on its way into LDS
 *     into bf16 head + bf16 remainder and a.b taken as a_hi b_hi + a_hi b_lo + a_lo b_hi (~16 mantissa bits per product, fp32
 *     accumulation) - csrc/linear_split.hip.  terms = 3: as described; terms = 6: three pieces per operand (all 24 mantissa bits)
 *     and the six products down to 2^-16 - the error class of an fp32 GEMM at 6/16 of its matrix time.  N % 64 == 0, K % 64 == 0. */
int dhz_linear_fwd_split(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int T, int N, int K,
                         int terms, void* stream);
int dhz_linear_dgrad_split(const float* dy, int ldy, const float* w, float* dx, int ldx, int T, int N, int K, int terms,
                           void* stream);
/* The product's default form of the two GEMMs above (dehaze_hip.ops.SPLIT_BF16 == 6; csrc/split6_gemm.hip): the six-term split with
 *     the WEIGHT operand pre-split - w_hi / w_mid / w_lo are the three bf16 planes of w[N,K] (same layout, truncation pieces:
 *     hi + mid + lo == w exactly), written by dhz_split3_planes (one launch over the flat parameter buffer after every dhz_adamw_step; + dhz_split3_planes_t for W^T).  The
 *     activation operand is split inside the kernel.  fp32 activations, bias, accumulation and results; replaces the same
 *     aten::addmm / aten::mm as dhz_linear_fwd / dhz_linear_dgrad.  K % 32 == 0; N % 32 == 0 (forward), N % 32 == 0 and
 *     K % 64 == 0 (backward-data: its output features are w's K columns); planes 16-byte aligned. */
int dhz_linear_fwd_split6(const float* x, int ldx, const void* w_hi, const void* w_mid, const void* w_lo, const float* bias, float* y,
                          int ldy, int T, int N, int K, void* stream);
int dhz_linear_dgrad_split6(const float* dy, int ldy, const void* w_hi, const void* w_mid, const void* w_lo, float* dx, int ldx, int T,
                            int N, int K, void* stream);
/* K4 INSIDE the GEMM (csrc/tok_epilogue.h): the out-projection / linear2 product whose epilogue is the block's residual step -
 *     out[dst(t), :] = res[dst(t), :] + scale[t / tokens_per_image] * (x[t, :] . w^T + bias)
 *   windowed = 1: row t of x is a window slot (the order dhz_ln_partition_fwd writes: M1:846-852) and dst(t) is its token-order position
 *                 after window_reverse + roll(+shift)  =  attn out-projection + M1:859-868 + `shortcut + drop_path(x)` M1:872;
 *   windowed = 0: dst(t) = t                           =  LeFF linear2 / Mlp fc2 + `x + drop_path(mlp(norm2(x)))` M1:873.
 *   res == NULL adds nothing (with bias == NULL and windowed = 0 this is the per-image factor of a backward-data product:
 *   d(ctx) = scale . (d(out) . W_o), the DropPath factor of M1:872 in the backward pass); scale == NULL means 1.
 *   The GEMM result never exists in HBM in window order: replaces dhz_linear_fwd_split6 + dhz_reverse_residual_fwd.
 *   res / out: rows of ldo floats in token order; tokens_per_image (= Hres * Wres when windowed) a multiple of 64 dividing T whenever
 *   scale != NULL or windowed; Hres, Wres multiples of 8, 0 <= shift < 8.  Same shape contract as dhz_linear_fwd_split6 otherwise.
 *   _split_res / _dgrad_split_scaled: the same epilogue on the kernels of dhz_linear_fwd_split / dhz_linear_dgrad_split (few-tile shapes). */
int dhz_linear_fwd_split6_res(const float* x, int ldx, const void* w_hi, const void* w_mid, const void* w_lo, const float* bias,
                              const float* res, const float* scale, float* out, int ldo, int T, int N, int K, int tokens_per_image,
                              int Hres, int Wres, int shift, int windowed, void* stream);
/*     dhz_linear_split6_tile: which kernel dhz_linear_fwd_split6 / _split6_res (mode 1) or dhz_linear_dgrad_split6 (mode 2) runs for T
 *     tokens, N = w's rows, K = w's columns (mode 2 answers for K output features and contraction N, as the entry passes them) under
 *     the current dhz_set_reserved_cus / dhz_set_deterministic state: 10 (tile rows / 32) + tile columns / 32, i.e. 84 = 256 x 128,
 *     44 = 128 x 128, 42 = 128 x 64, 41 = 128 x 32; 0 for a shape the entry refuses.  Host-side only; the dispatch asks the same function. */
int dhz_linear_split6_tile(int mode, int T, int N, int K);
int dhz_linear_fwd_split_res(const float* x, int ldx, const float* w, const float* bias, const float* res, const float* scale, float* out,
                             int ldo, int T, int N, int K, int tokens_per_image, int Hres, int Wres, int shift, int windowed, int terms,
                             void* stream);
int dhz_linear_dgrad_split_scaled(const float* dy, int ldy, const float* w, const float* scale, float* dx, int ldx, int T, int N, int K,
                                  int tokens_per_image, int terms, void* stream);
/*   ... and on the bf16 kernels of BASELINE config 4 (dhz_linear_fwd_bf16): x, w, res, out in bf16, bias / scale fp32, fp32 accumulation;
 *   out = bf16(res + scale (x . w^T + bias)) - one rounding less than the two-launch form (the product is not rounded to bf16 first). */
int dhz_linear_fwd_bf16_res(const void* x, int ldx, const void* w, const float* bias, const void* res, const float* scale, void* out, int ldo,
                            int T, int N, int K, int tokens_per_image, int Hres, int Wres, int shift, int windowed, void* stream);
/*     hi[i] + mid[i] + lo[i] == src[i] exactly (three bf16 by truncation); n % 8 == 0, 16-byte aligned pointers. */
int dhz_split3_planes(const float* src, int64_t n, void* hi, void* mid, void* lo, void* stream);
/*     ... and the planes of the TRANSPOSES of nmat matrices inside one buffer: desc (device, int[nmat][4]) = {offset, rows R, cols C, index
 *     of the matrix's first 32 x 32 tile}; matrix m ([R][C] at src + offset) is written as [C][R] at the same offset of the planes.
 *     dx = dy . w is then dhz_linear_fwd_split6 on them (no bias): the backward-data GEMM without transposed fragment reads. */
int dhz_split3_planes_t(const float* src, void* hi, void* mid, void* lo, const int* desc, int nmat, int ntiles, void* stream);
/* bf16 (round to nearest even) copies of the TRANSPOSES of the same table of matrices: dst (bf16, as many elements as src) receives
 *     matrix m transposed at its own offset.  dhz_linear_fwd_bf16(dy, ldy, dst + off, NULL, dx, ldx, T, K, N) is then the backward-data
 *     product dx = dy . W of a Linear with weight W [N, K] (M1:487-492 under autocast) on the software-pipelined forward kernel. */
int dhz_bf16_transpose_batched(const float* src, void* dst, const int* desc, int nmat, int ntiles, void* stream);
/*     ... and the weight gradient (contract of dhz_linear_wgrad_multi + the row scale of dhz_linear_wgrad_rs: row_scale may be NULL;
 *     dw / db HOST arrays of nmat device pointers; ACCUMULATED; db exact fp32 column sums).  T % 64 == 0, nper % 64 == 0, K % 64 == 0. */
int dhz_linear_wgrad_split(const float* dy, int ldy, const float* x, int ldx, int T, int nmat, int nper, int K, float* const* dw,
                           float* const* db, const float* row_scale, int rows_per_scale, int terms, void* stream);
/*     The whole backward of such a Linear from ONE pass over dy (csrc/linear_bwd_pair.hip; fp32 storage, six-term products): replaces
 *         dhz_linear_fwd_split6(dy, ldy, planes of W^T, NULL, dx, K, T, K, N)          dx [T, K] = dy . W       (written in full)
 *         dhz_linear_wgrad_split(dy, ldy, x, ldx, T, nmat, nper, K, dw, db, NULL, 0, 6)  dw[m] += ..., db[m] += ...  (fp32 atomics)
 *     where dy [T, N = nmat * nper] is the wide tensor: dy and x are read and cut into bf16 pieces once.  wt_hi / mid / lo: the three
 *     planes of W^T ([K][N] row-major, W = the nmat matrices stacked; what dhz_split3_planes_t maintains).  dw / db: HOST arrays of nmat
 *     device pointers, db or any db[m] may be NULL.  Instances N x K = 128 x 32, 256 x 64, 192 x 64; T % 32 == 0; ldy, ldx multiples
 *     of 4; dy, x, the planes and dx 16-byte aligned; dx contiguous.  DHZ_EINVAL in deterministic mode (callers run the pair above).
 *     dhz_linear_bwd_pair_grid: the persistent grid of that launch under the current dhz_set_reserved_cus (each workgroup walks a
 *     contiguous slab of the T / 32 stages); 0 for a shape the entry refuses.  Host-side only. */
int dhz_linear_bwd_pair(const float* dy, int ldy, const float* x, int ldx, const void* wt_hi, const void* wt_mid, const void* wt_lo,
                        float* dx, int T, int nmat, int nper, int K, float* const* dw, float* const* db, void* stream);
int dhz_linear_bwd_pair_grid(int T, int N, int K);

/* bf16 forms of the three token-Linear GEMMs (BASELINE config 4: bf16 activations and bf16 weight copies, fp32 accumulation on
 *     v_mfma_f32_16x16x32_bf16; biases and all parameter gradients stay fp32).  Same contracts as dhz_linear_fwd / _dgrad /
 *     _wgrad_multi with bf16 token tensors (x, y, dy, dx) and a bf16 copy of w [N,K]; N % 64 == 0, K % 64 == 0, wgrad T % 64 == 0;
 *     token operands 16-byte aligned, leading dimensions multiples of 8 elements.  The reference runs this path under
 *     torch.cuda.amp.autocast (TR:224). */
int dhz_linear_fwd_bf16(const void* x, int ldx, const void* w, const float* bias, void* y, int ldy, int T, int N, int K,
                        void* stream);
int dhz_linear_dgrad_bf16(const void* dy, int ldy, const void* w, void* dx, int ldx, int T, int N, int K, void* stream);
int dhz_linear_wgrad_bf16(const void* dy, int ldy, const void* x, int ldx, int T, int nmat, int nper, int K,
                          float* const* dw, float* const* db, void* stream);

/* K5b Mlp activation (token_mlp = 'ffn', My_model_1.py:442-468 - the constructor default of Uformer; options.py selects 'leff'): y = GELU(u)
 *     (exact-erf form) over n elements; backward du = dy * GELU'(u) * scale[e / elems_per_scale] (scale NULL = 1: the per-image DropPath
 *     factor of the branch folded in).  Replaces aten::gelu / aten::gelu_backward between the two token Linears. */
int dhz_gelu_fwd_dt(const void* u, void* y, int64_t n, int dtype, void* stream);
int dhz_gelu_bwd_dt(const void* dy, const void* u, void* du, int64_t n, const float* scale, int64_t elems_per_scale, int dtype, void* stream);
/* dtype-generic forms (dtype = DHZ_F32 / DHZ_BF16 storage of the token tensors, fp32 arithmetic inside) of the streaming
 * kernels around the GEMMs; argument meaning as the fp32 entry points of the same name. */
int dhz_ln_partition_fwd_dt(const void* x, const float* gamma, const float* beta, void* xw, float* stats, int B, int Hres,
                            int Wres, int C, int shift, int partition, int dtype, void* stream);
int dhz_ln_partition_bwd_dt(const void* dxw, const void* x, const float* gamma, const float* stats, const void* dres, void* dx,
                            float* dgamma, float* dbeta, int B, int Hres, int Wres, int C, int shift, int partition, int dtype,
                            void* stream);
/* dhz_ln_partition_bwd_dt with the gradient LAYOUTS of a whole LeWin block's backward pass (M1:839-873 under autograd): the LeFF branch's
 * LayerNorm backward (partition = 0) writes dx in the window order of the attention branch (dx_windowed = 1, dx_shift = its shift) -
 * exactly the d(out) operand the out-projection's backward-data / weight-gradient products read, so no dhz_reverse_residual_bwd pass
 * runs - and the attention branch's LayerNorm backward (partition = 1) reads its residual gradient dres in that same order
 * (dres_windowed = 1).  dx_windowed needs Hres, Wres multiples of 8 and dx != dres. */
int dhz_ln_partition_bwd_lay(const void* dxw, const void* x, const float* gamma, const float* stats, const void* dres, void* dx,
                             float* dgamma, float* dbeta, int B, int Hres, int Wres, int C, int shift, int partition, int dres_windowed,
                             int dx_windowed, int dx_shift, int dtype, void* stream);
/* ... with a SECOND output: dx2 (may be NULL) receives scale2[image] * dx in the window order of dx_shift (scale2 NULL = 1) - the scaled,
 * window-ordered d(out) operand of the out-projection's backward products for storage types whose GEMMs take no row factor (bf16). */
int dhz_ln_partition_bwd_lay2(const void* dxw, const void* x, const float* gamma, const float* stats, const void* dres, void* dx,
                              float* dgamma, float* dbeta, int B, int Hres, int Wres, int C, int shift, int partition, int dres_windowed,
                              int dx_windowed, int dx_shift, void* dx2, const float* scale2, int dtype, void* stream);
int dhz_reverse_residual_fwd_dt(const void* yw, const void* shortcut, const float* scale, void* out, int B, int Hres, int Wres,
                                int C, int shift, int partition, int dtype, void* stream);
int dhz_reverse_residual_bwd_dt(const void* dout, const float* scale, void* dyw, int B, int Hres, int Wres, int C, int shift,
                                int partition, int dtype, void* stream);
int dhz_leff_dwconv_fwd_dt(const void* u, const float* w, const float* b, void* t, void* z, int B, int Hres, int Wres, int Ch,
                           int dtype, void* stream);
int dhz_leff_dwconv_bwd_dt(const void* dz, const void* u, const void* t, const float* w, void* du, float* dw, float* db, int B,
                           int Hres, int Wres, int Ch, int dtype, void* stream);
/*      the same with dz multiplied by dz_scale[b] per image on the way in (the DropPath scale of M1:873 folded into this kernel;
 *      dz_scale NULL = 1) */
int dhz_leff_dwconv_bwd_scaled_dt(const void* dz, const void* u, const void* t, const float* w, void* du, float* dw, float* db,
                                  const float* dz_scale, int B, int Hres, int Wres, int Ch, int dtype, void* stream);
/*      the same with dz FORMED IN THE KERNEL from linear2's output gradient (fp32 storage; csrc/leff_dwconv_dz.hip): replaces
 *          dz = dy @ W2                                   (at::mm; [T, C] x [C, Ch], written and read once)
 *          dhz_leff_dwconv_bwd_scaled_dt(dz, ...)
 *      dy: [B Hres Wres, C] in token order with row stride ldy (ldy % 4 == 0, ldy >= C); w2t_hi / mid / lo: the three bf16 truncation
 *      planes of W2^T ([Ch][C] row-major, what dhz_split3_planes writes for W2.t().contiguous() and dhz_split3_planes_t maintains); the
 *      product is the six-term one on the bf16 matrix pipe, fp32 accumulation.  C in {32, 64, 128}, Ch % 32 == 0.  dw / db accumulate. */
int dhz_leff_dwconv_bwd_dy(const float* dy, int ldy, const void* w2t_hi, const void* w2t_mid, const void* w2t_lo, const float* u,
                           const float* tpre, const float* wd, float* du, float* dw, float* db, const float* dz_scale, int B, int Hres,
                           int Wres, int C, int Ch, void* stream);
int dhz_ps_attn_fwd_dt(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias,
                       const float* mask, void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d, int dtype,
                       void* stream);
int dhz_ps_attn_bwd_dt(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask,
                       const uint8_t* rank, const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg,
                       float* dbias_part, int B_, int H, int nW, int d, int dtype, void* stream);
/*      ... with the padding mask of any-size evaluation (M1:791-800) as one uint64 per window instead of a [B_, 64, 64] tensor: replaces
 *          am = window_partition(F.interpolate(mask, (H, W))); am = am[:, :, None] * am[:, None, :]
 *          attn_mask = am.masked_fill(am != 0, -100) (+ shift_mask)                 -> ProbAttention.forward(..., attn_mask)
 *      pad[B_]: bit j of word b = token j of GLOBAL window b is padding (dhz_pad_window_bits); mask stays the [nW, 64, 64] shift mask
 *      (window b % nW) or NULL.  B_ must be a whole number of images (B_ % nW == 0, nW > 0 also without a shift mask).  The kernels add
 *      (shift term + padding term), both exact, where they add the mask: bit-identical to the entries above given the summed tensor.  The
 *      backward needs the words only to recompute P. */
int dhz_ps_attn_fwd_dt_pad(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias, const float* mask,
                           const uint64_t* pad, void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d, int dtype, void* stream);
int dhz_ps_attn_bwd_dt_pad(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask, const uint64_t* pad,
                           const uint8_t* rank, const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg, float* dbias_part, int B_,
                           int H, int nW, int d, int dtype, void* stream);

/* K2/K4/K5 (backward)  weight + bias gradient of every token-major nn.Linear on the path
 *     (query/key/value/out projections ATT:420-422,454-458; LeFF linear1/linear2 M1:487-492):
 *     dw[N,K] += dy^T[N,T] . x[T,K]        db[N] += sum_t dy[t,:]        (ACCUMULATED: caller zeroes,
 *     which lets the gradients land directly in the optimizer's flat gradient buffer).
 *     dy: [T,N] with row stride ldy, x: [T,K] with row stride ldx; T % 16 == 0 (tokens in 16s: a 4x4 map has 16 per image), N % 16 == 0,
 *     K % 16 == 0.  Rows at or beyond T are never read: dy and x may end at row T of their allocation.  db may be NULL.  Default mode: the token slabs meet in fp32 atomics, the summation order over T is not deterministic and the slab count
 *     follows the CU count.  Deterministic mode (dhz_set_deterministic): slabs cut by the shape alone, stored and summed in slab order. */
int dhz_linear_wgrad(const float* dy, int ldy, const float* x, int ldx, int T, int N, int K,
                     float* dw, float* db, void* stream);
/*      Same contraction for nmat (1..4) parameters that share the input x - the Q / K / V projections of
 *      AttentionLayer.forward (ATT:385-461): columns [i*nper, (i+1)*nper) of dy belong to dw[i] / db[i] (HOST arrays of
 *      nmat device pointers; db may be NULL, or all of its entries NULL).  One launch reads x once instead of nmat times.
 *      T % 16 == 0 as above; rows at or beyond T are never read. */
/*      dhz_linear_wgrad with row t of dy multiplied by row_scale[t / rows_per_scale] on the way in (per-image DropPath scale of the
 *      branch output; rows_per_scale a multiple of 32 that divides T - with a row scale T therefore stays in 32s; row_scale NULL =
 *      plain dhz_linear_wgrad, tokens in 16s; rows at or beyond T are never read). */
int dhz_linear_wgrad_rs(const float* dy, int ldy, const float* x, int ldx, int T, int N, int K, float* dw, float* db,
                        const float* row_scale, int rows_per_scale, void* stream);
int dhz_linear_wgrad_multi(const float* dy, int ldy, const float* x, int ldx, int T, int nmat, int nper, int K,
                           float* const* dw, float* const* db, void* stream);

/* K11  3x3 / stride 1 / pad 1 convolution of the VGG19 feature stack (My_CR.py:56-86) as Winograd F(2x2,3x3) on the
 *      fp32 matrix pipe.  Tensors are channel-blocked NCHW8c: x[b][c/8][h][w][c%8] (dhz_layout_blocked8 converts).
 *      dhz_winograd_prepack: weight [Kout,Cin,3,3] -> transform-domain filters upack (16*Kout*Cin floats);
 *        transposed_rot != 0 builds the backward-data filters from the forward weight [Cin,Kout,3,3] (the roles of
 *        the two channel counts swap, taps rotate by 180 degrees).  The VGG weights are frozen: prepack once.
 *      dhz_winograd_conv3x3: forward  y = conv(x, W) [+ bias] [ReLU]                (out_mask = out_addend = NULL)
 *                            backward y = out_mask > 0 ? conv(x, W') + out_addend : 0   (bias = NULL, relu = 0)
 *        where W' are the backward-data filters, out_mask (shape of y, may be NULL) is the saved post-ReLU activation
 *        at the OUTPUT positions - the ReLU of the layer below, fused into the store - and out_addend (shape of y, may
 *        be NULL) the gradient reaching that activation from a loss tap.
 *        H % 16 == 0 and W % 16 == 0, or H == W == 8 (the conv5_1 geometry of 128 x 128 patches: four images share one
 *        16 x 16 block of the kernel); C % 8 == 0, K % 32 == 0.  Every other map size: dhz_winograd_conv3x3_any (K11d).
 *      dhz_maxpool2x2_blocked_fwd / _bwd: the 2x2/stride-2 max pooling between VGG stages in the same layout
 *        (N = B*C/8 planes of [H][W][8]); the backward routes gy to the first maximum of each window of the saved
 *        post-ReLU map `act` and applies that map's ReLU (act > 0) in the same pass. */
int dhz_winograd_prepack(const float* weight, float* upack, int Kout, int Cin, int transposed_rot, void* stream);
int dhz_winograd_conv3x3(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                         const float* out_addend, float* y, int B, int H, int W, int C, int K, void* stream);
/* K11b The same convolution as Winograd F(4x4,3x3) (round 5; csrc/winograd43_conv.hip): 36 transform-domain products per 16 outputs
 *      instead of 16 per 4.  Same tensors, same epilogues, same argument meaning as the two entry points above; upack holds
 *      36*Kout*Cin floats.  H % 16 == 0, W % 16 == 0 (maps of 16 x 16 and more: the 8 x 8 layer stays on dhz_winograd_conv3x3),
 *      C % 16 == 0, K % 32 == 0 (a workgroup owns 32 output channels; other K: DHZ_EINVAL).  Interpolation points (0, +-3/4, +-3/2, inf),
 *      filters transformed in double.  Input channels are accumulated in the transform domain in chains of 256: C <= 256 is one launch;
 *      C > 256 runs as chained launches over 256-channel slices in which y carries the partial sums (READ and written by every launch
 *      but the first; bias / relu / out_mask / out_addend applied by the last) - ~2x the rounding error of F(2x2,3x3), inside the same
 *      test tolerances. */
int dhz_winograd43_prepack(const float* weight, float* upack, int Kout, int Cin, int transposed_rot, void* stream);
int dhz_winograd43_conv3x3(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                           const float* out_addend, float* y, int B, int H, int W, int C, int K, void* stream);
/* ... + bias + ReLU + 2 x 2 / stride-2 max pooling in the same launch (replaces F.relu(conv2d) followed by nn.MaxPool2d(2, 2) of the VGG19
 * slices, My_CR.py:60-86, where the un-pooled map is not a tap): ypool [B][K/8][H/2][W/2][8].  scratch: full-resolution map
 * [B][K/8][H][W][8], needed only for C > 256 (partial sums of the accumulation chains), may be NULL otherwise. */
int dhz_winograd43_conv3x3_pool(const float* x, const float* upack, const float* bias, float* ypool, float* scratch, int B, int H, int W,
                                int C, int K, void* stream);
/* K11c Channel slices for launches whose grid leaves CUs idle (the 8 x 8 and 16 x 16 maps of a 128 x 128 patch): the input-channel
 *      contraction is cut into `slices` ranges of 8-channel groups, ONE grid of slices x (the plain grid) workgroups leaves the raw sums of
 *      slice s in part s of workspace (slices * B * K * H * W floats, contents undefined before and after), and a second kernel adds the
 *      parts in a fixed order - r = p_0 + ... + p_{S-2}, then (p_{S-1} + bias) + r - and applies the store epilogue (bias / ReLU, or
 *      out_mask / out_addend).  No atomics: the same bits from run to run.  Other arguments as dhz_winograd_conv3x3 / dhz_winograd43_conv3x3.
 *      dhz_winograd_conv3x3_slices: 1 <= slices <= C / 8 (uneven ranges allowed); slices == 1 is dhz_winograd_conv3x3 bit for bit and
 *        takes no workspace; slices > 1 with a null workspace: DHZ_EINVAL.
 *      dhz_winograd43_conv3x3_slices: slices >= 2, (C / 8) % slices == 0 and C / slices <= 256: every slice is one accumulation-chain link.
 *        Two slices of 512 channels give the bits of dhz_winograd43_conv3x3 (the same links, added in the same order).
 *      dhz_winograd_slices: the slice count the library recommends for dhz_winograd_conv3x3_slices - the largest S in {1, 2, 4} with
 *        S x grid <= physical CUs (dhz_grid_cus() + dhz_get_reserved_cus(): these grids are not persistent) and at least 16 channel groups
 *        per slice; 1 = the plain launch (also for a shape the entry refuses).  Host-side only. */
int dhz_winograd_conv3x3_slices(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                                const float* out_addend, float* y, float* workspace, int slices, int B, int H, int W, int C, int K,
                                void* stream);
int dhz_winograd43_conv3x3_slices(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                                  const float* out_addend, float* y, float* workspace, int slices, int B, int H, int W, int C, int K,
                                  void* stream);
int dhz_winograd_slices(int B, int H, int W, int C, int K);
/* K11d The F(2x2,3x3) convolution on maps of ANY size (H, W >= 1; C % 8 == 0, K % 32 == 0): what lets the feature stack run patches whose
 *      maps are no multiples of 16 (64, 192, 240, 384 pixels ...).  Same filters (dhz_winograd_prepack), same epilogues, same error codes as
 *      dhz_winograd_conv3x3.  How the kernel's 16 x 16 blocks lie on the maps:
 *        4 x 4                      sixteen images per block (4 x 4 arrangement; a partly filled last block stores only its own images)
 *        8 x 8                      four images per block   - the launch of dhz_winograd_conv3x3, bit for bit
 *        H % 16 == 0, W % 16 == 0   whole blocks            - the launch of dhz_winograd_conv3x3, bit for bit
 *        everything else            ceil(H / 16) x ceil(W / 16) ragged blocks per image: pixels outside the map are zero padding on the way in
 *                                   and are neither stored nor read (out_mask / out_addend) on the way out.
 *      dhz_winograd_conv3x3_any_slices: dhz_winograd_conv3x3_slices on the same shapes (slices == 1 is dhz_winograd_conv3x3_any bit for bit).
 *      dhz_winograd_slices_any: the rule of dhz_winograd_slices (same constants) on the block count of the launch above; 1 for a shape the
 *        entry refuses.  dhz_winograd_any_blocks: that block count - ceil(B / 16) at 4 x 4, ceil(B / 4) at 8 x 8, B ceil(H / 16) ceil(W / 16)
 *        otherwise; <= 0 on bad arguments.  Both host-side only.
 *      The LeakyReLU entry (K11a) and the F(4x4,3x3) kernel (K11b) keep their contracts. */
int dhz_winograd_conv3x3_any(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                             const float* out_addend, float* y, int B, int H, int W, int C, int K, void* stream);
int dhz_winograd_conv3x3_any_slices(const float* x, const float* upack, const float* bias, int relu, const float* out_mask,
                                    const float* out_addend, float* y, float* workspace, int slices, int B, int H, int W, int C, int K,
                                    void* stream);
int dhz_winograd_slices_any(int B, int H, int W, int C, int K);
int dhz_winograd_any_blocks(int B, int H, int W);
int dhz_maxpool2x2_blocked_fwd(const float* x, float* y, int N, int H, int W, void* stream);
int dhz_maxpool2x2_blocked_bwd(const float* gy, const float* act, float* gx, int N, int H, int W, void* stream);
int dhz_layout_blocked8(const float* src, float* dst, int B, int C, int HW, int to_blocked, const float* bias, int relu,
                        void* stream);   /* towards the blocked layout optionally dst = max(src + bias[c], 0) */

/* K11a dhz_winograd_conv3x3 with LeakyReLU(0.01) in its store: the Conv2d(3x3, pad 1) + LeakyReLU pairs of the UNet baseline's ConvBlock
 *      and their autograd (M1:28-40: aten::convolution + aten::leaky_relu_, the `+ conv11(x)` of M1:40, aten::leaky_relu_backward +
 *      aten::convolution_backward's input gradient) without an elementwise pass over the map.  Same tensors, layout and shape contract
 *      as dhz_winograd_conv3x3 (upack from dhz_winograd_prepack).
 *        backward == 0:  y = leaky(conv(x, W) + bias) + out_addend    (bias, out_addend may be NULL; out_mask must be NULL)
 *        backward != 0:  y = (conv(x, W') + out_addend) * (out_mask > 0 ? 1 : 0.01)   with W' the backward-data filters and out_mask the
 *                        saved LeakyReLU output at the OUTPUT positions, whose sign is the pre-activation's (bias must be NULL).  With an
 *                        out_addend the forward's y is not that activation: a caller that needs the sign later keeps the addend out of this
 *                        store (dehaze_hip/unet.py adds conv11(x) in dhz_blocked8_to_tokens).
 *      There is no F(4x4,3x3) instance of this entry. */
int dhz_winograd_conv3x3_act(const float* x, const float* upack, const float* bias, int backward, const float* out_mask,
                             const float* out_addend, float* y, int B, int H, int W, int C, int K, void* stream);

/*      Layout changes between tokens [B][HW][C] (row stride ld floats, ld % 4 == 0) and the blocked layout [B][C/8][HW][8], C % 8 == 0,
 *      16-byte aligned pointers, with the elementwise factors of a ConvBlock (M1:28-40) folded into the copy:
 *      dhz_tokens_to_blocked8: blk = tok * (leaky_mask > 0 ? 1 : 0.01) - the aten::leaky_relu_backward of a gradient on its way to the
 *        backward-data and weight-gradient kernels; leaky_mask (blocked, the saved LeakyReLU output) may be NULL: a plain copy.
 *      dhz_blocked8_to_tokens: tok = blk + addend (tokens with row stride ld_add; may be NULL) - the `+ conv11(x)` of M1:40. */
int dhz_tokens_to_blocked8(const float* tok, int ld, const float* leaky_mask, float* blk, int B, int HW, int C, void* stream);
int dhz_blocked8_to_tokens(const float* blk, const float* addend, int ld_add, float* tok, int ld, int B, int HW, int C, void* stream);

/* K11w Weight and bias gradient of a dense 3x3 / stride 1 / pad 1 convolution (csrc/conv3x3_wgrad.hip) in the same channel-blocked layout
 *      as K11, so that forward, backward-data and weight gradient of a layer share their maps without a repacking pass.  Replaces the
 *      weight / bias outputs of aten::convolution_backward that autograd runs for the nn.Conv2d(C, K, 3, padding=1) layers of the UNet
 *      baseline's ConvBlock (M1:28-40; the VGG filters of K11 are frozen and never needed it).
 *        x  [B][Cin/8][H][W][8], dy [B][Kout/8][H][W][8];  dw [Kout][Cin][3][3] and db [Kout] (may be NULL) are WRITTEN, not accumulated:
 *        dw[k][c][r][s] = sum_{b,h,w} dy[b][k][h][w] x[b][c][h+r-1][w+s-1],  db[k] = sum dy[b][k][h][w].  The zero padding around the map is
 *        never read: x may begin and end with its allocation.
 *        Cin and Kout multiples of 32, up to 512; H and W multiples of 16, or H == W == 8; any B >= 1; anything else DHZ_EINVAL before
 *        any launch.
 *      The contraction over B*H*W is cut into dhz_conv3x3_wgrad_parts(...) slabs of whole 64-position chunks (4 rows x 16 columns, or one
 *      8 x 8 image; B*(H/4)*(W/16) or B chunks), accumulated in fp32 on the fp32 matrix pipe by a persistent grid, stored to the workspace
 *      and summed in slab order by a second kernel.  No atomics; the cut depends on the shapes alone: the same bits from run to run, under
 *      any dhz_set_reserved_cus, with the deterministic mode on or off.
 *      ws: dhz_conv3x3_wgrad_workspace_bytes(...) bytes of device memory (contents undefined before and after; 0 for an unsupported
 *      shape).  With dhz_set_deterministic on, the mode's workspace (dhz_set_det_workspace) is used instead and ws may be NULL. */
size_t dhz_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Kout);
int dhz_conv3x3_wgrad_parts(int B, int H, int W, int Cin, int Kout);
int dhz_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, float* ws, size_t ws_bytes, int B, int H, int W, int Cin,
                      int Kout, void* stream);
/*      The same on maps of ANY size (H, W >= 1; the channel constraints, the tensors, the workspace rules and the error codes are those
 *      above): what lets FFA-Net's 64 -> 64 layers train and be scored on whole images.  How the 64-position chunks lie on the maps:
 *        8 x 8                      one image per chunk        - the launch of dhz_conv3x3_wgrad, bit for bit
 *        H % 16 == 0, W % 16 == 0   whole 4 x 16 chunks        - the launch of dhz_conv3x3_wgrad, bit for bit
 *        everything else            ceil(H / 4) x ceil(W / 16) chunks per image, B ceil(H / 4) ceil(W / 16) in all (times 64 must fit an
 *                                   int): dy positions outside the map are zeros in LDS and never loaded, like the x halo, so they add
 *                                   zero to dw and db.
 *      The slab rule is the one above - min(ceil(512 / tiles), chunks / 4), at least 1 - on that chunk count.
 *      dhz_conv3x3_wgrad_workspace_bytes_any / dhz_conv3x3_wgrad_parts_any: the two queries for these shapes (equal to the queries above
 *      wherever those answer; 0 for a shape this entry refuses). */
size_t dhz_conv3x3_wgrad_workspace_bytes_any(int B, int H, int W, int Cin, int Kout);
int dhz_conv3x3_wgrad_parts_any(int B, int H, int W, int Cin, int Kout);
int dhz_conv3x3_wgrad_any(const float* x, const float* dy, float* dw, float* db, float* ws, size_t ws_bytes, int B, int H, int W, int Cin,
                          int Kout, void* stream);

/* K9b  output projection (My_model_1.py:696-723): Conv2d(C -> 3, 3x3, pad 1) from tokens x[B, H*W, C] to an NCHW image
 *      y[B, 3, H, W] (+ bias[3], may be NULL); backward-data dx[B, H*W, C] from dy[B, 3, H, W]; weight / bias gradient
 *      dw[3, C, 3, 3], db[3] (ACCUMULATED; db may be NULL).  w is the layer's own [3, C, 3, 3] tensor.  C in {64, 128}. */
int dhz_thin_conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, void* stream);
int dhz_thin_conv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int C, void* stream);
int dhz_thin_conv3x3_wgrad(const float* dy, const float* x, float* dw, float* db, int B, int H, int W, int C, void* stream);
/* the same with the token tensors (x, dx) stored as `dtype` (DHZ_F32 / DHZ_BF16; images, weights and gradients fp32) */
int dhz_thin_conv3x3_fwd_dt(const void* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, int dtype,
                            void* stream);
int dhz_thin_conv3x3_dgrad_dt(const float* dy, const float* w, void* dx, int B, int H, int W, int C, int dtype, void* stream);
int dhz_thin_conv3x3_wgrad_dt(const float* dy, const void* x, float* dw, float* db, int B, int H, int W, int C, int dtype,
                              void* stream);
/*      backward-data of a 3 -> C convolution (the first VGG19 layer, My_CR.py:65) from a channel-blocked gradient
 *      gb[B, C/8, H, W, 8] and that layer's weight w[C, 3, 3, 3]: dx[B, 3, H, W].  C = 64. */
/*      the same layer forward: y[B, K/8, H, W, 8] (channel-blocked) = max(conv(x[B, 3, H, W], w[K, 3, 3, 3]) + bias, 0 if relu).
 *      K = 64. */
int dhz_conv3x3_in3_blocked(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int K, int relu,
                            void* stream);
int dhz_thin_conv3x3_dgrad_blocked(const float* gb, const float* w, float* dx, int B, int H, int W, int C, void* stream);

/* K11b the two L1 distances of one ContrastLoss feature tap (My_CR.py:108-112): sums[0] += sum|a-p|, sums[1] += sum|a-n|
 *      (n may be NULL: ablation, My_CR.py:114-119); backward da = (g[0] sign(a-p) + g[1] sign(a-n)) / count with g the
 *      device-resident gradients of the two MEANS.  count % 4 == 0; any (common) element order. */
int dhz_l1_pair_fwd(const float* a, const float* p, const float* n, float* sums, int64_t count, void* stream);
int dhz_l1_pair_bwd(const float* a, const float* p, const float* n, const float* g, float* da, int64_t count, void* stream);

/* K11d the squared error of one feature tap of FFA-Net's perceptual loss (FFA_model/models/PerceptualLoss.py:24-31: F.mse_loss of the
 *      VGG16 features at relu1_2 / relu2_2 / relu3_3), csrc/perceptual.hip:
 *      dhz_mse_pair_fwd: sum[0] += sum (a - g)^2 (the caller zeroes, the kernel accumulates; deterministic mode: workspace slots and
 *        dhz_det_reduce, no atomic).  dhz_mse_pair_bwd: da = gmean[0] (2 / count) (a - g) with gmean the device-resident gradient of the
 *        MEAN; relu_mask != 0: da = 0 where a <= 0 (a is a post-ReLU map: the gradient below that ReLU).
 *        count > 0, count % 4 == 0, a / g / da 16-byte aligned (DHZ_EINVAL otherwise); any (common) element order; fp32 only.
 *      dhz_maxpool2x2_blocked_bwd_add: dhz_maxpool2x2_blocked_bwd for a post-ReLU map `act` that is a loss tap as well:
 *        gx = act > 0 ? (gy routed to the first maximum of each window) + addend : 0, addend [N][H][W][8] the tap's own gradient. */
int dhz_mse_pair_fwd(const float* a, const float* g, float* sum, int64_t count, void* stream);
int dhz_mse_pair_bwd(const float* a, const float* g, const float* gmean, float* da, int64_t count, int relu_mask, void* stream);
int dhz_maxpool2x2_blocked_bwd_add(const float* gy, const float* act, const float* addend, float* gx, int N, int H, int W,
                                   void* stream);

/* K11e whole images (the reference's default, FFA_model/data_utils.py:21: crop_size = 'whole_img'): the three poolings of the blocked layout
 *      and the L1 mean on ANY size.  fp32 only.
 *      dhz_maxpool2x2_blocked_fwd_any / _bwd_any / _bwd_add_any: the entries of the same name without `_any` for any H, W >= 2 (DHZ_EINVAL
 *        below, before a launch), floor mode as nn.MaxPool2d(2, 2): x / act / addend / gx [N][H][W][8], y / gy [N][H / 2][W / 2][8]; an odd
 *        last row or column feeds no window.  The two backward entries write EVERY element of gx: inside the windows the routing above
 *        (first maximum, through the ReLU act > 0); on the dropped row / column gx = 0 (_bwd_any) or gx = act > 0 ? addend : 0
 *        (_bwd_add_any: the tap's own gradient alone).  Maps 16-byte aligned.  On even H, W the bits of the entries above.  No atomics.
 *      dhz_l1_pair_fwd_any / _bwd_any: K11b for any count >= 1 and 4-byte aligned pointers: a float4 body from the first element at which
 *        all pointers are 16-byte aligned (none when they never are together), the elements before and behind it one by one.  Same
 *        accumulation as K11b (one partial per workgroup, fp32 atomics or, in deterministic mode, workspace slots and dhz_det_reduce;
 *        the cut into workgroups is a function of count and of the pointers' alignment); where K11b applies (count % 4 == 0, 16-byte
 *        aligned pointers), the same launch geometry and the same bits per workgroup. */
int dhz_maxpool2x2_blocked_fwd_any(const float* x, float* y, int N, int H, int W, void* stream);
int dhz_maxpool2x2_blocked_bwd_any(const float* gy, const float* act, float* gx, int N, int H, int W, void* stream);
int dhz_maxpool2x2_blocked_bwd_add_any(const float* gy, const float* act, const float* addend, float* gx, int N, int H, int W,
                                       void* stream);
int dhz_l1_pair_fwd_any(const float* a, const float* p, const float* n, float* sums, int64_t count, void* stream);
int dhz_l1_pair_bwd_any(const float* a, const float* p, const float* n, const float* g, float* da, int64_t count, void* stream);

/* K10b the same feature stack for BASELINE config 4 (bf16 feature maps in NHWC / token layout [N, H, W, C]; what torch.autocast
 *      makes of My_CR.py:65-72's convolutions), csrc/vgg_bf16.hip:
 *      dhz_vgg_prepack_bf16: filter w[K, C, 3, 3] fp32 -> bf16 [K][9 C] tap-major (transpose = 0) or the backward-data filter
 *        [C][9 K] with the taps rotated by 180 degrees (transpose = 1).
 *      dhz_vgg_conv3x3_bf16: y[N, H, W, Cout] = conv3x3(x[N, H, W, Cin], pad 1) as an implicit GEMM on the bf16 matrix pipe
 *        (fp32 accumulation); forward y = max(. + bias, 0 if relu); backward-data (bias NULL, relu 0, wp the transposed pack)
 *        y = act > 0 ? . + addend : 0 with act (may be NULL) the saved post-ReLU map at the OUTPUT positions and addend (may be
 *        NULL; needs act) the gradient reaching that map from its loss tap.  Cin a power of two >= 64, Cout % 64 == 0.
 *      dhz_maxpool2x2_nhwc_bf16_fwd / _bwd: 2x2 / stride-2 max pooling; the backward routes gy to the first maximum of each
 *        window of the saved post-ReLU map `act` and applies act > 0.  C % 8 == 0.
 *      dhz_l1_pair_fwd_bf16 / _bwd_bf16: K11b on bf16 maps (fp32 sums; da in bf16).  count % 8 == 0. */
int dhz_vgg_prepack_bf16(const float* w, void* out, int K, int C, int transpose, void* stream);
int dhz_vgg_conv3x3_bf16(const void* x, const void* wp, const float* bias, int relu, const void* act, const void* addend, void* y,
                         int N, int H, int W, int Cin, int Cout, void* stream);
int dhz_maxpool2x2_nhwc_bf16_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream);
int dhz_maxpool2x2_nhwc_bf16_bwd(const void* gy, const void* act, void* gx, int N, int H, int W, int C, void* stream);
int dhz_l1_pair_fwd_bf16(const void* a, const void* p, const void* n, float* sums, int64_t count, void* stream);
int dhz_l1_pair_bwd_bf16(const void* a, const void* p, const void* n, const float* g, void* da, int64_t count, void* stream);

/* K11c the scalar side of ContrastLoss.forward (My_CR.py:104-123) over k feature taps: d[i] = (ap_i, an_i) = sums[i] * inv_cnt[i];
 *      out = (sum_i w_i ap_i / (an_i + 1e-7)  [ablation: sum_i w_i ap_i],  sum_i ap_i,  sum_i an_i).  Backward: g[i] = gradient of
 *      (out . (g_loss, g_ap, g_an)) w.r.t. (ap_i, an_i); a NULL upstream gradient counts as zero.  Replaces the [k]-vector
 *      mul / div / add / sum chain of torch ops.  1 <= k <= 64; all pointers device memory. */
int dhz_contrast_combine_fwd(const float* sums, const float* inv_cnt, const float* w, int k, int ablation, float* d, float* out,
                             void* stream);
int dhz_contrast_combine_bwd(const float* d, const float* w, int k, int ablation, const float* g_loss, const float* g_ap,
                             const float* g_an, float* g, void* stream);

/* F2  training feed (dataset.py:17-77, FFA_model/data_utils.py:51-81): batch item t -> an h x w crop of a uint8 HWC (RGB) image pair in HBM,
 *     one of eight rotate / flip maps, float32 [n,3,h,w] = value / 255 for the clear (out_gt) and the hazy (out_hazy) image.  Five entries,
 *     one kernel; they differ in the row format that carries an item's geometry and in whether MixUp is formed in the same launch.
 *     Table rows (`table`, device memory, 4 int per item): (image id, r, c, k) - the crop at (r, c) of image id of two uint8 [N,Hs,Ws,3]
 *       stores.  h <= Hs, w <= Ws (h = Hs, w = Ws: whole images); the caller keeps r + h <= Hs and c + w <= Ws.
 *     Descriptor rows (`desc`, device memory, DHZ_RAGGED_DESC_WORDS int64 per item, computed on the host) - images that each have their own
 *       size, what data_utils.py:51-81 does per item on the host (PIL open, CenterCrop of the clear frame, RandomCrop, flip / rotate,
 *       ToTensor, Normalize).  gt_pool / hazy_pool are uint8 pools, every image HWC at its own offset; a pool may exceed 4 GiB, all
 *       addresses are formed in 64 bits.
 *       [0] pixel offset (bytes / 3) in hazy_pool of the crop's origin: image base + r * hazy stride + c
 *       [1] hazy row stride in pixels (the hazy image's width)
 *       [2] pixel offset in gt_pool of the crop's origin: image base + (top + r) * clear stride + left + c, (top, left) the centre-crop
 *           origin of the larger clear frame
 *       [3] clear row stride in pixels (the clear image's width)
 *       [4] the map k
 *       The entry cannot see the images' sizes: the caller keeps every crop inside its image (dataset.ImageStoreHBM.batch checks it).
 *     Map k, 0..7, of utils/dataset_utils.py:6-40: 0 id, 1-3 rot90 k with dims=[-1,-2], 4-7 the same followed by flip(-2).  For h != w only
 *       the four shape-preserving maps exist and the kernel reads k & 6 (0 id, 2 rot180, 4 flip(-2), 6 flip(-1)); for h == w all eight.
 *     norm (descriptor entries): NULL, or six floats in HOST memory (mean[3], std[3]) read during the call; then out_hazy =
 *       ((float)v / 255.f - mean[ch]) / std[ch], two IEEE operations after the division (ToTensor + Normalize in fp32); out_gt is never
 *       normalised.
 *     MixUp (`_mix` entries; utils/dataset_utils.py:39-45, My_train.py from epoch 6 on): with A[t] what the entry of the same name without
 *       `_mix` writes for item t - crop, map k, / 255.f, on the hazy output the normalisation -,
 *         out[t] = lam[t] * A[t] + (1 - lam[t]) * A[partner[t]]
 *       as FOUR fp32 operations, each rounded once (1 - lam, two products, one sum; no FMA): bit for bit ATen's
 *       `lam * x + (1 - lam) * x[partner]` on the outputs of the plain entries; norm is applied to either hazy value BEFORE the mix.
 *       partner and lam travel in the rows, lam as the bit pattern of its fp32 value, so a batch still costs one upload: table rows of
 *       DHZ_MIX_TABLE_WORDS int, (id, r, c, k, partner, lam bits); descriptor rows of DHZ_RAGGED_MIX_DESC_WORDS int64, the five words
 *       above, then [5] partner, [6] lam bits in the low 32 bits.  The device cannot check partner: the caller keeps 0 <= partner < n.
 *     Every entry refuses, before a launch, a null pointer, sizes that are not positive or exceed the store, and n * h * w >= 2^31.
 *     dhz_crop_augment_pair: table rows, the ps x ps crop - dhz_crop_augment_pair_rect with h = w = ps, bit for bit.  (It used to launch
 *       whatever n * ps * ps it was given; two float32 outputs of 8 GiB and more each are now refused like everywhere else.)
 *     dhz_crop_augment_pair_rect, dhz_crop_augment_mix_pair_rect (square crops go through it with h == w): table rows.
 *     dhz_crop_augment_pair_ragged, dhz_crop_augment_mix_pair_ragged: descriptor rows; position for position the rect entries' output. */
#define DHZ_RAGGED_DESC_WORDS 5
#define DHZ_MIX_TABLE_WORDS 6
#define DHZ_RAGGED_MIX_DESC_WORDS 7
int dhz_crop_augment_pair(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                          int n, int Hs, int Ws, int ps, void* stream);
int dhz_crop_augment_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                               int n, int Hs, int Ws, int h, int w, void* stream);
int dhz_crop_augment_mix_pair_rect(const uint8_t* gt, const uint8_t* hazy, const int* table, float* out_gt, float* out_hazy,
                                   int n, int Hs, int Ws, int h, int w, void* stream);
int dhz_crop_augment_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt, float* out_hazy,
                                 const float* norm, int n, int h, int w, void* stream);
int dhz_crop_augment_mix_pair_ragged(const uint8_t* gt_pool, const uint8_t* hazy_pool, const int64_t* desc, float* out_gt, float* out_hazy,
                                     const float* norm, int n, int h, int w, void* stream);
/*     dhz_gather_mix_pair: the same for pairs that are resident as float32 [N, per_item] tensors (My_train.py --synthetic, .pt files).
 *     table: device memory, rows of DHZ_GATHER_MIX_TABLE_WORDS int64, (source item, partner, lam bits in the low 32 bits).  mix == 0:
 *     out[t] = src[source[t]], a plain gather of both tensors in one launch; mix != 0: lam[t] * src[source[t]] + (1 - lam[t]) *
 *     src[source[partner[t]]], MixUp's four operations above.  16-byte accesses where per_item % 4 == 0 and all four pointers are 16-byte
 *     aligned, 4-byte ones otherwise.  n * per_item < 2^31; the caller keeps 0 <= source < N and 0 <= partner < n. */
#define DHZ_GATHER_MIX_TABLE_WORDS 3
int dhz_gather_mix_pair(const float* gt, const float* hazy, const int64_t* table, float* out_gt, float* out_hazy, int n,
                        int64_t per_item, int mix, void* stream);

/* K6  shift mask builder: mask[nW,64,64] in {0,-100}  (M1:803-836), Hres x Wres map, win 8. */
int dhz_shift_mask(float* mask, int Hres, int Wres, int shift, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K1  LayerNorm + cyclic shift + window partition.  Replaces norm1 M1:839, roll M1:846,
 *     window_partition M1:550-574.   x: [B, Hres*Wres, C] -> xw: [B*nW, 64, C].
 *     stats: [B*Hres*Wres, 2] (mean, rstd) saved for backward.  eps = 1e-5.  C % 4 == 0, C <= 1024.
 *     partition == 0: plain LayerNorm, tokens stay in place (norm2, M1:873).
 */
int dhz_ln_partition_fwd(const float* x, const float* gamma, const float* beta, float* xw,
                         float* stats, int B, int Hres, int Wres, int C, int shift, int partition,
                         void* stream);
/* dxw: [B*nW,64,C] -> dx: [B,HW,C] = LN-backward(dxw) (+ dres when dres != NULL: the gradient that reaches x
 * through the residual shortcut, M1:872 - dx may alias dres);  dgamma,dbeta [C] are ACCUMULATED (caller zeroes). */
int dhz_ln_partition_bwd(const float* dxw, const float* x, const float* gamma, const float* stats,
                         const float* dres, float* dx, float* dgamma, float* dbeta, int B, int Hres,
                         int Wres, int C, int shift, int partition, void* stream);

/* K4 (tail)  window reverse + un-shift + residual with per-sample DropPath scale.
 *     Replaces window_reverse M1:577-601, roll M1:866, shortcut + drop_path(x) M1:872.
 *     out[b,p,:] = shortcut[b,p,:] + scale[b] * yw[window-position(b,p),:]   (scale == NULL -> 1).
 *     partition == 0: yw is already in token order (the LeFF residual x + drop_path(mlp(..)), M1:873).
 */
int dhz_reverse_residual_fwd(const float* yw, const float* shortcut, const float* scale, float* out,
                             int B, int Hres, int Wres, int C, int shift, int partition, void* stream);
/* dyw[window-position] = scale[b] * dout[b,p,:]  (the shortcut gradient is dout itself). */
int dhz_reverse_residual_bwd(const float* dout, const float* scale, float* dyw, int B, int Hres,
                             int Wres, int C, int shift, int partition, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Windows of win x win tokens, win = 4 or 8 (`_w` entries).  The block clamps its window to the map (M1:764-766): four down-samplings
 *     of a 64 x 64 patch leave a 4 x 4 map whose block runs ONE 4 x 4 window without shift; `--win_size 4` (options.py) runs 4 x 4
 *     windows at every level.  A 4 x 4 window has N = 16 tokens, u = n_top(16) = 15 sampled keys per query and 15 selected queries
 *     (ATT:310-315).  Every entry below is the entry of the same name without `_w` plus `win`; win = 8 RUNS that entry (same kernel,
 *     same bits), win = 4 the 16-token kernels (csrc/ps_attn16.hip: one wave per window-head), any other win returns DHZ_EINVAL - and so
 *     do a head_dim outside {16, 32, 64}, a map that is no multiple of win and a shift outside [0, win).
 *
 * K3  dhz_ps_attn_fwd_w / _bwd_w replace ProbAttention.forward ATT:287-342 and its autograd for N = win^2: q, k, v [B_, N, H, d] with
 *     token stride ld, idx [N, u] uint8, bias [H, N, N] or NULL, mask [nW, N, N] or NULL (window id b mod nW), out stride ldo, rank
 *     [B_, H, N] uint8 (0 .. u-1 by descending sparsity measure, 255 = not selected; at N = 16 exactly one query per window-head).
 *     dtype = DHZ_F32 / DHZ_BF16 storage.  Backward: dq (zero rows for unselected queries), dk, dv with every element written;
 *     dbias_part [dhz_ps_attn_bwd_parts_w(B_, H, d, win), N, N] written, not accumulated, row p belongs to head p % H (NULL iff
 *     bias == NULL).  The 16-token kernels use no float atomics: deterministic in every mode.
 * K3-dense  dhz_dense_attn_fwd_w / _bwd_w replace WindowAttention.forward M0:428-492 and its autograd; dbias_part has
 *     dhz_ps_attn_bwd_parts_w(B_, H, d, win) rows at win = 4 and dhz_ps_attn_bwd_parts(B_, H) rows at win = 8. */
#define DHZ_NTOK16 16 /* tokens per 4x4 window */
#define DHZ_NTOP16 15 /* u = 5*ceil(ln 16) */
int dhz_ps_attn_fwd_w(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias, const float* mask,
                      void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d, int win, int dtype, void* stream);
int dhz_ps_attn_bwd_parts_w(int B_, int H, int d, int win);
int dhz_ps_attn_bwd_w(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask, const uint8_t* rank,
                      const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg, float* dbias_part, int B_, int H, int nW, int d,
                      int win, int dtype, void* stream);
/* K3 with padding words (see dhz_ps_attn_fwd_dt_pad, which win = 8 runs): pad[B_] uint64, 4 x 4 windows use the low 16 bits. */
int dhz_ps_attn_fwd_w_pad(const void* q, const void* k, const void* v, int ld, const uint8_t* idx, const float* bias, const float* mask,
                          const uint64_t* pad, void* out, int ldo, uint8_t* rank, int B_, int H, int nW, int d, int win, int dtype,
                          void* stream);
int dhz_ps_attn_bwd_w_pad(const void* q, const void* k, const void* v, int ld, const float* bias, const float* mask, const uint64_t* pad,
                          const uint8_t* rank, const void* dout, int ldo, void* dq, void* dk, void* dv, int ldg, float* dbias_part, int B_,
                          int H, int nW, int d, int win, int dtype, void* stream);
/* The padding words of one block resolution: replaces
 *          m = F.interpolate(mask, (H, W)); am = window_partition(m.permute(0, 2, 3, 1), win).view(-1, win win)    (M1:791-793)
 *     and keeps of it what the attention reads: bits[b] bit i = (am[b, i] != 0), b over B (H / win) (W / win) windows in window_partition's
 *     order (no cyclic shift, as the reference).  mask [B, 1, Himg, Wimg] fp32; Himg % H == 0 and Wimg % W == 0 (nearest resampling then
 *     reads mask[y Himg / H, x Wimg / W] exactly), anything else returns DHZ_EINVAL; win = 4 or 8. */
int dhz_pad_window_bits(const float* mask, uint64_t* bits, int B, int Himg, int Wimg, int H, int W, int win, void* stream);
int dhz_dense_attn_fwd_w(const float* q, const float* k, const float* v, int ld, const float* bias, const float* mask, float* out,
                         int ldo, int B_, int H, int nW, int d, float scale, int win, void* stream);
int dhz_dense_attn_bwd_w(const float* q, const float* k, const float* v, int ld, const float* bias, const float* mask, const float* dout,
                         int ldo, float* dq, float* dk, float* dv, int ldg, float* dbias_part, int B_, int H, int nW, int d, float scale,
                         int win, void* stream);
/* K1 / K4 (tail) for win x win windows: LayerNorm + roll + window_partition M1:839-852, 550-574 and window_reverse + roll + residual
 *     M1:577-601, 866, 872 (arguments of the `_dt` entries plus win; xw / yw / dyw rows in the order [B * nW, win^2, C]). */
int dhz_ln_partition_fwd_w(const void* x, const float* gamma, const float* beta, void* xw, float* stats, int B, int Hres, int Wres, int C,
                           int shift, int partition, int win, int dtype, void* stream);
int dhz_ln_partition_bwd_w(const void* dxw, const void* x, const float* gamma, const float* stats, const void* dres, void* dx,
                           float* dgamma, float* dbeta, int B, int Hres, int Wres, int C, int shift, int partition, int win, int dtype,
                           void* stream);
int dhz_reverse_residual_fwd_w(const void* yw, const void* shortcut, const float* scale, void* out, int B, int Hres, int Wres, int C,
                               int shift, int partition, int win, int dtype, void* stream);
int dhz_reverse_residual_bwd_w(const void* dout, const float* scale, void* dyw, int B, int Hres, int Wres, int C, int shift, int partition,
                               int win, int dtype, void* stream);
/* K6  shift mask builder M1:803-836 for win x win windows: mask [nW, win^2, win^2] in {0, -100}; 0 < shift < win, maps larger than win. */
int dhz_shift_mask_w(float* mask, int Hres, int Wres, int shift, int win, void* stream);
/* K7  relative-position bias M1:408-410 for win x win windows: table [(2 win - 1)^2, H] -> bias [H, win^2, win^2], and the table gradient
 *     from the partial tiles of the backward kernels (dtable [(2 win - 1)^2, H], overwritten when accumulate == 0).  At win = 4 the
 *     gradient is a fixed-order sum without atomics. */
int dhz_bias_gather_w(const float* table, float* bias, int H, int win, void* stream);
int dhz_bias_table_grad_w(const float* dbias_part, int parts, float* dtable, int H, int accumulate, int win, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K5 (middle)  LeFF depthwise stage in token (NHWC) layout.  Replaces the NHWC<->NCHW rearranges,
 *     the GELU after linear1, the depthwise 3x3 conv and its GELU  (M1:488,514-520).
 *     u: [B, Hres*Wres, Ch] = linear1 output BEFORE GELU.  w: [Ch,1,3,3] (PyTorch layout), b: [Ch].
 *     z = gelu(dwconv3x3(gelu(u)) + b).   When t != NULL the kernel also stores t = gelu'(pre-activation),
 *     the only thing the backward needs from the second GELU (same bytes as saving the pre-activation,
 *     one exponential fewer per element in the backward).  GELU is the exact-erf form evaluated with the
 *     Abramowitz-Stegun 7.1.26 rational approximation of erf (|error| <= 1.5e-7, i.e. fp32 rounding level).
 */
int dhz_leff_dwconv_fwd(const float* u, const float* w, const float* b, float* t, float* z, int B,
                        int Hres, int Wres, int Ch, void* stream);
/* du (overwritten); dw [Ch*9], db [Ch] ACCUMULATED (caller zeroes). */
int dhz_leff_dwconv_bwd(const float* dz, const float* u, const float* t, const float* w, float* du,
                        float* dw, float* db, int B, int Hres, int Wres, int Ch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K10  Charbonnier loss on clamp(x,0,1)  (TR:230 + losses.py:48-52).
 *      loss_sum (1 float, ACCUMULATED; caller zeroes) = sum sqrt((clamp(x)-y)^2 + eps^2).
 *      The mean is loss_sum / n.  Backward: dx = gscale * d/sqrt(d^2+eps^2) inside (0,1), 0 outside
 *      (clamp has zero gradient outside [0,1]; boundary convention of torch.clamp: pass-through at
 *      exactly 0 or 1).  `clampd` (optional, may be NULL) receives clamp(x,0,1).
 *      clamp01 == 0: plain CharbonnierLoss.forward(x, y) without the clamp.
 */
int dhz_charbonnier_fwd(const float* x, const float* y, float* clampd, float* loss_sum, int64_t n,
                        float eps, int clamp01, void* stream);
/* gclamp (optional): gradient arriving at clamp(x,0,1) from other consumers (the contrastive loss);
 * dx = inside(x) * (gscale[0]*inv_n * d/sqrt(d^2+eps^2) + gclamp). */
int dhz_charbonnier_bwd(const float* x, const float* y, const float* gscale, const float* gclamp,
                        float* dx, int64_t n, float eps, float inv_n, int clamp01, void* stream);

/* K12  AdamW step over one flat fp32 buffer (torch.optim.AdamW semantics, TR:90-92):
 *      p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;
 *      p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).   `step` is t (>= 1).
 *      grad_scale multiplies g first (1/world_size after a sum all-reduce). */
int dhz_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float wd, int step, float grad_scale, void* stream);
/*      the same, also writing the updated parameters as bf16 to p16[n] (may be NULL): the weight copy the bf16 GEMMs of BASELINE
 *      config 4 read, produced in the optimizer's own pass instead of a separate cast of the whole buffer */
int dhz_adamw_step_shadow(float* p, const float* g, float* m, float* v, void* p16, int64_t n, float lr, float beta1,
                          float beta2, float eps, float wd, int step, float grad_scale, void* stream);

/* C1   The gradient exchange of the data-parallel path (one process per GPU, batch-axis sharding): thin wrappers over RCCL for a
 *      host that binds only this library - replaces nn.DataParallel's gradient reduction (My_train.py:97).  RCCL is resolved at
 *      run time (dlopen; a copy the process already holds, e.g. PyTorch's, is shared), so single-GPU users never load it.
 *      dhz_comm_unique_id : rank 0 fills id128 (128 bytes) and hands it to the other ranks out of band (a file, MPI, a socket)
 *      dhz_comm_init      : every rank, after hipSetDevice(its GPU); *comm receives the communicator
 *      dhz_comm_allreduce_sum_f32 : in-place SUM all-reduce of buf[n] (a bucket of the flat gradient), enqueued on `stream`; the
 *                           1/world factor belongs to dhz_adamw_step's grad_scale
 *      dhz_comm_destroy   : releases the communicator.
 *      The Python host of this repository reaches the same RCCL through torch.distributed("nccl") (dehaze_hip/train.py::GradReducer). */
int dhz_comm_unique_id(void* id128);
int dhz_comm_init(void** comm, int rank, int nranks, const void* id128);
int dhz_comm_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int dhz_comm_destroy(void* comm);

/* K13  FFA-Net's own layers (FFA = FFA_model/models/FFA.py) in the channel-blocked layout of K11, fp32, C = 64 (csrc/ffa_attn.hip):
 *      channel attention CALayer (FFA:24-38: aten::mean -> 1x1 convolution -> relu_ -> 1x1 convolution -> sigmoid -> mul), pixel attention
 *      PALayer (FFA:9-21: 1x1 convolution 64 -> 8 -> relu_ -> 1x1 convolution 8 -> 1 -> sigmoid -> mul) and the `res += x` of a Block
 *      (FFA:54-56) with G = 1 map; the fusion head (FFA:105-108: aten::cat of the three group outputs -> mean -> the gate MLP -> three
 *      slices, three mul, two add -> PALayer) with G = 3 maps m0, m1, m2 (m1, m2 are ignored for G = 1; no concatenated tensor exists).
 *      Maps are [B][8][H][W][8]; H and W multiples of 16 (any H, W: the `_any` entries below); 16-byte aligned pointers.
 *        mean[b][g 64 + c] = (1 / HW) sum_p m_g[b][c][p]
 *        hid = relu(Wa mean + ba)     Wa [hc][64 G], hc = 8 (G = 1, FFA:29) or 4 (G = 3, FFA:86)
 *        ca  = sigmoid(Wb hid + bb)   Wb [64 G][hc]
 *        t[b][c][p] = sum_g ca[b][g 64 + c] m_g[b][c][p]
 *        h[b][i][p] = relu(sum_c Wp1[i][c] t[b][c][p] + bp1[i]), i < 8  (FFA:13);   pg[b][p] = sigmoid(sum_i wp2[i] h[b][i][p] + bp2)  (FFA:15)
 *        out = t pg (+ res when res != NULL)
 *      dhz_ffa_ca_fwd: mean [B][64 G], hid [B][hc], ca [B][64 G] are all written (the backward reads them).  Pooling in chunks of 1024
 *        pixels, one partial vector per (image, group, chunk) in ws, summed per image in ascending chunk order.
 *      dhz_ffa_gate_pa_fwd: t, h, pg and out in one pass; writes out only.
 *      Backward of both (autograd of the sequences above), given dout, in three entries:
 *        dhz_ffa_gate_pa_bwd_a recomputes t, h, pg from m_g and ca, writes dt (one map)
 *              dpg = sum_c dout t;  dz = dpg pg (1 - pg);  dh_i = dz wp2[i] [h_i > 0];  dt_c = dout_c pg + sum_i Wp1[i][c] dh_i
 *          and, per workgroup of 128 pixels, the partial sums of dca[b][g 64 + c] = sum_p dt_c m_g, dWp1[i][c] = sum dh_i t_c,
 *          dbp1[i] = sum dh_i, dwp2[i] = sum dz h_i, dbp2 = sum dz to ws.
 *        dhz_ffa_ca_bwd sums those partials in fixed order (16 consecutive workgroups, then the groups of 16, then the images, each
 *          ascending) and runs the gate MLP backwards: dzb = dca ca (1 - ca); dWb = sum_b dzb (x) hid; dbb = sum_b dzb;
 *          dhid = (Wb^T dzb) [hid > 0]; dWa = sum_b dhid (x) mean; dba = sum_b dhid; dmean [B][64 G] = Wa^T dhid.  ws must be the
 *          workspace dhz_ffa_gate_pa_bwd_a has just filled for the same B, H, W, G.  It leaves the level-1 sums behind the partials, at
 *          float offset B chunks (64 G + 532), chunks = H W / 128, as [B][ceil(chunks / 16)][64 G + 532]: the first 64 G floats of an
 *          image's segments add up to dca[b] (tests read it there).
 *        dhz_ffa_gate_pa_bwd_b writes dm_g = ca[b][g 64 + c] dt + dmean[b][g 64 + c] / HW for each g (dm1, dm2 ignored for G = 1).
 *          The gradient of res is dout itself.
 *      All parameter gradients (dWa, dba, dWb, dbb, dWp1, dbp1, dwp2, dbp2) are WRITTEN, not accumulated, as dhz_conv3x3_wgrad does.
 *      No atomics; the cut of every reduction depends on the shapes alone: the same bits from run to run, under any
 *      dhz_set_reserved_cus, with the deterministic mode on or off.
 *      ws: dhz_ffa_workspace_bytes(B, H, W, G) bytes (one size for the three entries that take it; a function of the shapes alone; 0
 *      for an unsupported shape), 16-byte aligned.  With dhz_set_deterministic on, the mode's workspace (dhz_set_det_workspace) is used
 *      instead and ws may be NULL; dhz_ffa_ca_bwd must then follow its dhz_ffa_gate_pa_bwd_a with no other accumulating entry between.
 *      Anything else - a null pointer, B < 1, H or W no multiple of 16, G outside {1, 3}, a missing or too small workspace, a pointer
 *      that is not 16-byte aligned - is DHZ_EINVAL before any launch. */
size_t dhz_ffa_workspace_bytes(int B, int H, int W, int G);
int dhz_ffa_ca_fwd(const float* m0, const float* m1, const float* m2, const float* Wa, const float* ba, const float* Wb, const float* bb,
                   float* mean, float* hid, float* ca, float* ws, size_t ws_bytes, int B, int H, int W, int G, void* stream);
int dhz_ffa_gate_pa_fwd(const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1, const float* bp1,
                        const float* wp2, const float* bp2, const float* res, float* out, int B, int H, int W, int G, void* stream);
int dhz_ffa_gate_pa_bwd_a(const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1, const float* bp1,
                          const float* wp2, const float* bp2, const float* dout, float* dt, float* ws, size_t ws_bytes, int B, int H, int W,
                          int G, void* stream);
int dhz_ffa_ca_bwd(float* ws, size_t ws_bytes, const float* Wa, const float* Wb, const float* mean, const float* hid, const float* ca,
                   float* dWa, float* dba, float* dWb, float* dbb, float* dmean, float* dWp1, float* dbp1, float* dwp2, float* dbp2, int B,
                   int H, int W, int G, void* stream);
int dhz_ffa_gate_pa_bwd_b(const float* dt, const float* ca, const float* dmean, float* dm0, float* dm1, float* dm2, int B, int H, int W,
                          int G, void* stream);
/*      The six entries on maps of ANY size (H, W >= 1; 64 H W < 2^31): FFA-Net on whole images, as FFA_model/test.py feeds it.  Formulas,
 *      tensors, G, alignment and workspace rules, error codes: those above.  The kernels index a flat pixel p < HW; what the ragged
 *      sizes change is the tails, each a function of the shapes alone:
 *        pooling       chunks of 1024 pixels; the last chunk holds HW - 1024 (chunks - 1) pixels, of any count
 *        gate forward  ceil(HW / 256) workgroups per image; threads whose pixel is >= HW do nothing
 *        backward a    chunks = ceil(HW / 128) workgroups per image; in a partly filled last one the pixels >= HW are neither loaded
 *                      nor stored and enter the slot's sums as zeros.  The workspace layout is the one above with this `chunks`: the
 *                      level-1 sums at float offset B chunks (64 G + 532), as [B][ceil(chunks / 16)][64 G + 532]
 *        backward b    one thread per float4 of dt, bounded by 16 B HW
 *      On a shape the entries above take (H, W multiples of 16) each `_any` entry issues the same launches and writes the same bits, and
 *      dhz_ffa_workspace_bytes_any equals dhz_ffa_workspace_bytes.  No atomics: the same bits from run to run, under any
 *      dhz_set_reserved_cus, with the deterministic mode on or off. */
size_t dhz_ffa_workspace_bytes_any(int B, int H, int W, int G);
int dhz_ffa_ca_fwd_any(const float* m0, const float* m1, const float* m2, const float* Wa, const float* ba, const float* Wb,
                       const float* bb, float* mean, float* hid, float* ca, float* ws, size_t ws_bytes, int B, int H, int W, int G,
                       void* stream);
int dhz_ffa_gate_pa_fwd_any(const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1, const float* bp1,
                            const float* wp2, const float* bp2, const float* res, float* out, int B, int H, int W, int G, void* stream);
int dhz_ffa_gate_pa_bwd_a_any(const float* m0, const float* m1, const float* m2, const float* ca, const float* Wp1, const float* bp1,
                              const float* wp2, const float* bp2, const float* dout, float* dt, float* ws, size_t ws_bytes, int B, int H,
                              int W, int G, void* stream);
int dhz_ffa_ca_bwd_any(float* ws, size_t ws_bytes, const float* Wa, const float* Wb, const float* mean, const float* hid, const float* ca,
                       float* dWa, float* dba, float* dWb, float* dbb, float* dmean, float* dWp1, float* dbp1, float* dwp2, float* dbp2,
                       int B, int H, int W, int G, void* stream);
int dhz_ffa_gate_pa_bwd_b_any(const float* dt, const float* ca, const float* dmean, float* dm0, float* dm1, float* dm2, int B, int H,
                              int W, int G, void* stream);
/*      The two elementwise passes of a Block (FFA:51-56) over n floats (n % 4 == 0, any common element order):
 *      dhz_ffa_add: y = a + x  (`res = res + x`, FFA:52: aten::add; also the group residual FFA:69 and the `+ x1` of FFA:110).
 *      dhz_ffa_relu_bwd_add: dpre1 = a1 > 0 ? dr : 0 (aten::threshold_backward of act1 by the sign of the saved activation a1) and
 *        s = dout + dr (the two gradients that reach the block input besides conv1's) in one pass. */
int dhz_ffa_add(const float* a, const float* x, float* y, int64_t n, void* stream);
/*      dhz_ffa_add_any: dhz_ffa_add for any n > 0 (the last n % 4 floats are added one by one; where n % 4 == 0, the same bits): the `+ x1` of
 *        FFA:110 on an image whose 3 B H W is no multiple of 4. */
int dhz_ffa_add_any(const float* a, const float* x, float* y, int64_t n, void* stream);
int dhz_ffa_relu_bwd_add(const float* a1, const float* dr, const float* dout, float* dpre1, float* s, int64_t n, void* stream);

/* K14  SSIM and squared error of image pairs, scored in float64 (csrc/metrics.hip): the validation metrics of FFA-Net's recipe
 *      (M = FFA_model/metrics.py; FFA_model/main.py:151-173 scores every validation image with them) and of utils/metrics.py (U, the
 *      scikit-image form test_long_GPU.py:94-98 uses), from one kernel.  a, b: fp32 planes, plane (i, c) of `a` starts at
 *      a + i a_img_stride + c a_ch_stride (elements, >= 0), its rows are W floats apart; only 4-byte alignment is assumed (image 1 of a
 *      stacked batch may start anywhere).  With clamp01 != 0 both inputs are clamped to [0, 1] on load (M:51-52, M:62-63).  Per plane, with
 *      x, y the (clamped) inputs as doubles and w = `window` (K x K fp32 weights, row-major, on the device), all arithmetic in double:
 *        mx = wscale sum w x,  my = wscale sum w y,  mxx = wscale sum w x x,  myy = wscale sum w y y,  mxy = wscale sum w x y      (M:32-39, U:38-41)
 *        vx = cov_norm (mxx - mx mx),  vy = cov_norm (myy - my my),  vxy = cov_norm (mxy - mx my)                                    (M:37-39, U:42)
 *        S  = ((2 mx my + C1)(2 vxy + C2)) / ((mx mx + my my + C1)(vx + vy + C2))                                                    (M:42,    U:44)
 *      valid == 0, the zero-padded rule: S on all H x W pixels, window centred, taps outside the plane contribute 0 (M:32: padding =
 *        window_size // 2); any H, W >= 1, planes smaller than the window included.
 *      valid == 1: S on the (H - K + 1) x (W - K + 1) pixels whose window lies inside the plane (U:45-46: what is left after the border
 *        crop, which uniform_filter's reflection never reaches); needs H, W >= K.
 *      ssim_sum[i C + c] = sum of S over that extent (the caller divides by its pixel count: M:45, M:47, U:46);
 *      sqerr_sum[i C + c] = sum over all H x W pixels of (x - y)^2, the subtraction and the square in fp32 as both host routes form them
 *        (M:64-65, U:30), added in double.  Both are WRITTEN.
 *      M is K = 11, window = create_window's fp32 outer product (M:25-26: not separable to the last bit, hence a table), wscale = 1,
 *        valid = 0, C1 = 0.01^2, C2 = 0.03^2 (M:40-41), cov_norm = 1, clamp01 = 1.
 *      U is K = 7, window = 49 ones, wscale = 1 / 49 (a double: the fp32 value of 1 / 49 is 4.6e-8 off, which 1 / C2 would amplify),
 *        valid = 1, C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = data_range (U:43), cov_norm = 49 / 48 (U:36-37), clamp01 = 0.
 *      Cuts: bands of 32 columns x 64 rows, one workgroup and one pair of double partial sums in ws each; a second launch adds a plane's
 *      pairs in ascending band order, one owner thread per result.  No atomics; every cut is a function of the shapes: the same bits from
 *      run to run, under any dhz_set_reserved_cus, with the deterministic mode on or off (the mode's workspace is not used).
 *      ws: dhz_ssim_pair_workspace_bytes(B, C, H, W) bytes (0 for an unsupported shape), 8-byte aligned like ssim_sum and sqerr_sum.
 *      Anything else - a null pointer, K outside {7, 11}, B, C, H or W < 1 (or B C > 65535, H > 4194240, H W >= 2^31), H or W < K under the
 *      valid rule, a border rule outside {0, 1}, a negative stride, a missing, too small or misaligned workspace - is DHZ_EINVAL before
 *      any launch. */
size_t dhz_ssim_pair_workspace_bytes(int B, int C, int H, int W);
int dhz_ssim_pair(double* ssim_sum, double* sqerr_sum, const float* a, int64_t a_img_stride, int64_t a_ch_stride, const float* b,
                  int64_t b_img_stride, int64_t b_ch_stride, int B, int C, int H, int W, int K, const float* window, double wscale,
                  int valid, double C1, double C2, double cov_norm, int clamp01, void* ws, size_t ws_bytes, void* stream);

/* K15  SSIM as a training loss (csrc/ssim_loss.hip): loss = 1 - mean(S) of the Gaussian-window SSIM map and its gradient with respect to the
 *      prediction, for both forms the reference has: M = FFA_model/metrics.py (`ssim`, M:31-58: zero padding of 5, inputs clamped) and
 *      A = Uformer_ProbSparse/aaa.py (`ssim`, A:26-75: no padding, A:42-57, no clamp).  x (prediction), y (target): contiguous fp32
 *      [B, C, H, W]; window: the K x K = 11 x 11 fp32 table of create_window (M:24-28, A:15-19), row-major, on the device, under BOTH border
 *      rules; valid, C1, C2, clamp01 as in K14 (wscale = cov_norm = 1).  With mux, muy, Exx, Eyy, Exy the five local moments (correlation
 *      with the window, M:32-39 / A:48-57) of the (clamped) inputs as doubles, all arithmetic in double:
 *        A1 = 2 mux muy + C1,  A2 = 2 (Exy - mux muy) + C2,  B1 = mux^2 + muy^2 + C1,  B2 = (Exx - mux^2) + (Eyy - muy^2) + C2
 *        S  = A1 A2 / (B1 B2)                                                                                      (M:42, A:62-66)
 *      valid == 0: S on all H x W pixels over zero padding (M:32), any H, W >= 1; valid == 1: S on the (H - 10) x (W - 10) pixels whose
 *        window lies inside the plane (A:42, padd = 0), H, W >= 11.  N = the number of map pixels, B C H' W'.
 *      dhz_ssim_loss_fwd: loss[0] = (float)(1 - sum S / N) (M:45, A:69), WRITTEN.  With need_grad != 0 it also keeps, per map pixel, in ws
 *        a = -S / B2,  b = 2 A1 / (B1 B2),  m = 2 muy A2 / (B1 B2) - 2 mux S / B1 - 2 mux a - muy b      (dS/dExx, dS/dExy, dS/dmux)
 *      dhz_ssim_loss_bwd (after a forward with need_grad on the same ws, same arguments):
 *        dx(q) = -gloss[0] / N [ (w^T * m)(q) + 2 x(q) (w^T * a)(q) + y(q) (w^T * b)(q) ],  WRITTEN, not accumulated; gloss is a device
 *        scalar (no host sync); w^T * is the transposed correlation (the same window over zero padding when valid == 0, the full
 *        correlation of the smaller map when valid == 1).  With clamp01, x and y above are the clamped values and dx is 0 where the raw x
 *        lies outside [0, 1]; the bounds themselves pass the gradient, as torch.clamp does.  There is no gradient for y.
 *      Cuts: bands of 32 columns x 64 rows, one workgroup and one double partial sum each; a one-workgroup launch adds them in a fixed
 *      order.  No atomics; every cut is a function of the shapes: the same bits from run to run, under any dhz_set_reserved_cus, with the
 *      deterministic mode on or off (the mode's workspace is not used).
 *      ws: dhz_ssim_loss_workspace_bytes(B, C, H, W, valid) bytes - the partial sums and the three maps as doubles; 0 for an unsupported
 *      shape - 8-byte aligned.  A null pointer, K != 11, B, C, H or W < 1 (or B C > 65535, H > 4194240, B C H W >= 2^31), H or W < 11
 *      under the valid rule, a border rule outside {0, 1}, a missing, too small or misaligned workspace: DHZ_EINVAL before any launch. */
size_t dhz_ssim_loss_workspace_bytes(int B, int C, int H, int W, int valid);
int dhz_ssim_loss_fwd(float* loss, const float* x, const float* y, int B, int C, int H, int W, int K, const float* window, int valid,
                      double C1, double C2, int clamp01, int need_grad, void* ws, size_t ws_bytes, void* stream);
int dhz_ssim_loss_bwd(float* dx, const float* gloss, const float* x, const float* y, int B, int C, int H, int W, int K, const float* window,
                      int valid, double C1, double C2, int clamp01, void* ws, size_t ws_bytes, void* stream);

/* K16  Total-variation losses (csrc/tv_loss.hip): the two smoothness terms of Uformer_ProbSparse/losses.py (L) and their gradients.
 *      x: contiguous fp32 [B, C, H, W]; all arithmetic in double (a difference of two fp32 values is exact there); sums are per plane.
 *      form == 0, "beta" (`tv_loss`, L:8-18): on the (H - 1) x (W - 1) sites i < H - 1, j < W - 1 of a plane
 *        s = (x[i,j+1] - x[i,j])^2 + (x[i+1,j] - x[i,j])^2,   loss = coeff sum s^beta / (B C H W)          (coeff = reg_coeff, L:18)
 *        the last row and column hold no site; the divisor is the full element count, as in L.
 *      form == 1, "sq" (`TVLoss.forward`, L:25-33): with sum_v, sum_h the sums of the squared vertical / horizontal first differences
 *        loss = coeff 2 (sum_v / (C (H - 1) W) + sum_h / (C H (W - 1))) / B                                (coeff = tv_loss_weight, L:33)
 *        beta is checked and otherwise unused.
 *      Zero-site rule (the one deviation from autograd of L): a site with s == 0 - both differences exactly zero, a function of the input
 *        bits - contributes 0 to the gradient; the value is unaffected (0^beta = 0).  Autograd of L gives inf * 0 = NaN there for beta < 1,
 *        on every pixel of such a site, and a prediction clamped to [0, 1] always has such sites.  The other sites a pixel belongs to
 *        contribute as ever.
 *      dhz_tv_loss_fwd: loss[0] = (float) of the above, WRITTEN.
 *      dhz_tv_loss_bwd: dx = gloss[0] * d loss / d x, WRITTEN, not accumulated, recomputed from x alone in gather form (pixel (i, j) reads
 *        the sites (i, j), (i, j - 1), (i - 1, j) under beta, its four neighbours under sq): no saved maps, no workspace, no atomics.
 *        gloss is a device scalar (no host sync).
 *      Cuts: bands of 64 columns x 64 rows, one workgroup and one double partial sum each; a one-workgroup launch adds them in a fixed
 *      order.  Every cut is a function of the shapes: the same bits from run to run, under any dhz_set_reserved_cus, with the
 *      deterministic mode on or off (the mode's workspace is not used).
 *      ws: dhz_tv_loss_workspace_bytes(B, C, H, W) bytes - one double per band; 0 for an unsupported shape - 8-byte aligned.  A null
 *      pointer, a form outside {0, 1}, beta <= 0 or not finite, B or C < 1, H or W < 2 (no site; the Python module routes such planes to
 *      the ATen formula), B C > 65535, H > 4194240, B C H W >= 2^31, a missing, too small or misaligned workspace: DHZ_EINVAL before any
 *      launch. */
size_t dhz_tv_loss_workspace_bytes(int B, int C, int H, int W);
int dhz_tv_loss_fwd(float* loss, const float* x, int B, int C, int H, int W, int form, double beta, double coeff, void* ws, size_t ws_bytes,
                    void* stream);
int dhz_tv_loss_bwd(float* dx, const float* gloss, const float* x, int B, int C, int H, int W, int form, double beta, double coeff,
                    void* stream);

/* K17  Fourier and variance analysis of feature maps (csrc/fourier.hip): what the reference's fourier_analysis.ipynb and
 *      featuremap_variance.ipynb compute from a latent, in one read of it and without a 2-D transform.  Per n x n map f = (b, c) of x:
 *        A[b, c, k] = log(|F[k][k]| + 1e-6), k = 0 .. n/2 - 1, F = the 2-D DFT of f: the notebook's fft2 -> log(abs + 1e-6) -> shift ->
 *                     .diag()[n/2:], before its mean over batch and channels;
 *        V[b, c]    = the unbiased variance of f over its n^2 positions (latent.var(dim=[-1, -2]));
 *        sumA[k], sumV[0] = the sums of A[., ., k] and of V over the M = B C maps m = b C + c, in a fixed order: partial j = the maps
 *                     j, j + 16, j + 32, ... added in ascending order, j = 0 .. 15, then the partials added in ascending j.
 *      The diagonal comes from g[s] = sum of f[y][x] over (y + x) mod n = s:  F[k][k] = sum_s g[s] exp(-2 pi i k s / n), summed over
 *      s = 0 .. n - 1 in that order with the twiddle index (k s) mod n reduced in integers.  V is accumulated around the map's first
 *      element: V = (sum d^2 - (sum d)^2 / n^2) / (n^2 - 1), d = f - f[0][0].  All arithmetic is double, no atomics, every cut (rows per
 *      workgroup, channel tiles) a function of the shapes: the same bits from run to run, under any dhz_set_reserved_cus, with the
 *      deterministic mode on or off (the mode's workspace is not used).
 *      x: layout 0 = tokens [B, n n, C] (what the Uformer blocks hold), layout 1 = NCHW [B, C, n, n]; contiguous; dtype DHZ_F32 or DHZ_BF16.
 *      A [B, C, n/2], V [B, C], sumA [n/2], sumV [1]: doubles, all WRITTEN.  n even, 2 <= n <= 2048; 1 <= B, C <= 65535.
 *      ws: dhz_fourier_diag_workspace_bytes(B, C, n, layout) bytes (the partial g vectors and variance sums of the row cuts; 0 for an
 *      unsupported shape), 8-byte aligned like the four outputs.  An odd n, n out of range, a layout or dtype code outside {0, 1}, B or C out
 *      of range, a null pointer, a missing, too small (the message names the bytes needed) or misaligned workspace: DHZ_EINVAL before any
 *      launch. */
size_t dhz_fourier_diag_workspace_bytes(int B, int C, int n, int layout);
int dhz_fourier_diag(double* A, double* V, double* sumA, double* sumV, const void* x, int B, int C, int n, int layout, int dtype, void* ws,
                     size_t ws_bytes, void* stream);

/* K18  Frequency-band noise (csrc/freq_noise.hip): the reference's FreqAttack._fourier_mask (ops/adversarial.py: fft2 -> shift -> mask ->
 *      unshift -> ifft2 -> real part) without a 2-D transform.  A width w (even, 0 <= w <= n) keeps the frequencies
 *      B(w) = {-w/2 .. w/2 - 1} on each axis; the band is B(w1) x B(w1) minus B(w2) x B(w2).  With
 *        c_w[t] = (1/n) sum_{k in B(w)} cos(2 pi k t / n),   s_w[t] = (1/n) sum_{k in B(w)} sin(2 pi k t / n),
 *      C_w[a][b] = c_w[(a - b) mod n] and S_w likewise, per n x n plane
 *        band(d)  = (C_w1 d C_w1^T - S_w1 d S_w1^T) - (C_w2 d C_w2^T - S_w2 d S_w2^T),
 *        d        = delta (take_sign 0) or sign(delta) with sign(+-0) = 0 (take_sign 1),
 *        noise    = scale * band(d)              doubles, WRITTEN where the pointer is non-null,
 *        out      = (float)((double)x + noise)   one rounding.
 *      x, delta, out: [M, n, n] fp32, contiguous, M planes (B C; any channel count).  out must not overlap x or delta.  n even,
 *      2 <= n <= 512; 1 <= M <= 65535; M n n < 2^31.  w1 = w2 (0, 0 included): out = x bit for bit, noise = +0.0, no band work.
 *      All arithmetic is double; the twiddles come from the index (k t) mod n reduced in integers (csrc/twiddle.h); sums run over k, then b,
 *      then (vector, a) in ascending order; no atomics; every cut (64 x 64 tiles, runs of 32) is a function of the shapes: the same bits
 *      from run to run, under any dhz_set_reserved_cus, with the deterministic mode on or off (the mode's workspace is not used).
 *      ws: dhz_band_noise_workspace_bytes(M, n) bytes (the four vectors and the four row products d C^T, d S^T per width; 0 for an
 *      unsupported shape), 8-byte aligned like noise.  An odd n, n, M or M n n out of range, an odd width or one outside [0, n], w2 > w1,
 *      a take_sign outside {0, 1}, a null out, x or delta, an out that overlaps x or delta, a missing, too small (the message names the
 *      bytes needed) or misaligned workspace: DHZ_EINVAL before any launch. */
size_t dhz_band_noise_workspace_bytes(int M, int n);
int dhz_band_noise(float* out, double* noise, const float* x, const float* delta, int M, int n, int w1, int w2, double scale, int take_sign,
                   void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEHAZE_HIP_H */
