"""torch.autograd.Function wrappers over the C-ABI (include/dehaze_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator), the current HIP stream and the
autograd tape; the ops below run hand-written gfx950 kernels through ctypes (the token-Linear GEMMs included:
dhz_linear_fwd / dhz_linear_dgrad / dhz_linear_wgrad).  No vendor compute kernel is left in the fp32 or the bf16 training
step; the library is reached only for shapes the kernels do not tile (e.g. the VGG19 stack of the contrastive loss on images
smaller than 64 pixels or with sides that are no multiples of 16 - every larger such patch, 64 / 192 / 240 / 384 pixels
included, runs the Winograd kernels on maps of any size -, Downsample / projections of unusual channel counts - DESIGN.md
section 2).  CPU tensors are rejected - there is no fallback path.
"""
import collections
import ctypes

import os

import torch
from torch.autograd import Function

from . import _lib

NTOK, NTOP = 64, 25            # 8 x 8 windows
NTOK16, NTOP16 = 16, 15        # 4 x 4 windows: u = n_top(16) = 15
WINDOWS = {NTOK: 8, NTOK16: 4}  # tokens per window -> window side of the kernels that exist


def _win_of(N):
    """window side for N tokens per window; the kernels exist for 8 x 8 and 4 x 4 windows only"""
    try:
        return WINDOWS[int(N)]
    except KeyError:
        raise NotImplementedError(f"windows of {N} tokens: the HIP kernels exist for 4x4 and 8x8 windows (16 or 64 tokens) only") from None

# bench.py sets this to {"<entry point>": []} to collect (start_event, end_event, units) per launch of
# that kernel, recorded on the stream the kernel is launched on (torch's current stream).
KERNEL_TIMING = None


def _stream():
    if DETERMINISTIC and _DET_WS is None:
        _det_workspace()
    return torch.cuda.current_stream().cuda_stream


# Deterministic mode (include/dehaze_hip.h, dhz_set_deterministic): every accumulating kernel stores per-work-item partials in a
# workspace and a fixed-order reduction adds them to the target - no fp32 atomics, a cut into work items that depends on the shapes alone:
# the same step gives the same bits from run to run, under any CU reservation.  fp32 storage, one process; off by default.
# DHZ_DETERMINISTIC=1 in the environment turns it on at import; DHZ_DET_WORKSPACE_MB sizes the workspace (default 256: the largest need of
# the E = 32 model's step at 256 x 256 is 17 MB, of a UNet step at dim 32, 128 x 128, batch 32 19 MB; a call that needs more fails
# and names the bytes).
DETERMINISTIC = False
_DET_WS = None


def _det_workspace(nbytes=None):
    """allocate the workspace on the current device and hand it to the library (on the first launch after the switch: importing with
    DHZ_DETERMINISTIC=1 must not initialise the GPU)"""
    global _DET_WS
    if nbytes is None:
        nbytes = int(float(os.environ.get("DHZ_DET_WORKSPACE_MB", "256")) * (1 << 20))
    _DET_WS = torch.empty(max(nbytes // 4, 1), device="cuda", dtype=torch.float32)
    _lib.call("dhz_set_det_workspace", _DET_WS.data_ptr(), _DET_WS.numel() * 4)


def set_deterministic(on, workspace_bytes=None):
    """switch the deterministic mode of the library (process-global) and own its workspace.  workspace_bytes: a size other than
    DHZ_DET_WORKSPACE_MB's (allocated at once; needs the GPU).  A process that launches through the raw C-ABI only, before any ops.* call
    and before the GPU is initialised, hands a workspace over itself (dhz_set_det_workspace) or calls ops._stream() once."""
    global DETERMINISTIC, _DET_WS
    on = bool(on)
    if _DET_WS is not None:                              # give the old workspace back (stream order: its last reader is enqueued already)
        _lib.call("dhz_set_det_workspace", None, 0)
        _DET_WS = None
    _lib.call("dhz_set_deterministic", int(on))
    DETERMINISTIC = on
    # at once where the GPU is up already, so that raw C-ABI calls which never pass ops._stream() find it; else on the first launch
    if on and (workspace_bytes is not None or torch.cuda.is_initialized()):
        _det_workspace(None if workspace_bytes is None else int(workspace_bytes))


if os.environ.get("DHZ_DETERMINISTIC", "0") == "1":
    set_deterministic(True)


def _refuse_bf16_deterministic(what):
    if DETERMINISTIC:
        raise NotImplementedError(f"{what}: bf16 storage is outside the deterministic mode (DHZ_DETERMINISTIC / ops.set_deterministic): "
                                  "it covers fp32 storage only")


# The last tensors whose device pointers were handed to a launch: a pointer argument is often taken from a temporary
# (`_p(g.contiguous())`, `_p(w.to(dtype))`), which Python drops as soon as `_p` returns - before the launch is even enqueued.
# Stream order makes a later reuse of that block by the same stream harmless, but not a reuse from another stream (the
# reducer's, a loader's).  Keeping the most recent ones referenced closes the whole class; 64 covers the longest argument list.
_RECENT = collections.deque(maxlen=64)


def _p(t):
    if t is None:
        return None
    _RECENT.append(t)
    return t.data_ptr()


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dehaze_hip: this op runs only on a HIP device (got a CPU tensor); "
                               "there is deliberately no CPU/PyTorch fallback")
        if t is not None and t.dtype not in (torch.float32, torch.uint8, torch.bfloat16):
            raise RuntimeError(f"dehaze_hip: fp32 (or bf16 token tensors, BASELINE config 4) expected, got {t.dtype}")


BF16 = torch.bfloat16

_WARNED = set()


def warn_library_fallback(what, shape):
    """One warning per (layer kind, shape): a shape the hand-written kernels do not tile went to the library convolution."""
    key = (what, tuple(shape))
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(f"dehaze_hip: {what} with shape {tuple(shape)} is not tiled by the HIP kernels - running the library "
                      "convolution (MIOpen) for it", stacklevel=3)


def _dt(t):
    """dtype code of the dhz_*_dt entry points (include/dehaze_hip.h: DHZ_F32 = 0, DHZ_BF16 = 1)."""
    return 1 if t.dtype == BF16 else 0


# Derived copies of the flat fp32 parameter buffer that FlatAdamW keeps for the GEMMs:
#   BF16_SHADOW  = [flat f32, its bf16 copy]                      (config 4: the bf16 GEMMs' weight operand)
#   SPLIT_SHADOW = [flat f32, hi plane, mid plane, lo plane]      (the six-term split GEMMs' pre-split weight operand, bf16 each)
# A weight that is a view of the flat buffer gets the matching views - one launch per optimizer step for all parameters instead
# of one per Linear and pass.  The optimizer kernel keeps them current.  Writes that bypass it (a loaded checkpoint, a landscape
# probe, `with torch.no_grad(): p.add_(...)`) bump the autograd version counter of the PARAMETER (parameters are views with counters
# of their own: the flat buffer's counter does not see them).  Two guards, both through SHADOW_OWNER (a weak reference to the
# FlatAdamW that registered the copies - weak, so that dropping the optimizer frees its buffers and un-registers the copies):
#   * every lookup (split_planes, split_planes_t, bf16_copy, bf16_copy_t) validates itself: the counters of the parameters that
#     overlap the requested region are compared with the values recorded when the copies were derived (_shadow_fresh); on a
#     mismatch ALL copies are re-derived before the views are handed out.  So any entry that reaches a GEMM - a block, a layer, a
#     bare ops.* call - multiplies with current weights, not only train_step / Uformer.forward;
#   * sync_shadows() (train_step, Uformer.forward) checks all parameters at once.
# NOT seen by either: writes that bump no counter - `p.data.copy_(...)` / `p.data.add_(...)` (a fresh view with a fresh counter) and
# raw-pointer kernels.  After such a write call FlatAdamW.sync_shadows(force=True).
BF16_SHADOW = None
SPLIT_SHADOW = None
SHADOW_OWNER = None          # weakref.ref(FlatAdamW) or None


def _shadow_owner():
    global SHADOW_OWNER
    if SHADOW_OWNER is None:
        return None
    o = SHADOW_OWNER()
    if o is None:                # the optimizer is gone: its copies are meaningless
        SHADOW_OWNER = None
        set_bf16_shadow(None, None)
        set_split_shadow(None, None)
    return o


def sync_shadows(force=False):
    o = _shadow_owner()
    if o is not None:
        o.sync_shadows(force)


def _shadow_fresh(off, n):
    """called by the lookups with the flat-buffer region they are about to hand out views for"""
    o = _shadow_owner()
    if o is not None and not o.region_current(off, n):
        o.sync_shadows()

# Which matrix pipe takes the PRODUCTS of the fp32 path's GEMM-shaped kernels (storage, accumulation, bias / statistics stay fp32):
#   6 (default) - the bf16 pipe by operand splitting into three bf16 pieces (hi + mid + lo = all 24 mantissa bits, exactly) and the
#                 six products down to 2^-16 (hh, hm, mh, hl, lh, mm); what is dropped (ml, lm, ll) is <= 2^-24 relative - the size of
#                 ONE fp32 rounding, i.e. the error class of an fp32 FMA chain (csrc/linear_split.hip; every kernel-level fp32
#                 tolerance of tests/ holds under it).  6 / 16 of the fp32 pipe's matrix time.
#   0           - the fp32 matrix pipe itself (v_mfma_f32_16x16x4_f32, csrc/linear_gemm.hip / linear_wgrad.hip): bench.py times the
#                 same step on it as `fp32_pipe` beside the headline.
#   3           - EXPERIMENT, never a product setting: hi / lo pieces, three products (~16 mantissa bits per product).
# DHZ_SPLIT_BF16 in the environment overrides the default (1 means 3).
def _split_terms(v):
    try:
        return {0: 0, 1: 3, 3: 3, 6: 6}[int(v)]
    except (KeyError, ValueError):
        raise ValueError(f"DHZ_SPLIT_BF16={v!r}: expected 0 (fp32 matrix pipe), 6 (default: six-term bf16 split) or 3 (or 1; experiment)") from None


SPLIT_BF16 = _split_terms(os.environ.get("DHZ_SPLIT_BF16", "6"))
SPLIT_MIN_K = 128          # smallest contraction the three-term experiment splits in the forward / backward-data GEMMs


def set_bf16_shadow(f32, b16, b16t=None, desc=None, index=None, ntiles=0):
    """b16: bf16 mirror of the flat buffer; b16t (optional): the same with every registered matrix stored TRANSPOSED at its offset
    (desc / ntiles: the table of dhz_bf16_transpose_batched, index: {(offset, rows, cols)})."""
    global BF16_SHADOW
    BF16_SHADOW = None if f32 is None else [f32, b16, b16t, desc, index or set(), int(ntiles)]


def refresh_bf16_shadow_t():
    sh = BF16_SHADOW
    if sh is not None and sh[2] is not None:
        _lib.call("dhz_bf16_transpose_batched", sh[0].data_ptr(), sh[2].data_ptr(), sh[3].data_ptr(), sh[3].shape[0], sh[5], _stream())


def _t_offset(sh, t, index, W):
    """element offset of W in the flat buffer when the shadow `sh` keeps a TRANSPOSED copy of it (slot t; slot index: the registered
    matrices), else -1.  No side effect: the route function asks this, the lookups below validate and hand out the views."""
    if sh is None or sh[t] is None or not W.is_contiguous() or W.dim() != 2:
        return -1
    o = _view_of(sh[0], W)
    return o if o >= 0 and (o, W.shape[0], W.shape[1]) in sh[index] else -1


def bf16_copy_t(W):
    """bf16 copy of W^T ([K, N] row-major for W [N, K]) when FlatAdamW keeps one for this matrix, else None."""
    o = _t_offset(BF16_SHADOW, 2, 4, W)
    if o < 0:
        return None
    _shadow_fresh(o, W.numel())
    return BF16_SHADOW[2][o: o + W.numel()]


def refresh_bf16_shadow():
    sh = BF16_SHADOW
    if sh is not None:
        sh[1].copy_(sh[0])                   # one cast launch for all parameters
        refresh_bf16_shadow_t()


def _view_of(flat, W):
    """element offset of contiguous W inside the flat buffer, or -1"""
    off = W.data_ptr() - flat.data_ptr()
    if 0 <= off < 4 * flat.numel() and W.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr():
        return off // 4
    return -1


def bf16_copy(W):
    """bf16 copy of an fp32 master weight for the bf16 GEMMs (parameters stay fp32)."""
    if W.dtype == BF16:
        return W
    sh = BF16_SHADOW
    if sh is not None and W.is_contiguous():
        o = _view_of(sh[0], W)
        if o >= 0:
            _shadow_fresh(o, W.numel())
            return sh[1][o: o + W.numel()].view(W.shape)
    return W.detach().to(BF16)


def set_split_shadow(f32, planes, planes_t=None, desc=None, index=None, ntiles=0):
    """planes: [3, n] bf16 mirror of the flat buffer; planes_t (optional): the same with every registered matrix stored TRANSPOSED at
    its offset; desc / ntiles: device int32 [nmat, 4] table of dhz_split3_planes_t and its tile count; index: {(offset, rows, cols)} of
    the registered matrices."""
    global SPLIT_SHADOW
    SPLIT_SHADOW = None if f32 is None else [f32, planes[0], planes[1], planes[2], planes_t, desc, index or set(), int(ntiles)]


def refresh_split_shadow():
    sh = SPLIT_SHADOW
    if sh is not None:
        _lib.call("dhz_split3_planes", sh[0].data_ptr(), sh[0].numel(), sh[1].data_ptr(), sh[2].data_ptr(), sh[3].data_ptr(), _stream())
        if sh[4] is not None:
            pt, desc = sh[4], sh[5]
            _lib.call("dhz_split3_planes_t", sh[0].data_ptr(), pt[0].data_ptr(), pt[1].data_ptr(), pt[2].data_ptr(), desc.data_ptr(),
                      desc.shape[0], sh[7], _stream())


def split_planes_t(W):
    """(hi, mid, lo) planes of W^T ([K, N] row-major for W [N, K]) when FlatAdamW keeps them for this matrix (every Linear weight of
    the flat buffer; the adjacent Q / K / V weights as ONE packed [3C, C] matrix), else None."""
    o = _t_offset(SPLIT_SHADOW, 4, 6, W)
    if o < 0:
        return None
    n = W.numel()
    _shadow_fresh(o, n)
    pt = SPLIT_SHADOW[4]
    return pt[0][o: o + n], pt[1][o: o + n], pt[2][o: o + n]


def split_planes(W):
    """(hi, mid, lo): the three bf16 truncation pieces of a contiguous fp32 weight (hi + mid + lo == W exactly) - views of
    FlatAdamW's planes when W lives in its flat buffer, otherwise one dhz_split3_planes launch."""
    assert W.dtype == torch.float32 and W.is_contiguous() and W.numel() % 8 == 0
    sh = SPLIT_SHADOW
    if sh is not None:
        o = _view_of(sh[0], W)
        if o >= 0 and o % 8 == 0:
            n = W.numel()
            _shadow_fresh(o, n)
            return sh[1][o: o + n], sh[2][o: o + n], sh[3][o: o + n]
    pl = torch.empty((3, W.numel()), device=W.device, dtype=BF16)
    _lib.call("dhz_split3_planes", _p(W), W.numel(), pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), _stream())
    _RECENT.append(pl)
    return pl[0], pl[1], pl[2]


_NO_TPLANES = bool(os.environ.get("DHZ_S6_NO_TPLANES"))       # diagnostics: backward-data through the transposed-read kernel
RES_EPILOGUE = not os.environ.get("DHZ_NO_RES_EPILOGUE")        # A/B switch: K4 / the DropPath row factor as a pass of its own


def _route6(T, contraction, out, dgrad):
    """which kernel takes a six-term GEMM of T tokens (measured per shape on the config-2 step, tools/bench_split6.py):
    'new' = csrc/split6_gemm.hip (pre-split weight planes; 256 x 128 / 128 x 128 tiles), 'old' = csrc/linear_split.hip (both
    operands split in the kernel; 128 x 64 tiles, two workgroups per CU: ahead on narrow outputs and few-tile problems),
    'f32' = the fp32 pipe (HBM-bound shapes where the split buys nothing)."""
    if contraction % 32 or out % 32 or contraction < 64 or out < 64:
        return "f32"
    old_ok = contraction % 64 == 0 and out % 64 == 0
    new_ok = not dgrad or out % 64 == 0
    if T <= 2048 and out < 2048 and old_ok:
        return "old"
    if dgrad and out == 64 and old_ok:
        return "old"
    if not dgrad and contraction <= 64 and out % 128 and T >= (1 << 19):
        return "f32"
    if new_ok and out <= 2048:
        return "new"
    return "old" if old_ok else "f32"


def _route(product, T, contraction, out, bf16, ld, HW=0, tplanes=False):
    """THE answer to "which kernel takes this token-Linear product", from numbers and switches alone.
    product: 'fwd' (y = x W^T + b), 'fwd_res' (the same with the residual epilogue over images of HW tokens), 'dgrad' (dx = dy W; the
    contraction runs over W's rows), 'dgrad_rs' (the same with a factor per image of HW rows); bf16: storage dtype of the activations;
    ld: their row stride; tplanes: the optimizer keeps a copy of W^T in the operand format of this dtype.  Returns
      'bf16'     bf16 operands, fp32 accumulation                        'bf16_t'   ... the FORWARD kernel on the bf16 copy of W^T
      'split6'   six-term, pre-split weight planes (split6_gemm.hip)     'split6_t' ... the FORWARD kernel on the planes of W^T
      'split'    six-term, both operands split in the kernel             'split3'   the three-term experiment
      'f32'      the fp32 matrix pipe
      'two'      (fwd_res / dgrad_rs only) no single kernel: the plain product, then dhz_reverse_residual_*_dt."""
    back = product in ("dgrad", "dgrad_rs")
    fused_rows = product in ("fwd_res", "dgrad_rs")
    t_form = back and tplanes and not _NO_TPLANES
    if bf16:
        if fused_rows:
            ok = product == "fwd_res" and RES_EPILOGUE and HW % 64 == 0 and out % 64 == 0 and contraction % 64 == 0 and ld % 8 == 0
            return "bf16" if ok else "two"
        return "bf16_t" if t_form else "bf16"
    if SPLIT_BF16 == 6 and ld % 4 == 0 and (not fused_rows or (RES_EPILOGUE and HW % 64 == 0)):
        # backward-data asks two different questions: "is W^T a forward problem for the plane kernel" (it then needs no transposed
        # fragment reads), and only if not, "which backward-data kernel"
        r = _route6(T, contraction, out, back and not t_form)
        if t_form:
            return "split6_t" if r == "new" else _route(product, T, contraction, out, bf16, ld, HW, False)
        if product == "dgrad_rs":
            return "split" if r == "old" else "two"          # (the plane backward-data kernel has no row-factor form)
        if r != "f32":
            return "split6" if r == "new" else "split"
    if fused_rows:
        return "two"
    if SPLIT_BF16 == 3 and contraction >= SPLIT_MIN_K and contraction % 64 == 0 and out % 64 == 0:
        return "split3"
    return "f32"


def _terms():
    """3 or 6 for the split kernels (True counts as 3)"""
    return 6 if SPLIT_BF16 == 6 else 3


def _timed(name):
    """(list, start event) when bench.py collects HIP-event timings under this KERNEL_TIMING key, else None: the event is recorded on
    the launch stream right before the kernel it brackets."""
    lst = KERNEL_TIMING.get(name) if KERNEL_TIMING is not None else None
    if lst is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return lst, e0


def _timed_end(ev, *tail):
    """appends (start event, end event, *tail)"""
    if ev is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        ev[0].append((ev[1], e1) + tail)


def _ptr_array(ptrs):
    """device-pointer list -> void** argument"""
    return ctypes.cast((ctypes.c_void_p * len(ptrs))(*ptrs), ctypes.c_void_p)


def _int_array(vals):
    return ctypes.cast((ctypes.c_int * len(vals))(*vals), ctypes.c_void_p)


# KERNEL_TIMING key and issued FLOPs per multiply-add of a route (six products per multiply-add in the six-term kernels)
_GEMM_TIMING = {"bf16": ("dhz_linear_bf16", 2.0), "bf16_t": ("dhz_linear_bf16", 2.0), "split6": ("dhz_linear_split6", 12.0),
                "split6_t": ("dhz_linear_split6", 12.0), "split": ("dhz_linear_split6", 12.0)}


def _gemm(route, name, T, N, K, *args):
    key, flops = _GEMM_TIMING.get(route, (None, 0.0))
    ev = _timed(key)
    _lib.call(name, *args, _stream())
    _timed_end(ev, flops * T * N * K)


def _weight_operand(route, W):
    """the pointer argument(s) that stand for W on this route, and the trailing term count of the kernels that split in flight"""
    if route in ("split6", "split6_t"):
        return tuple(_p(pl) for pl in (split_planes(W) if route == "split6" else split_planes_t(W))), ()
    if route in ("bf16", "bf16_t"):
        return (_p(bf16_copy(W) if route == "bf16" else bf16_copy_t(W)),), ()
    return (_p(W),), {"split": (6,), "split3": (3,)}.get(route, ())


def gemm_fwd(x, W, b=None):
    """y[T,N] = x[T,K] W[N,K]^T + b.  x: rows of K contiguous elements (any row stride)."""
    _require_gpu(x, W, b)
    T, K = x.shape
    N = W.shape[0]
    assert x.stride(1) == 1 and W.shape[1] == K
    W = W if W.is_contiguous() else W.contiguous()
    y = torch.empty((T, N), device=x.device, dtype=x.dtype)
    route = _route("fwd", T, K, N, x.dtype == BF16, x.stride(0))
    name = {"bf16": "dhz_linear_fwd_bf16", "split6": "dhz_linear_fwd_split6", "split": "dhz_linear_fwd_split", "split3": "dhz_linear_fwd_split",
            "f32": "dhz_linear_fwd"}[route]
    w, terms = _weight_operand(route, W)
    _gemm(route, name, T, N, K, _p(x), x.stride(0), *w, _p(b), _p(y), N, T, N, K, *terms)
    return y


def gemm_fwd_res(x, W, b, res, scale, B, Hres, Wres, shift, windowed):
    """out = res + scale[image] * (x W^T + b) with the rows stored at their token-order position: K4 (window reverse, un-roll,
    DropPath factor, residual; M1:859-873) as the EPILOGUE of the out-projection / linear2 GEMM (csrc/tok_epilogue.h).  x: [T, K]
    (window order when `windowed`, the order dhz_ln_partition_fwd writes); res: [T, N] in token order; scale: [B] or None.  Shapes /
    arithmetic the epilogue kernels do not cover run the GEMM and dhz_reverse_residual_fwd as two launches."""
    _require_gpu(x, W, b, res, scale)
    T, K = x.shape
    N = W.shape[0]
    HW = Hres * Wres
    assert x.stride(1) == 1 and W.shape[1] == K and res.is_contiguous() and T == B * HW and x.dtype == res.dtype
    W = W if W.is_contiguous() else W.contiguous()
    out = torch.empty_like(res)
    win = 1 if windowed else 0
    route = _route("fwd_res", T, K, N, x.dtype == BF16, x.stride(0), HW)
    if route == "two":
        y = gemm_fwd(x, W, b)
        _lib.call("dhz_reverse_residual_fwd_dt", _p(y), _p(res), _p(scale), _p(out), B, Hres, Wres, N, shift, win, _dt(res), _stream())
        return out
    name = {"bf16": "dhz_linear_fwd_bf16_res", "split6": "dhz_linear_fwd_split6_res", "split": "dhz_linear_fwd_split_res"}[route]
    w, terms = _weight_operand(route, W)
    _gemm(route, name, T, N, K, _p(x), x.stride(0), *w, _p(b), _p(res), _p(scale), _p(out), N, T, N, K, HW, Hres, Wres, shift, win, *terms)
    return out


def gemm_dgrad(dy, W, row_scale=None):
    """dx[T,K] = dy[T,N] W[N,K].  row_scale = (scale[B], rows_per_image): dx rows carry the per-image factor (the DropPath factor of
    the branch in the backward pass) - in the epilogue of the six-term kernels, a pass of its own elsewhere."""
    _require_gpu(dy, W)
    T, N = dy.shape
    K = W.shape[1]
    assert dy.stride(1) == 1 and W.shape[0] == N
    W = W if W.is_contiguous() else W.contiguous()
    bf16 = dy.dtype == BF16
    tplanes = (_t_offset(BF16_SHADOW, 2, 4, W) if bf16 else _t_offset(SPLIT_SHADOW, 4, 6, W)) >= 0
    sc, rows = row_scale if row_scale is not None else (None, 0)
    assert row_scale is None or T % rows == 0
    route = _route("dgrad" if row_scale is None else "dgrad_rs", T, N, K, bf16, dy.stride(0), rows, tplanes)
    if route == "two":
        dx = gemm_dgrad(dy, W)
        out = torch.empty_like(dx)
        _lib.call("dhz_reverse_residual_bwd_dt", _p(dx), _p(sc), _p(out), T // rows, rows, 1, K, 0, 0, _dt(dx), _stream())
        return out
    dx = torch.empty((T, K), device=dy.device, dtype=dy.dtype)
    w, terms = _weight_operand(route, W)
    if route in ("split6_t", "bf16_t"):
        # dx = dy . W = dy . (W^T)^T: the FORWARD kernel on the optimizer's copy of W^T - no transposed fragment reads
        if row_scale is not None:
            _gemm(route, "dhz_linear_fwd_split6_res", T, N, K, _p(dy), dy.stride(0), *w, None, None, _p(sc), _p(dx), K, T, K, N, rows, 0, 0, 0, 0)
        else:
            _gemm(route, "dhz_linear_fwd_split6" if route == "split6_t" else "dhz_linear_fwd_bf16", T, N, K, _p(dy), dy.stride(0), *w, None,
                  _p(dx), K, T, K, N)
    elif row_scale is not None:
        _gemm(route, "dhz_linear_dgrad_split_scaled", T, N, K, _p(dy), dy.stride(0), *w, _p(sc), _p(dx), K, T, N, K, rows, *terms)
    else:
        name = {"bf16": "dhz_linear_dgrad_bf16", "split6": "dhz_linear_dgrad_split6", "split": "dhz_linear_dgrad_split",
                "split3": "dhz_linear_dgrad_split", "f32": "dhz_linear_dgrad"}[route]
        _gemm(route, name, T, N, K, _p(dy), dy.stride(0), *w, _p(dx), K, T, N, K, *terms)
    return dx


# ----------------------------------------------------------------------------- K3 / K7
# The padding mask of any-size evaluation (M1:791-800) travels as ONE 64-bit word per window (bit i: token i is padding) instead of a
# [B nW, N, N] fp32 tensor; the kernels form the -100 term from it in registers.  DHZ_PAD_BITS=0 restores the tensor everywhere (A/B).
PAD_BITS = os.environ.get("DHZ_PAD_BITS", "1") != "0"


def pad_bits_cover(mask, H, W):
    """padding words exist for this mask on an H x W map: [B, 1, Himg, Wimg] with Himg, Wimg whole multiples of H, W (what the model's
    stages give).  Any other mask - another ratio, more channels - keeps the tensor route, which resamples with F.interpolate."""
    return mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] % H == 0 and mask.shape[3] % W == 0


_WARNED_PAD_GRAD = False


def warn_pad_under_grad():
    """once: a masked forward with gradients enabled does not reach the fused window-attention kernel"""
    global _WARNED_PAD_GRAD
    if not _WARNED_PAD_GRAD:
        _WARNED_PAD_GRAD = True
        import warnings
        warnings.warn("dehaze_hip: a forward with a padding mask runs with gradients enabled: its blocks take the unfused kernel chain "
                      "(with padding words); run any-size evaluation under torch.no_grad() to reach the fused window-attention kernel",
                      stacklevel=3)


def pad_window_bits(mask, H, W, win=8):
    """mask [B, 1, Himg, Wimg] fp32 -> [B (H / win) (W / win)] int64 words (the bit pattern of a uint64) for a block that works on an
    H x W map: bit i of word b = (window_partition(F.interpolate(mask, (H, W)))[b, i] != 0), the windows in window_partition's order
    (dhz_pad_window_bits; Himg % H == 0 and Wimg % W == 0)"""
    _win_of(win * win)
    _require_gpu(mask)
    assert mask.dim() == 4 and mask.shape[1] == 1, f"padding mask {tuple(mask.shape)}: [B, 1, Himg, Wimg] expected"
    m = mask.contiguous().float()
    B, _, Himg, Wimg = m.shape
    bits = torch.empty((B * (H // win) * (W // win),), device=m.device, dtype=torch.int64)
    _lib.call("dhz_pad_window_bits", _p(m), _p(bits), B, Himg, Wimg, H, W, win, _stream())
    return bits


def _pad_nw(pad, mask, B_, nW):
    """windows per image of a launch with padding words: the shift mask's, else the caller's, else one image"""
    assert pad.is_cuda and pad.dtype == torch.int64 and pad.numel() == B_ and pad.is_contiguous(), \
        f"padding words {tuple(pad.shape)} {pad.dtype} on {pad.device} for {B_} windows"
    return mask.shape[0] if mask is not None else (nW or B_)


# Every window-side op below makes ONE call, to the `_w` entry of include/dehaze_hip.h with win = _win_of(N): at win = 8 that entry runs
# the function behind the entry without `_w` (dhz_ps_attn_fwd_dt, dhz_bias_gather, ...) with the same arguments - the same kernel
# instance, the same bits (tests/test_gpu_win4_kernels.py pins it) - so there is nothing for Python to choose.
def _pad_splice(pad, mask, B_, nW):
    """("_pad", the pad word as the argument behind `mask`, windows per image) of a launch with padding words, else ("", nothing, the
    shift mask's window count)"""
    if pad is None:
        return "", (), (mask.shape[0] if mask is not None else 1)
    return "_pad", (_p(pad),), _pad_nw(pad, mask, B_, nW)


def ps_attn_fwd_launch(qkv, idx, bias, mask, out, rank, B_, H, d, N=NTOK, pad=None, nW=None):
    """dhz_ps_attn_fwd_w on a packed [T, 3C] buffer (columns [Q | K | V]), inside bench.py's timing bracket; pad: the padding words of
    the B_ windows (dhz_ps_attn_fwd_w_pad), nW: windows per image"""
    C, es, base = H * d, qkv.element_size(), qkv.data_ptr()
    sfx, padarg, nW = _pad_splice(pad, mask, B_, nW)
    ev = _timed("dhz_ps_attn_fwd")
    _lib.call("dhz_ps_attn_fwd_w" + sfx, base, base + es * C, base + 2 * es * C, 3 * C, _p(idx), _p(bias), _p(mask), *padarg, _p(out), C,
              _p(rank), B_, H, nW, d, _win_of(N), _dt(qkv), _stream())
    _timed_end(ev, B_ * H * 4 * N * d * es)


def ps_attn_bwd_launch(qkv, dqkv, bias, mask, rank, dout, dpart, B_, H, d, N=NTOK, pad=None, nW=None):
    """dhz_ps_attn_bwd_w: packed qkv / dqkv [T, 3C]; pad / nW as in ps_attn_fwd_launch (dhz_ps_attn_bwd_w_pad)"""
    C, es, base, gb = H * d, qkv.element_size(), qkv.data_ptr(), dqkv.data_ptr()
    sfx, padarg, nW = _pad_splice(pad, mask, B_, nW)
    _lib.call("dhz_ps_attn_bwd_w" + sfx, base, base + es * C, base + 2 * es * C, 3 * C, _p(bias), _p(mask), *padarg, _p(rank), _p(dout), C,
              gb, gb + es * C, gb + 2 * es * C, 3 * C, _p(dpart), B_, H, nW, d, _win_of(N), _dt(qkv), _stream())


def ps_attn_bwd_parts(B_, H, d, N=NTOK):
    """rows of the [parts, N, N] partial bias gradient that dhz_ps_attn_bwd_w / dhz_dense_attn_bwd_w write (dhz_ps_attn_bwd_parts_w)"""
    return _lib.load().dhz_ps_attn_bwd_parts_w(B_, H, d, _win_of(N))


def bias_tile(table, H, N=NTOK):
    """[H, N, N] relative-position bias of a [(2 win - 1)^2, H] table (M1:408-410; dhz_bias_gather_w)"""
    win = _win_of(N)
    assert tuple(table.shape) == ((2 * win - 1) ** 2, H), f"bias table {tuple(table.shape)} for {win}x{win} windows, {H} heads"
    bias = torch.empty((H, N, N), device=table.device, dtype=torch.float32)
    _lib.call("dhz_bias_gather_w", _p(table.contiguous()), _p(bias), H, win, _stream())
    return bias


def bias_table_grad(dpart, parts, H, N=NTOK, out=None, accumulate=False):
    """[(2 win - 1)^2, H] table gradient from the partial [parts, N, N] tiles of a backward kernel (dhz_bias_table_grad_w), written to a
    new tensor or to `out`, which it is added to when accumulate"""
    win = _win_of(N)
    if out is None:
        out = torch.empty(((2 * win - 1) ** 2, H), device=dpart.device, dtype=torch.float32)
    _lib.call("dhz_bias_table_grad_w", _p(dpart), parts, _p(out), H, int(accumulate), win, _stream())
    return out


class _PSWindowAttention(Function):
    """ProbAttention.forward (ATT:287-342) on a packed QKV buffer.

    qkv   : [T, 3C] (T = B_*N window-ordered tokens; columns [Q | K | V], each [H, d])
    table : [(2 win - 1)^2, H] relative position bias table, or None (options.is_relative_position_bias False)
    idx   : [N, u] uint8 sampled keys ([64, 25] for 8 x 8 windows, [16, 15] for 4 x 4: N is taken from it);  mask: [nW, N, N] or None
    pad   : [B_] int64 padding words (pad_window_bits) or None; nW: windows per image (with pad and without mask)
    """

    @staticmethod
    def forward(ctx, qkv, table, idx, mask, H, d, pad=None, nW=None):
        _require_gpu(qkv, table, idx, mask)
        T, C3 = qkv.shape
        C = H * d
        N = idx.shape[0]
        assert tuple(idx.shape) == ((NTOK, NTOP) if _win_of(N) == 8 else (NTOK16, NTOP16)), f"sample table {tuple(idx.shape)}"
        assert C3 == 3 * C and T % N == 0 and qkv.is_contiguous() and (mask is None or tuple(mask.shape[1:]) == (N, N))
        B_ = T // N
        out = torch.empty((T, C), device=qkv.device, dtype=qkv.dtype)
        rank = torch.empty((B_ * H * N,), device=qkv.device, dtype=torch.uint8)
        bias = bias_tile(table, H, N) if table is not None else None
        ps_attn_fwd_launch(qkv, idx, bias, mask, out, rank, B_, H, d, N, pad, nW)
        ctx.save_for_backward(qkv, bias, mask, rank, pad)
        ctx.dims = (B_, H, d, N, nW)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bias, mask, rank, pad = ctx.saved_tensors
        B_, H, d, N, nW = ctx.dims
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dpart, dtable = None, None
        parts = ps_attn_bwd_parts(B_, H, d, N)
        if bias is not None:
            dpart = torch.empty((parts, N, N), device=qkv.device, dtype=torch.float32)
        ps_attn_bwd_launch(qkv, dqkv, bias, mask, rank, dout, dpart, B_, H, d, N, pad, nW)
        if bias is not None:
            dtable = bias_table_grad(dpart, parts, H, N)
        return dqkv, dtable, None, None, None, None, None, None


def ps_window_attention(qkv, table, idx, mask, H, d, pad=None, nW=None):
    return _PSWindowAttention.apply(qkv, table, idx, mask, H, d, pad, nW)


def ps_window_attention_rank(qkv, table, idx, mask, H, d):
    """Forward only, fp32 storage; also returns the saved selection ranks [B_,H,N] (tests / diagnostics)."""
    assert qkv.dtype == torch.float32, qkv.dtype
    T = qkv.shape[0]
    C = H * d
    N = idx.shape[0]
    B_ = T // N
    out = torch.empty((T, C), device=qkv.device, dtype=torch.float32)
    rank = torch.empty((B_, H, N), device=qkv.device, dtype=torch.uint8)
    bias = bias_tile(table, H, N) if table is not None else None
    ps_attn_fwd_launch(qkv, idx, bias, mask, out, rank, B_, H, d, N)
    return out, rank


class _DenseWindowAttention(Function):
    """Dense window attention (My_model twin, M0:428-492) on a packed [T,3C] QKV buffer."""

    @staticmethod
    def forward(ctx, qkv, table, mask, H, d, scale, N):
        _require_gpu(qkv, table, mask)
        T, C3 = qkv.shape
        C = H * d
        assert C3 == 3 * C and T % N == 0 and qkv.is_contiguous() and (mask is None or tuple(mask.shape[1:]) == (N, N))
        B_ = T // N
        out = torch.empty((T, C), device=qkv.device, dtype=torch.float32)
        bias = bias_tile(table, H, N)
        nW = mask.shape[0] if mask is not None else 1
        base = qkv.data_ptr()
        _lib.call("dhz_dense_attn_fwd_w", base, base + 4 * C, base + 8 * C, 3 * C, _p(bias), _p(mask), _p(out), C, B_, H,
                  nW, d, float(scale), _win_of(N), _stream())
        ctx.save_for_backward(qkv, bias, mask)
        ctx.dims = (B_, H, d, nW, float(scale), N)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bias, mask = ctx.saved_tensors
        B_, H, d, nW, scale, N = ctx.dims
        C = H * d
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        parts = ps_attn_bwd_parts(B_, H, d, N)       # (at win = 8 the count does not depend on d: it is dhz_ps_attn_bwd_parts(B_, H))
        dpart = torch.empty((parts, N, N), device=qkv.device, dtype=torch.float32)
        base, gb = qkv.data_ptr(), dqkv.data_ptr()
        _lib.call("dhz_dense_attn_bwd_w", base, base + 4 * C, base + 8 * C, 3 * C, _p(bias), _p(mask), _p(dout), C,
                  gb, gb + 4 * C, gb + 8 * C, 3 * C, _p(dpart), B_, H, nW, d, scale, _win_of(N), _stream())
        return dqkv, bias_table_grad(dpart, parts, H, N), None, None, None, None, None


def dense_window_attention(qkv, table, mask, H, d, scale, N=NTOK):
    """N: tokens per window (64 or 16)"""
    _win_of(N)
    return _DenseWindowAttention.apply(qkv, table, mask, H, d, scale, N)


def shift_mask(Hres, Wres, shift, device, win=8):
    """[nW, win^2, win^2] 0/-100 mask of M1:803-836 (cached by callers; depends only on the geometry)."""
    N = win * win
    _win_of(N)
    m = torch.empty(((Hres // win) * (Wres // win), N, N), device=device, dtype=torch.float32)
    _lib.call("dhz_shift_mask_w", _p(m), Hres, Wres, shift, win, _stream())
    return m


# ----------------------------------------------------------------------------- token-major Linear (K2 / K4 / K5 GEMMs)
# Called with every parameter whose gradient has just been accumulated IN PLACE by a wgrad kernel (autograd's
# AccumulateGrad - and therefore its post-accumulate hooks - is bypassed for those); the gradient reducer
# installs itself here to keep its bucket bookkeeping.
GRAD_READY = None
# [zeroed fp32 tensor, bump offset, weakref(owner)]: FlatAdamW.zero_grad() zeroes it together with the flat gradient buffer and resets the
# offset; zeros_f32 carves accumulation targets of the backward pass out of it (valid until the next zero_grad)
ZERO_SCRATCH = None


def zeros_f32(shape, device):
    """torch.zeros(shape, fp32) - from the optimizer's pre-zeroed scratch region when one is registered for this device and has room
    (no fill launch), else a fresh allocation.  Only for temporaries of ONE backward pass."""
    n = 1
    for d in shape:
        n *= int(d)
    zs = ZERO_SCRATCH
    if zs is not None and zs[2]() is not None and zs[0].device == device:
        off = (zs[1] + 7) // 8 * 8
        if off + n <= zs[0].numel():
            zs[1] = off + n
            return zs[0][off: off + n].view(shape)
    return torch.zeros(shape, device=device, dtype=torch.float32)


def _grad_buf(p):
    """Zero-initialised, contiguous .grad of a leaf parameter (the optimizer's flat-buffer view when FlatAdamW is in
    use), or None when in-place accumulation is not possible."""
    if not (p.is_leaf and p.requires_grad):
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad if p.grad.is_contiguous() else None


def _grad_pair(w, b):
    """(.grad of w, .grad of b or None) when the gradients of a weight and its optional bias can BOTH be accumulated in place (announce
    them with _ready afterwards), else None: the caller hands fresh tensors to autograd."""
    gw, gb = _grad_buf(w), _grad_buf(b) if b is not None else None
    return (gw, gb) if gw is not None and (b is None or gb is not None) else None


def _ready(*params):
    if GRAD_READY is not None:
        for p in params:
            if p is not None:
                GRAD_READY(p)


def _wgrad_launch(dy, off, x, targets, row_scale):
    """dw[N,K] += dy[:, off:off+N]^T x, db += column sums for consecutive column blocks of dy; targets: [(N, dw, db or None)], fp32
    accumulators.  Blocks of equal width (the Q / K / V projections) share ONE launch that reads x once."""
    T, K = x.shape
    bf16 = dy.dtype == BF16
    assert row_scale is None or (not bf16 and len(targets) == 1)
    rs = (_p(row_scale[0]), int(row_scale[1])) if row_scale is not None else (None, 0)
    # fp32 storage: the contraction over T on the bf16 pipe with split operands (csrc/linear_split.hip) wherever its 64-tiles fit
    split = not bf16 and SPLIT_BF16 and T % 64 == 0 and K % 64 == 0 and all(N % 64 == 0 for N, _, _ in targets)
    same = 1 < len(targets) <= 4 and len({N for N, _, _ in targets}) == 1 and len({db is None for _, _, db in targets}) == 1
    for grp in ([targets] if same else [[t] for t in targets]):
        n, N = len(grp), grp[0][0]
        lead = (dy.data_ptr() + dy.element_size() * off, dy.stride(0), _p(x), x.stride(0), T)
        if bf16 or split or n > 1:
            arrays = (_ptr_array([_p(dw) for _, dw, _ in grp]), _ptr_array([_p(db) for _, _, db in grp]))
            if bf16:
                _refuse_bf16_deterministic("linear weight gradient")
                _lib.call("dhz_linear_wgrad_bf16", *lead, n, N, K, *arrays, _stream())
            elif split:
                ev = _timed("dhz_linear_wgrad_split")
                _lib.call("dhz_linear_wgrad_split", *lead, n, N, K, *arrays, *rs, _terms(), _stream())
                _timed_end(ev, 2.0 * _terms() * T * n * N * K)
            else:
                _lib.call("dhz_linear_wgrad_multi", *lead, n, N, K, *arrays, _stream())
        elif row_scale is not None:
            _lib.call("dhz_linear_wgrad_rs", *lead, N, K, _p(grp[0][1]), _p(grp[0][2]), *rs, _stream())
        else:
            _lib.call("dhz_linear_wgrad", *lead, N, K, _p(grp[0][1]), _p(grp[0][2]), _stream())
        off += n * N


def linear_wgrad(dy, off, x, params, row_scale=None):
    """Weight / bias gradients of the Linears [(W, b or None)] whose outputs are consecutive column blocks of dy from column `off`, from
    dy [T, .] and their common input x [T, K].  Returns the autograd slots (dW_1, db_1, dW_2, ...): None for a frozen Linear and for
    gradients that were accumulated in place into .grad (leaf parameters; GRAD_READY is told), fresh tensors otherwise.
    row_scale = (scale[B], rows_per_scale): row t of dy counts as scale[t // rows_per_scale] * dy[t] (fp32, one Linear only).
    The kernels' shape contract: bf16 storage - T, N, K in 64s; fp32 - T, N and K in 16s (a 4x4 bottleneck has 16 tokens per image: any
    batch trains; the 16-wide tile forms exist for the embed_dim = 16 model, csrc/linear_wgrad.hip).  With a row_scale, rows_per_scale
    is a multiple of 32.  There is deliberately no library fallback."""
    T, K = x.shape
    q, tq = (64, 64) if dy.dtype == BF16 else (16, 16)
    slots, targets, inplace = [], [], []
    for w, b in params:
        pair = None
        if not w.requires_grad and (b is None or not b.requires_grad):
            dw = db = None                                     # frozen Linear: nothing to compute (its columns are skipped below)
        elif T % tq or K % q or w.shape[0] % q:
            raise RuntimeError(f"dehaze_hip: Linear weight gradient for T={T}, N={w.shape[0]}, K={K}: the HIP kernel needs T in {tq}s "
                               f"and N, K in {q}s for {dy.dtype} (there is deliberately no library fallback)")
        else:
            pair = _grad_pair(w, b)
            # handed to autograd, which may keep them: fresh tensors, never the optimizer's zeroed scratch (valid until zero_grad only)
            dw, db = pair or (torch.zeros(w.shape, device=w.device, dtype=torch.float32),
                              torch.zeros(b.shape, device=b.device, dtype=torch.float32) if b is not None else None)
            inplace += [w, b] if pair else []
        targets.append((w.shape[0], dw, db))
        slots += [None, None] if dw is None or pair else [dw, db]
    # one call for all of them when every gradient lands in place (equal widths then share a launch), else one per live Linear at its
    # column offset
    if len(inplace) == 2 * len(params):
        _wgrad_launch(dy, off, x, targets, row_scale)
    else:
        for N, dw, db in targets:
            if dw is not None:
                _wgrad_launch(dy, off, x, [(N, dw, db)], row_scale)
            off += N
    _ready(*inplace)
    return tuple(slots)


# dx, dW and db of a Linear from ONE pass over dy (csrc/linear_bwd_pair.hip) where dy is the wide tensor of its block: LeFF linear1 and the
# packed Q / K / V projection at C = 32 / 64.  DHZ_LINEAR_BWD_PAIR=0: the two launches everywhere.  A shape (N, K) is listed only when the
# kernel beats gemm_dgrad + linear_wgrad by more than the spread between rounds on every map size it occurs at; a built shape that does
# not stays tested and undispatched.  Measured (tools/bench_linear_bwd_pair.py, bs 32, us, two launches -> one kernel; spreads 0.4 - 9.6;
# profiles/r09_linear_bwd_pair.txt): (128, 32) at 128 x 128 139 -> 104; (256, 64) at 64 x 64 82.3 -> 77.8, at 128 x 128 296 -> 216;
# (192, 64) at 64 x 64 67.6 -> 60.6, at 128 x 128 253 -> 169.  The config-2 step: -0.29 ms slowest on against fastest off, -0.46 ms by the means.
LINEAR_BWD_PAIR = os.environ.get("DHZ_LINEAR_BWD_PAIR", "1") != "0"
LINEAR_BWD_PAIR_BUILT = ((128, 32), (256, 64), (192, 64))
LINEAR_BWD_PAIR_SHAPES = ((128, 32), (256, 64), (192, 64))


def _bwd_pair_operands(dy, x, W, params):
    """(planes of W^T, [(dW, db or None)]) when dhz_linear_bwd_pair takes this backward, else None"""
    T, K = x.shape
    N = W.shape[0]
    if not LINEAR_BWD_PAIR or (N, K) not in LINEAR_BWD_PAIR_SHAPES or DETERMINISTIC or SPLIT_BF16 != 6 or T % 32:
        return None
    if dy.dtype != torch.float32 or x.dtype != torch.float32 or dy.stride(1) != 1 or x.stride(1) != 1 or dy.stride(0) % 4 or x.stride(0) % 4:
        return None
    if _p(dy) % 16 or _p(x) % 16 or len({w.shape[0] for w, _ in params}) != 1 or sum(w.shape[0] for w, _ in params) != N:
        return None
    if any(not w.requires_grad or (b is not None and not b.requires_grad) for w, b in params):
        return None
    planes = split_planes_t(W)
    if planes is None or any(_p(pl) % 16 for pl in planes):
        return None
    pairs = [_grad_pair(w, b) for w, b in params]
    return (planes, pairs) if all(pr is not None for pr in pairs) else None


def linear_bwd_pair(dy, x, W, params):
    """Backward of the Linears [(W_i, b_i or None)] of equal width whose outputs are the column blocks of dy [T, N] and whose common input
    is x [T, K]; W [N, K] = their weights stacked (cat_rows).  Returns (dx [T, K], the autograd slots of linear_wgrad): one kernel when
    everything it needs holds - fp32 storage, six-term arithmetic, not deterministic, W^T planes registered and aligned, every gradient
    accumulated in place, the shape listed and the switch on - else exactly gemm_dgrad + linear_wgrad."""
    W = W if W.is_contiguous() else W.contiguous()
    took = _bwd_pair_operands(dy, x, W, params)
    if took is None:
        return gemm_dgrad(dy, W), linear_wgrad(dy, 0, x, params)
    planes, pairs = took
    T, K = x.shape
    dx = torch.empty((T, K), device=dy.device, dtype=dy.dtype)
    _lib.call("dhz_linear_bwd_pair", _p(dy), dy.stride(0), _p(x), x.stride(0), *[_p(pl) for pl in planes], _p(dx), T, len(params),
              params[0][0].shape[0], K, _ptr_array([_p(gw) for gw, _ in pairs]), _ptr_array([_p(gb) for _, gb in pairs]), _stream())
    _ready(*[p for wb in params for p in wb])
    return dx, (None,) * (2 * len(params))


def cat_rows(ts):
    """torch.cat(ts, 0) for detached row blocks - WITHOUT a copy when they already sit back to back in memory, which is how
    FlatAdamW lays out the Q / K / V weights (and biases) of an attention layer in its flat parameter buffer.  Only for use
    where autograd does not track the result (inside Function.forward / backward)."""
    t0 = ts[0]
    end = t0.data_ptr() + t0.numel() * t0.element_size()
    base = t0.untyped_storage().data_ptr()          # same allocation, not merely neighbouring ones
    ok = t0.is_contiguous() and not t0.requires_grad
    for t in ts[1:]:
        ok = ok and t.is_contiguous() and not t.requires_grad and t.dtype == t0.dtype and t.device == t0.device \
            and t.shape[1:] == t0.shape[1:] and t.data_ptr() == end and t.untyped_storage().data_ptr() == base
        if not ok:
            break
        end += t.numel() * t.element_size()
    if not ok:
        return torch.cat(list(ts), 0)
    rows = sum(t.shape[0] for t in ts)
    shape = (rows,) + tuple(t0.shape[1:])
    return t0.as_strided(shape, t0.stride())


class _LinearTokens(Function):
    """y = x [W_1;..;W_n]^T + [b_1;..;b_n] for token-major x [T,K]: gemm_fwd forward, gemm_dgrad for the input gradient,
    linear_wgrad for the weight / bias gradients, which are accumulated in place into the parameters' .grad (the optimizer's flat
    gradient buffer)."""

    @staticmethod
    def forward(ctx, x, *wb):
        _require_gpu(x)
        params = [(wb[i], wb[i + 1]) for i in range(0, len(wb), 2)]
        if len(params) == 1:
            W, b = params[0]
        else:
            W = cat_rows([w.detach() for w, _ in params])
            b = cat_rows([b_.detach() for _, b_ in params])
        if x.dtype == BF16:
            W = bf16_copy(W)                # one cast per Linear and step: the copy is saved for the backward-data GEMM
        y = gemm_fwd(x, W, b)
        ctx.save_for_backward(x, W)
        ctx.params = params
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dy = dy.contiguous()
        dx = gemm_dgrad(dy, W) if ctx.needs_input_grad[0] else None
        return (dx,) + linear_wgrad(dy, 0, x, ctx.params)


class _GeluTokens(Function):
    """GELU between the two Linears of Mlp (M1:460-461) on dhz_gelu_fwd / dhz_gelu_bwd."""

    @staticmethod
    def forward(ctx, u):
        _require_gpu(u)
        u = u.contiguous()
        y = torch.empty_like(u)
        _lib.call("dhz_gelu_fwd_dt", _p(u), _p(y), u.numel(), _dt(u), _stream())
        ctx.save_for_backward(u)
        return y

    @staticmethod
    def backward(ctx, dy):
        (u,) = ctx.saved_tensors
        dy = dy.contiguous()
        du = torch.empty_like(u)
        _lib.call("dhz_gelu_bwd_dt", _p(dy), _p(u), _p(du), u.numel(), None, 0, _dt(u), _stream())
        return du


def gelu_tokens(u):
    return _GeluTokens.apply(u)


def linear_tokens(x, *wb):
    """x [T,K] (contiguous); wb = W1, b1, W2, b2, ...  ->  [T, sum N_i]."""
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (x,) + wb):
        params = [(wb[i], wb[i + 1]) for i in range(0, len(wb), 2)]
        W = params[0][0] if len(params) == 1 else torch.cat([w for w, _ in params], 0)
        b = params[0][1] if len(params) == 1 else torch.cat([b_ for _, b_ in params], 0)
        return gemm_fwd(x.contiguous(), W, b)
    return _LinearTokens.apply(x.contiguous(), *wb)


# ----------------------------------------------------------------------------- K1
class _LNPartition(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, Hres, Wres, shift, partition, win):
        _require_gpu(x, gamma, beta)
        x = x.contiguous()
        B, L, C = x.shape
        assert L == Hres * Wres
        y = torch.empty((B * L, C), device=x.device, dtype=x.dtype)
        stats = torch.empty((B * L, 2), device=x.device, dtype=torch.float32)
        _lib.call("dhz_ln_partition_fwd_w", _p(x), _p(gamma), _p(beta), _p(y), _p(stats), B, Hres, Wres, C, shift,
                  int(partition), win, _dt(x), _stream())
        ctx.save_for_backward(x, gamma, stats)
        ctx.geom = (B, Hres, Wres, C, shift, int(partition), win)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, stats = ctx.saved_tensors
        B, Hres, Wres, C, shift, partition, win = ctx.geom
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dgb = torch.zeros((2, C), device=x.device, dtype=torch.float32)
        _lib.call("dhz_ln_partition_bwd_w", _p(dy), _p(x), _p(gamma), _p(stats), None, _p(dx), dgb[0].data_ptr(),
                  dgb[1].data_ptr(), B, Hres, Wres, C, shift, partition, win, _dt(x), _stream())
        return dx, dgb[0], dgb[1], None, None, None, None, None


def ln_partition(x, gamma, beta, Hres, Wres, shift, win=8):
    """LayerNorm -> roll(-shift) -> window_partition  (M1:839-852).  [B,L,C] -> [B*nW*win*win, C].  dhz_ln_partition_fwd_w / _bwd_w: at
    win = 8 the kernel instances of dhz_ln_partition_fwd_dt / dhz_ln_partition_bwd_dt."""
    _win_of(win * win)
    return _LNPartition.apply(x, gamma, beta, Hres, Wres, shift, True, win)


def layer_norm_tokens(x, gamma, beta):
    """Plain LayerNorm over the last dim, tokens stay in place (norm2, M1:873). [B,L,C] -> [B*L, C]."""
    return _LNPartition.apply(x, gamma, beta, x.shape[1], 1, 0, False, 8)


# ----------------------------------------------------------------------------- K4 tail
class _ReverseResidual(Function):
    @staticmethod
    def forward(ctx, yw, shortcut, scale, Hres, Wres, shift, partition, win):
        _require_gpu(yw, shortcut, scale)
        shortcut = shortcut.contiguous()
        yw = yw.contiguous()
        B, L, C = shortcut.shape
        out = torch.empty_like(shortcut)
        _lib.call("dhz_reverse_residual_fwd_w", _p(yw), _p(shortcut), _p(scale), _p(out), B, Hres, Wres, C, shift,
                  int(partition), win, _dt(shortcut), _stream())
        ctx.save_for_backward(scale)
        ctx.geom = (B, Hres, Wres, C, shift, int(partition), tuple(yw.shape), win)
        return out

    @staticmethod
    def backward(ctx, dout):
        (scale,) = ctx.saved_tensors
        B, Hres, Wres, C, shift, partition, yshape, win = ctx.geom
        dout = dout.contiguous()
        dyw = torch.empty(yshape, device=dout.device, dtype=dout.dtype)
        _lib.call("dhz_reverse_residual_bwd_w", _p(dout), _p(scale), _p(dyw), B, Hres, Wres, C, shift, partition, win,
                  _dt(dout), _stream())
        return dyw, dout, None, None, None, None, None, None


def reverse_residual(yw, shortcut, scale, Hres, Wres, shift, win=8):
    """window_reverse -> roll(+shift) -> shortcut + drop_path(.)  (M1:859-872).  dhz_reverse_residual_fwd_w / _bwd_w: at win = 8 the
    kernel instances of dhz_reverse_residual_fwd_dt / dhz_reverse_residual_bwd_dt."""
    _win_of(win * win)
    return _ReverseResidual.apply(yw, shortcut, scale, Hres, Wres, shift, True, win)


def residual_scale(y, shortcut, scale):
    """shortcut + scale[b] * y with y already in token order (M1:873)."""
    return _ReverseResidual.apply(y, shortcut, scale, shortcut.shape[1], 1, 0, False, 8)


# ----------------------------------------------------------------------------- K5 middle
class _LeffDwconv(Function):
    @staticmethod
    def forward(ctx, u, w, b, Hres, Wres):
        _require_gpu(u, w, b)
        u = u.contiguous()
        B, L, Ch = u.shape
        assert L == Hres * Wres
        z = torch.empty_like(u)
        keep = any(ctx.needs_input_grad)
        t = torch.empty_like(u) if keep else None
        w = w.contiguous()
        _lib.call("dhz_leff_dwconv_fwd_dt", _p(u), _p(w), _p(b), _p(t), _p(z), B, Hres, Wres, Ch, _dt(u), _stream())
        if keep:
            ctx.save_for_backward(u, t, w)
        ctx.geom = (B, Hres, Wres, Ch)
        return z

    @staticmethod
    def backward(ctx, dz):
        u, t, w = ctx.saved_tensors
        B, Hres, Wres, Ch = ctx.geom
        dz = dz.contiguous()
        du = torch.empty_like(u)
        dwb = torch.zeros((Ch * 10,), device=u.device, dtype=torch.float32)
        _lib.call("dhz_leff_dwconv_bwd_dt", _p(dz), _p(u), _p(t), _p(w), _p(du), dwb.data_ptr(),
                  dwb.data_ptr() + 4 * Ch * 9, B, Hres, Wres, Ch, _dt(u), _stream())
        return du, dwb[:Ch * 9].view(Ch, 1, 3, 3), dwb[Ch * 9:], None, None


def leff_dwconv(u, w, b, Hres, Wres):
    """gelu(dwconv3x3(gelu(u)) + b) in token layout (M1:488, 514-520)."""
    return _LeffDwconv.apply(u, w, b, Hres, Wres)


# ----------------------------------------------------------------------------- K10
class _CharbonnierClamped(Function):
    @staticmethod
    def forward(ctx, x, y, eps, clamp01):
        _require_gpu(x, y)
        x = x.contiguous()
        y = y.contiguous()
        n = x.numel()
        acc = zeros_f32((), x.device)
        clamped = torch.empty_like(x) if clamp01 else None
        _lib.call("dhz_charbonnier_fwd", _p(x), _p(y), _p(clamped), _p(acc), n, float(eps), int(clamp01), _stream())
        ctx.save_for_backward(x, y)
        ctx.eps, ctx.clamp01 = float(eps), int(clamp01)
        if not clamp01:
            clamped = x.new_empty(0)
            ctx.mark_non_differentiable(clamped)
        return acc / n, clamped

    @staticmethod
    def backward(ctx, gloss, gclamp):
        x, y = ctx.saved_tensors
        dx = torch.empty_like(x)
        if gloss is None:
            gloss = torch.zeros((), device=x.device, dtype=torch.float32)
        gloss = gloss.contiguous().float()
        gclamp = gclamp.contiguous() if (gclamp is not None and ctx.clamp01) else None
        _lib.call("dhz_charbonnier_bwd", _p(x), _p(y), _p(gloss), _p(gclamp), _p(dx), x.numel(), ctx.eps,
                  1.0 / x.numel(), ctx.clamp01, _stream())
        return dx, None, None, None


def charbonnier_clamped(x, y, eps=1e-3):
    """(mean(sqrt((clamp(x,0,1)-y)^2 + eps^2)), clamp(x,0,1))  - TR:230 + losses.py:48-52 in one pass."""
    return _CharbonnierClamped.apply(x, y, eps, True)


def charbonnier(x, y, eps=1e-3):
    """CharbonnierLoss.forward(x, y) - losses.py:48-52 (no clamp)."""
    return _CharbonnierClamped.apply(x, y, eps, False)[0]


# ----------------------------------------------------------------------------- K12
def adamw_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, p16=None):
    """In-place AdamW over flat fp32 buffers (torch.optim.AdamW semantics, TR:90-92); p16: optional bf16 buffer that receives
    the updated parameters in the same pass (the weight copy of the bf16 GEMMs)."""
    _require_gpu(p, g, m, v)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert p16 is None or (p16.dtype == BF16 and p16.is_contiguous() and p16.numel() == p.numel())
    _lib.call("dhz_adamw_step_shadow", _p(p), _p(g), _p(m), _p(v), _p(p16), p.numel(), float(lr), float(beta1), float(beta2),
              float(eps), float(weight_decay), int(step), float(grad_scale), _stream())


# ----------------------------------------------------------------------------- K9b
class _ThinConv(Function):
    """Output projection: tokens [B, H*W, C] -> Conv2d(C, 3, 3x3, pad 1) -> [B, 3, H, W]; weight and bias gradients are
    accumulated in place when the parameters are leaves."""

    @staticmethod
    def forward(ctx, x, w, b, H, W):
        _require_gpu(x, w)
        x = x.contiguous()
        B, L, C = x.shape
        assert L == H * W and w.shape == (3, C, 3, 3)
        wc = w.contiguous()
        y = torch.empty((B, 3, H, W), device=x.device, dtype=torch.float32)
        _lib.call("dhz_thin_conv3x3_fwd_dt", _p(x), _p(wc), _p(b), _p(y), B, H, W, C, _dt(x), _stream())
        ctx.save_for_backward(x, wc)
        ctx.params, ctx.geom = (w, b), (B, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wc = ctx.saved_tensors
        w, b = ctx.params
        B, H, W, C = ctx.geom
        dy = dy.contiguous().float()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("dhz_thin_conv3x3_dgrad_dt", _p(dy), _p(wc), _p(dx), B, H, W, C, _dt(x), _stream())
        pair = _grad_pair(w, b)
        dw, db = pair or (torch.zeros((3, C, 3, 3), device=x.device, dtype=torch.float32),
                          torch.zeros(3, device=x.device, dtype=torch.float32) if b is not None else None)
        _lib.call("dhz_thin_conv3x3_wgrad_dt", _p(dy), _p(x), _p(dw), _p(db), B, H, W, C, _dt(x), _stream())
        if pair:
            _ready(w, b)
            return dx, None, None, None, None
        return dx, dw, db, None, None


def thin_conv3x3(x, w, b, H, W):
    return _ThinConv.apply(x, w, b, H, W)


# ----------------------------------------------------------------------------- K8: 4x4 / stride-2 down-sampling convolution
def conv4s2_supported(x, H, W, need_grad):
    """Shapes the implicit-GEMM kernels take (csrc/conv_gemm.hip): fp32 tokens, even map, channels multiples of 32; the weight
    gradient additionally wants power-of-two output maps (the training patch sizes 128 / 256)."""
    Cin = x.shape[-1]
    ok = x.is_cuda and x.dtype == torch.float32 and H % 2 == 0 and W % 2 == 0 and Cin % 32 == 0
    if ok and need_grad:
        Ho, Wo = H // 2, W // 2
        ok = (Ho & (Ho - 1)) == 0 and (Wo & (Wo - 1)) == 0 and (x.shape[0] * Ho * Wo) % 32 == 0
    return ok


def _conv4s2_wgrad(w, b, zeros, launch):
    """the weight-gradient tail the fp32 and the bf16 Downsample convolution share: launch(dwp, db) accumulates into the zeroed
    tap-major dwp [Cout, 16 Cin] (from zeros(shape)) and into the bias gradient (b.grad itself when b is a leaf); dwp goes back to
    [co][ci][ky][kx] and is added to w.grad (leaf) or handed to autograd.  Returns the autograd slots (gw, gb)."""
    if not (w.requires_grad or (b is not None and b.requires_grad)):
        return None, None
    Cout, Cin = w.shape[0], w.shape[1]
    dwp = zeros((Cout, 16 * Cin))
    gbuf = _grad_buf(b) if b is not None else None
    dbv = gbuf if gbuf is not None else (torch.zeros_like(b) if b is not None else None)
    launch(dwp, dbv)
    dw = dwp.view(Cout, 4, 4, Cin).permute(0, 3, 1, 2)
    wbuf = _grad_buf(w)
    if wbuf is not None:
        wbuf.add_(dw)
        _ready(w)
    if gbuf is not None:
        _ready(b)
    return None if wbuf is not None else dw.contiguous(), None if gbuf is not None else dbv


# Forward and backward-data on the six-term plane kernels (dhz_conv4s2_fwd6 / _dgrad6, csrc/split6_gemm.hip) instead of the fp32 matrix
# pipe: fp32 storage, SPLIT_BF16 == 6, deterministic mode off (it keeps the fp32 entries, whose tile choice is a function of the shape),
# and a (Cin, Cout) that is listed for the product.  A level is listed only where the new entry beat the fp32 one by more than the spread
# between rounds at the headline shapes (B = 32, 128-pixel patches; DESIGN.md section 7d, profiles/conv4s2_split6.txt), each product on
# its own.  The weight gradient stays on dhz_conv4s2_wgrad.  DHZ_CONV4S2_SPLIT6=0 is the A/B switch.
CONV4S2_SPLIT6 = os.environ.get("DHZ_CONV4S2_SPLIT6", "1") != "0"
CONV4S2_SPLIT6_FWD = {(32, 64), (64, 128), (128, 256)}       # 256 -> 512: 128 tiles of 128 x 64 on 256 CUs, level with the fp32 entry
CONV4S2_SPLIT6_DGRAD = {(32, 64), (64, 128), (128, 256), (256, 512)}


def _conv4s2_split6(Cin, Cout):
    """(forward, backward-data): which products of this fp32 Downsample layer run the six-term entries"""
    if not CONV4S2_SPLIT6 or SPLIT_BF16 != 6 or DETERMINISTIC:
        return False, False
    return (Cin, Cout) in CONV4S2_SPLIT6_FWD, (Cin, Cout) in CONV4S2_SPLIT6_DGRAD


class _Conv4s2(Function):
    """Downsample.conv on the token layout (M1:606-622): x [B, H*W, Cin] -> [B, (H/2)*(W/2), Cout]."""

    @staticmethod
    def forward(ctx, x, w, b, H, W):
        _require_gpu(x, w, b)
        x = x.contiguous()
        B, L, Cin = x.shape
        Cout = w.shape[0]
        assert L == H * W and tuple(w.shape) == (Cout, Cin, 4, 4)
        y = torch.empty((B, L // 4, Cout), device=x.device, dtype=torch.float32)
        fwd6, dgrad6 = _conv4s2_split6(Cin, Cout)
        dgrad6 = dgrad6 and ctx.needs_input_grad[0]
        pf = pb = None
        if fwd6 or dgrad6:                                 # one launch writes the weight planes of both products (the weights change every step)
            pf = torch.empty((3, 16 * Cin * Cout), device=x.device, dtype=torch.int16) if fwd6 else None
            pb = torch.empty((3, 16 * Cin * Cout), device=x.device, dtype=torch.int16) if dgrad6 else None
            _lib.call("dhz_conv4s2_prepack6", _p(w.detach().contiguous()), _p(pf), _p(pb), Cin, Cout, _stream())
        if fwd6:
            _lib.call("dhz_conv4s2_fwd6", _p(x), _p(pf), _p(b), _p(y), B, H, W, Cin, Cout, _stream())
        else:
            wp = w.detach().permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).contiguous()      # [co][(ky, kx, ci)]
            _lib.call("dhz_conv4s2_fwd", _p(x), _p(wp), _p(b), _p(y), B, H, W, Cin, Cout, _stream())
        ctx.save_for_backward(x, w)
        ctx.params, ctx.geom, ctx.planes_t = (w, b), (B, H, W, Cin, Cout), pb
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ = ctx.saved_tensors
        w, b = ctx.params
        B, H, W, Cin, Cout = ctx.geom
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0] and ctx.planes_t is not None:
            dx = torch.empty_like(x)
            _lib.call("dhz_conv4s2_dgrad6", _p(dy), _p(ctx.planes_t), _p(dx), B, H, W, Cin, Cout, _stream())
        elif ctx.needs_input_grad[0]:
            wq = w_.detach().permute(2, 3, 0, 1).contiguous()                         # [(ky, kx, co)][ci]
            dx = torch.empty_like(x)
            _lib.call("dhz_conv4s2_dgrad", _p(dy), _p(wq), _p(dx), B, H, W, Cin, Cout, _stream())
        gw, gb = _conv4s2_wgrad(w, b, lambda shape: zeros_f32(shape, x.device), lambda dwp, dbv: _lib.call(
            "dhz_conv4s2_wgrad", _p(dy), _p(x), _p(dwp), _p(dbv), B, H, W, Cin, Cout, _stream()))
        return dx, gw, gb, None, None


class _Conv4s2BF16(Function):
    """Downsample.conv for bf16 tokens (BASELINE config 4): an explicit tap-major patch matrix (streaming copy in this layout)
    and the three bf16-MFMA token-Linear GEMMs over it (csrc/conv_bf16.hip); fp32 master weights / gradients."""

    @staticmethod
    def forward(ctx, x, w, b, H, W):
        _require_gpu(x, w, b)
        x = x.contiguous()
        B, L, Cin = x.shape
        Cout = w.shape[0]
        assert L == H * W and tuple(w.shape) == (Cout, Cin, 4, 4) and x.dtype == BF16
        wp = w.detach().permute(0, 2, 3, 1).reshape(Cout, 16 * Cin).to(BF16)          # [co][(ky, kx, ci)], one cast per pass
        col = torch.empty((B * (L // 4), 16 * Cin), device=x.device, dtype=BF16)
        _lib.call("dhz_im2col_k4s2_bf16", _p(x), _p(col), B, H, W, Cin, _stream())
        y = gemm_fwd(col, wp, b.detach() if b is not None else None)
        ctx.save_for_backward(col, wp)
        ctx.params, ctx.geom = (w, b), (B, H, W, Cin, Cout)
        return y.view(B, L // 4, Cout)

    @staticmethod
    def backward(ctx, dy):
        col, wp = ctx.saved_tensors
        w, b = ctx.params
        B, H, W, Cin, Cout = ctx.geom
        dy = dy.contiguous().view(-1, Cout)
        dx = None
        if ctx.needs_input_grad[0]:
            dcol = gemm_dgrad(dy, wp)
            dx = torch.empty((B, H * W, Cin), device=dy.device, dtype=BF16)
            _lib.call("dhz_col2im_k4s2_bf16", _p(dcol), _p(dx), B, H, W, Cin, _stream())
        gw, gb = _conv4s2_wgrad(w, b, lambda shape: torch.zeros(shape, device=dy.device, dtype=torch.float32),
                                lambda dwp, dbv: _wgrad_launch(dy, 0, col, [(Cout, dwp, dbv)], None))
        return dx, gw, gb, None, None


def conv4s2_bf16_supported(x, H, W):
    """bf16 tokens, even map, channels in 64s (the bf16 GEMM kernels' tiles), output tokens in 64s."""
    Cin = x.shape[-1]
    return x.is_cuda and x.dtype == BF16 and H % 2 == 0 and W % 2 == 0 and Cin % 64 == 0 and (x.shape[0] * (H // 2) * (W // 2)) % 64 == 0


def conv4s2_tokens(x, w, b, H, W):
    if x.dtype == BF16:
        return _Conv4s2BF16.apply(x, w, b, H, W)
    return _Conv4s2.apply(x, w, b, H, W)


# ----------------------------------------------------------------------------- K9: input projection
class _InputProj(Function):
    """Conv2d(3, E, 3x3, pad 1) + LeakyReLU from the NCHW image into tokens [B, H*W, E] (M1:659-682)."""

    @staticmethod
    def forward(ctx, img, w, b, slope, out_dtype=torch.float32):
        _require_gpu(img, w, b)
        img = img.contiguous()
        B, _, H, W = img.shape
        E = w.shape[0]
        y = torch.empty((B, H * W, E), device=img.device, dtype=out_dtype)
        _lib.call("dhz_input_proj_fwd_dt", _p(img), _p(w.contiguous()), _p(b), _p(y), B, H, W, E, float(slope), _dt(y), _stream())
        ctx.save_for_backward(img, y)
        ctx.params, ctx.slope = (w, b), float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        img, y = ctx.saved_tensors
        w, b = ctx.params
        if ctx.needs_input_grad[0]:
            raise RuntimeError("dehaze_hip: InputProj has no backward-data kernel (the image never needs a gradient on this path)")
        B, _, H, W = img.shape
        E = w.shape[0]
        pair = _grad_pair(w, b)
        gw, gb = pair or (torch.zeros_like(w, memory_format=torch.contiguous_format), torch.zeros_like(b))
        _lib.call("dhz_input_proj_bwd_dt", _p(dy.contiguous().to(y.dtype)), _p(y), _p(img), _p(gw), _p(gb), B, H, W, E, ctx.slope, _dt(y),
                  _stream())
        if pair:
            _ready(w, b)
            return None, None, None, None, None
        return None, gw, gb, None, None


def input_proj(img, w, b, slope=0.01, out_dtype=torch.float32):
    return _InputProj.apply(img, w, b, slope, out_dtype)
