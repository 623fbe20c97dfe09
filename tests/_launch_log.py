"""Drive the token-Linear wrappers of dehaze_hip.ops / fused WITHOUT a device and log what the library would be asked to do.

`_lib.call` is replaced by a recorder, `ops._require_gpu` by a no-op and `ops._stream` by a constant; the operands are torch.empty CPU
tensors (never touched: nothing is computed).  Per call the log keeps the entry-point name and every argument that is not a pointer
(positions from _lib.SIGNATURES).  tests/test_host.py compares the log of a grid of products, shapes and switches with a table that
was produced by the commit BEFORE the dispatch was rewritten into one route function and one weight-gradient entry."""
import contextlib
import ctypes

import torch

F32, BF16 = torch.float32, torch.bfloat16


@contextlib.contextmanager
def recorder():
    from dehaze_hip import _lib, fused, ops
    log = []

    def call(name, *args):
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), name
        vals = [a for a, t in zip(args, sig) if t is not ctypes.c_void_p]
        assert all(isinstance(v, (int, float)) for v in vals), (name, vals)
        log.append(name.replace("dhz_linear_", "").replace("dhz_", "") + "(" + ",".join(f"{v:g}" if isinstance(v, float) else str(v) for v in vals) + ")")

    saved = (_lib.call, ops._require_gpu, ops._stream, fused._require_gpu, fused._stream)
    _lib.call, ops._require_gpu, ops._stream = call, (lambda *t: None), (lambda: 0)
    fused._require_gpu, fused._stream = ops._require_gpu, ops._stream
    try:
        yield log
    finally:
        _lib.call, ops._require_gpu, ops._stream, fused._require_gpu, fused._stream = saved


@contextlib.contextmanager
def switches(split, res_epilogue, no_tplanes):
    from dehaze_hip import ops
    saved = (ops.SPLIT_BF16, ops.RES_EPILOGUE, ops._NO_TPLANES, ops.BF16_SHADOW, ops.SPLIT_SHADOW, ops.SHADOW_OWNER, ops.GRAD_READY)
    ops.SPLIT_BF16, ops.RES_EPILOGUE, ops._NO_TPLANES = split, res_epilogue, no_tplanes
    ops.set_bf16_shadow(None, None)
    ops.set_split_shadow(None, None)
    ops.SHADOW_OWNER = ops.GRAD_READY = None
    try:
        yield
    finally:
        ops.SPLIT_BF16, ops.RES_EPILOGUE, ops._NO_TPLANES, ops.BF16_SHADOW, ops.SPLIT_SHADOW, ops.SHADOW_OWNER, ops.GRAD_READY = saved


class _StaleOnce:
    """stands in for FlatAdamW as the owner of the derived copies: reports the first region it is asked about as written since the copies
    were derived, so that ONE lookup re-derives them (the refresh launches go through the recorder)"""

    def __init__(self):
        self.stale = True

    def region_current(self, off, n):
        return not self.stale

    def sync_shadows(self, force=False):
        from dehaze_hip import ops
        self.stale = False
        ops.refresh_split_shadow()
        ops.refresh_bf16_shadow()


def weights(N, K, nmat, shadow):
    """nmat (W [N, K], b [N]) fp32 pairs lying back to back in one flat buffer (weights first, then biases: how FlatAdamW packs Q / K / V);
    shadow: the buffer's bf16 copy, split planes and their transposed forms are registered for each matrix and for the packed one."""
    from dehaze_hip import ops
    n = nmat * N * K
    flat = torch.empty(n + nmat * N + 64, dtype=F32)
    Ws = [flat[i * N * K: (i + 1) * N * K].view(N, K) for i in range(nmat)]
    bs = [flat[n + i * N: n + (i + 1) * N] for i in range(nmat)]
    if shadow:
        index = {(i * N * K, N, K) for i in range(nmat)} | {(0, nmat * N, K)}
        desc = torch.empty((len(index), 4), dtype=torch.int32)
        m = flat.numel()
        ops.set_split_shadow(flat, torch.empty((3, m), dtype=BF16), torch.empty((3, m), dtype=BF16), desc, index, 7)
        ops.set_bf16_shadow(flat, torch.empty(m, dtype=BF16), torch.empty(m, dtype=BF16), desc, index, 7)
    return Ws, bs


def rows(T, C, dtype, ld=None):
    """[T, C] with row stride ld (default: contiguous)"""
    return torch.empty((T, ld or C), dtype=dtype)[:, :C]


def products(T, K, N, geom, dtype, shadow, ldx=None, stale=False):
    """every product of the grid for one x [T, K] . W [N, K]^T; geom = (B, Hres, Wres) with B * Hres * Wres == T.
    Returns {product name: "call; call; ..."}."""
    from dehaze_hip import fused, ops
    B, Hres, Wres = geom
    assert B * Hres * Wres == T
    out = {}

    def run(tag, fn):
        with recorder() as log:
            try:
                fn()
            except (RuntimeError, AssertionError) as e:         # a shape outside a kernel's contract is refused, not routed elsewhere
                log.append("raises " + type(e).__name__)
        out[tag] = "; ".join(log)

    (W,), (b,) = weights(N, K, 1, shadow)
    if stale:
        import weakref
        owner = _StaleOnce()
        ops.SHADOW_OWNER = weakref.ref(owner)
    x, dy = rows(T, K, dtype, ldx), rows(T, N, dtype, ldx and ldx - K + N)
    res, sc = torch.empty((T, N), dtype=dtype), torch.empty(B, dtype=F32)
    run("fwd", lambda: ops.gemm_fwd(x, W, b))
    run("res_win_sc", lambda: ops.gemm_fwd_res(x, W, b, res, sc, B, Hres, Wres, min(4, Hres - 1), True))
    run("res_win", lambda: ops.gemm_fwd_res(x, W, b, res, None, B, Hres, Wres, 0, True))
    run("res_tok_sc", lambda: ops.gemm_fwd_res(x, W, b, res, sc, B, Hres * Wres, 1, 0, False))
    run("res_tok", lambda: ops.gemm_fwd_res(x, W, b, res, None, B, Hres * Wres, 1, 0, False))
    run("dgrad", lambda: ops.gemm_dgrad(dy, W))
    run("dgrad_rs", lambda: ops.gemm_dgrad(dy, W, (sc, Hres * Wres)))
    if ldx is not None:
        return out
    for nmat in (1, 3):
        for kind in ("leaf", "frozen", "nonleaf"):
            Ws, bs = weights(N, K, nmat, shadow)
            if kind == "nonleaf":                       # the first weight is the result of an operation: its gradient goes back to autograd
                Ws, bs = [w.requires_grad_() for w in Ws], [v.requires_grad_() for v in bs]
                Ws[0] = Ws[0] * 1
            elif kind == "leaf":
                Ws, bs = [w.requires_grad_() for w in Ws], [v.requires_grad_() for v in bs]
            xa = torch.empty((T, K), dtype=dtype, requires_grad=True)

            def step():
                y = ops.linear_tokens(xa, *[t for pair in zip(Ws, bs) for t in pair])
                y.backward(torch.empty_like(y))
            run(f"lin{nmat}_{kind}", step)
    if dtype == F32:
        for kind in ("leaf", "nonleaf"):
            (W,), (b,) = weights(N, K, 1, shadow)
            W, b = W.requires_grad_(), b.requires_grad_()
            if kind == "nonleaf":
                W = W * 1
            run(f"wgrad_rs_{kind}", lambda: fused._wgrad(dy, 0, x, W, b, (sc, Hres * Wres)))
    return out


def model_shapes(embed_dim, ps, bs):
    """every (T, contraction, out, (B, Hres, Wres)) a token-Linear of the LeFF / ProbSparse model takes: walked from the model's own
    Linear modules (the packed Q / K / V product included)"""
    import My_model_1 as M1
    from dehaze_hip import model as dmodel
    net = M1.Uformer(img_size=ps, embed_dim=embed_dim, win_size=8, token_projection='linear', token_mlp='leff')
    shapes = set()
    for blk in net.modules():
        if isinstance(blk, dmodel.LeWinTransformerBlock):
            Hres, Wres = blk.input_resolution
            geom = (bs, Hres, Wres)
            T = bs * Hres * Wres
            for lin in blk.modules():
                if isinstance(lin, torch.nn.Linear):
                    shapes.add((T, lin.in_features, lin.out_features, geom))
            shapes.add((T, blk.dim, 3 * blk.dim, geom))
    return sorted(shapes)


SETTINGS = [(6, True, False), (0, True, False), (3, True, False), (6, False, False), (6, True, True), (6, False, True)]
# the edges of the ladder: T = 2048 / 2112, out = 64 / 2048 / 2112, contraction 32 / 48 / 64, out % 128 != 0 at T = 2^19, HW % 64 != 0
EDGES = [(2048, 64, 64, (2, 32, 32)), (2112, 64, 64, (33, 8, 8)), (2112, 64, 64, (44, 6, 8)), (2048, 64, 2048, (2, 32, 32)),
         (2112, 64, 2048, (33, 8, 8)), (2048, 64, 2112, (2, 32, 32)), (2112, 2112, 64, (33, 8, 8)), (2048, 2048, 64, (2, 32, 32)),
         (2112, 2048, 64, (33, 8, 8)), (4096, 32, 64, (1, 64, 64)), (4096, 48, 64, (1, 64, 64)), (4096, 64, 48, (1, 64, 64)),
         (4096, 64, 96, (1, 64, 64)), (4096, 96, 96, (1, 64, 64)), (4096, 128, 160, (4, 32, 32)), (1 << 19, 64, 64, (32, 128, 128)),
         (1 << 19, 64, 192, (32, 128, 128)), (1 << 19, 32, 96, (32, 128, 128)), (1 << 19, 64, 128, (32, 128, 128)),
         (1 << 19, 128, 64, (32, 128, 128)), (4000, 64, 64, (1, 40, 100)), (2080, 16, 48, (65, 4, 8))]
STRIDES = [(4096, 64, 128, (1, 64, 64), 66), (4096, 64, 128, (1, 64, 64), 68), (4096, 128, 64, (1, 64, 64), 136), (2048, 64, 64, (2, 32, 32), 70)]


def grid():
    """[(case name, {product: calls})] in a fixed order"""
    out = []

    def case(T, K, N, geom, dtype, shadow, setting, ldx=None, stale=False):
        name = f"T{T} K{K} N{N} {'x'.join(map(str, geom))} {'bf16' if dtype == BF16 else 'f32'} split{setting[0]} res{int(setting[1])} notp{int(setting[2])}" \
               f" shadow{int(shadow)}" + (f" ld{ldx}" if ldx else "") + (" stale" if stale else "")
        with switches(*setting):
            out.append((name, products(T, K, N, geom, dtype, shadow, ldx, stale)))

    S = SETTINGS
    own = [(F32, True, S[0]), (F32, False, S[0]), (F32, True, S[1]), (BF16, True, S[0])]        # the fp32 models: their step, bench.py's fp32_pipe leg
    for args, combos in (((32, 128, 32), own), ((16, 128, 2), own), ((64, 256, 8), [(BF16, True, S[0]), (BF16, False, S[0]), (F32, True, S[0])])):
        for T, K, N, geom in model_shapes(*args):
            for dtype, shadow, setting in combos:
                case(T, K, N, geom, dtype, shadow, setting)
    for T, K, N, geom in EDGES:
        for dtype in (F32, BF16):
            for setting in S:
                for shadow in ((True, False) if setting in (S[0], S[4], S[5]) else (True,)):
                    case(T, K, N, geom, dtype, shadow, setting)
    for T, K, N, geom, ld in STRIDES:
        for dtype in (F32, BF16):
            for setting in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
                case(T, K, N, geom, dtype, True, setting, ldx=ld)
    case(4096, 128, 128, (1, 64, 64), F32, True, SETTINGS[0], stale=True)
    case(4096, 128, 128, (1, 64, 64), BF16, True, SETTINGS[0], stale=True)
    return out
