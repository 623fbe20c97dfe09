"""Drive the window-side wrappers of dehaze_hip.ops / fused WITHOUT a device and log what the library would be asked to do, in the manner
of tests/_launch_log.py (whose recorder this uses): `_lib.call` is a recorder, the operands are torch.empty CPU tensors, nothing is
computed.  The host-side part-count queries, which the wrappers reach through `_lib.load()`, are recorded too and answer 3 H (a value no
other argument of the grid takes), so that the log does not depend on the CU count of the machine.  tests/test_window_calls_host.py
compares the log of the grid below with the one the commit BEFORE the `win == 8` branches were removed wrote."""
import contextlib

import torch

import _launch_log

F32, BF16 = torch.float32, torch.bfloat16
NTOP = {64: 25, 16: 15}


class _Queries:
    """stands in for the loaded library: only the part-count queries are asked for"""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        assert name.startswith("dhz_ps_attn_bwd_parts"), name

        def query(*args):
            self._log.append(name.replace("dhz_", "") + "(" + ",".join(str(a) for a in args) + ")")
            return 3 * args[1]
        return query


@contextlib.contextmanager
def recorder():
    """_launch_log.recorder plus the queries; CPU tensors pass for device tensors where a wrapper asserts it (the padding words)"""
    from dehaze_hip import _lib
    with _launch_log.recorder() as log:
        saved = _lib.load
        _lib.load = lambda: _Queries(log)
        torch.Tensor.is_cuda = property(lambda self: True)          # shadows the base class's attribute; removed below
        try:
            yield log
        finally:
            del torch.Tensor.is_cuda
            _lib.load = saved


def _run(out, tag, fn):
    with recorder() as log:
        fn()
    out.append(f"{tag} | " + "; ".join(log))


def _back(y):
    y.backward(torch.empty_like(y))


def grid(wins=(8, 4)):
    """["case | call; call; ..."] in a fixed order.  The sizes of one case are pairwise different (B_ = 8 windows, H = 2 heads, nW = 4,
    d = 32 or 16; maps of 2 x 3 windows) so that a permuted argument list changes the line."""
    from dehaze_hip import fused, ops
    out = []
    for win in wins:
        N = win * win
        Hres, Wres, B = 2 * win, 3 * win, 2
        L = Hres * Wres
        for dtype, dn in ((F32, "f32"), (BF16, "bf16")):
            for shift in (0, win // 2):
                for C in (32, 48):
                    tag = f"win{win} {dn} shift{shift} C{C}"
                    x = torch.empty((B, L, C), dtype=dtype, requires_grad=True)
                    gamma, beta = (torch.empty(C, requires_grad=True) for _ in range(2))
                    _run(out, "ln_partition " + tag, lambda: _back(ops.ln_partition(x, gamma, beta, Hres, Wres, shift, win)))
                    yw = torch.empty((B * L, C), dtype=dtype, requires_grad=True)
                    sc = torch.empty(B)
                    _run(out, "reverse_residual " + tag, lambda: _back(ops.reverse_residual(yw, x, sc, Hres, Wres, shift, win)))
            if win == 8:                                            # the token-order forms pass the window side 8 whatever the model's
                x = torch.empty((B, L, 32), dtype=dtype, requires_grad=True)
                gamma, beta = (torch.empty(32, requires_grad=True) for _ in range(2))
                _run(out, f"layer_norm_tokens {dn}", lambda: _back(ops.layer_norm_tokens(x, gamma, beta)))
                y = torch.empty((B, L, 32), dtype=dtype, requires_grad=True)
                _run(out, f"residual_scale {dn}", lambda: _back(ops.residual_scale(y, x, torch.empty(B))))
        _run(out, f"shift_mask win{win}", lambda: ops.shift_mask(Hres, Wres, win // 2, torch.device("cpu"), win))
        B_, nW = 8, 4
        idx = torch.empty((N, NTOP[N]), dtype=torch.uint8)
        for H, d in ((2, 32), (1, 16)):
            C = H * d
            tsize = ((2 * win - 1) ** 2, H)
            _run(out, f"bias_tile win{win} H{H}", lambda: ops.bias_tile(torch.empty(tsize), H, N))
            _run(out, f"bias_table_grad win{win} H{H}", lambda: ops.bias_table_grad(torch.empty((5 * H, N, N)), 5 * H, H, N))
            for has_mask in (False, True):
                mask = torch.empty((nW, N, N)) if has_mask else None
                for has_table in (False, True):
                    tail = f"win{win} H{H} d{d} mask{int(has_mask)} table{int(has_table)}"
                    for dtype, dn in ((F32, "f32"), (BF16, "bf16")):
                        for has_pad in (False, True):
                            pad = torch.empty(B_, dtype=torch.int64) if has_pad else None
                            for nw_arg in ((None, 2) if has_pad and not has_mask else (None,)):
                                qkv = torch.empty((B_ * N, 3 * C), dtype=dtype, requires_grad=True)
                                table = torch.empty(tsize, requires_grad=True) if has_table else None
                                _run(out, f"ps_window_attention {tail} {dn} pad{int(has_pad)} nW{nw_arg}",
                                     lambda: _back(ops.ps_window_attention(qkv, table, idx, mask, H, d, pad, nw_arg)))
                    qkv = torch.empty((B_ * N, 3 * C))
                    table = torch.empty(tsize) if has_table else None
                    _run(out, f"ps_window_attention_rank {tail}", lambda: ops.ps_window_attention_rank(qkv, table, idx, mask, H, d))
                qkv = torch.empty((B_ * N, 3 * C), requires_grad=True)
                table = torch.empty(tsize, requires_grad=True)
                _run(out, f"dense_window_attention win{win} H{H} d{d} mask{int(has_mask)}",
                     lambda: _back(ops.dense_window_attention(qkv, table, mask, H, d, d ** -0.5, N)))
        if win == 8:                                                # the autograd node of the 8 x 8 blocks keeps its own two helpers
            H = 2
            dev = torch.device("cpu")
            _run(out, "fused._bias_tile", lambda: fused._bias_tile(torch.empty((225, H)), H, dev))
            dpart = torch.empty((3 * H, 64, 64))
            leaf = torch.empty((225, H), requires_grad=True)
            _run(out, "fused._table_backward leaf", lambda: fused._table_backward(dpart, 3 * H, leaf, H))
            _run(out, "fused._table_backward nonleaf", lambda: fused._table_backward(dpart, 3 * H, leaf * 1, H))
            for has_table in (False, True):                         # the chain backward of the node: part count, core, table gradient
                _run(out, f"fused._attn_bwd table{int(has_table)}", lambda: fused._attn_bwd(_chain_record(has_table), torch.empty((1, 384, 64))))
    return out


def _chain_record(has_table, B=1, Hres=16, Wres=24, C=64, H=2):
    """what fused._attn_chain_fwd leaves for the backward of a 16 x 24 map at C = 64 (frozen projections: only the window side is logged)"""
    from dehaze_hip import fused
    T = B * Hres * Wres
    e = torch.empty
    ws = [e((C, C)) for _ in range(4)]
    bs = [e(C) for _ in range(4)]
    table = e((225, H), requires_grad=True) if has_table else None
    bias = e((H, 64, 64)) if has_table else None
    saved = (e((B, T // B, C)), e(C), e((T, 2)), e((T, C)), e((T, 3 * C)), e((T, C)), e((T // 64) * H * 64, dtype=torch.uint8), bias, None,
             None, ws[0], ws[1], ws[2], ws[3])
    params = (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], e(C), e(C), table)
    return fused._Rec("attn_chain_bwd", saved, params, (B, Hres, Wres, C, 0, H))
