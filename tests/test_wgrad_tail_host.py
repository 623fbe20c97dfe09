"""No GPU: the route of ops.linear_wgrad for a 16-token tail on the launch recorder of tests/_launch_log.py (the aligned shapes are
pinned by tests/test_host.py's grid), and the library's argument checks."""
import torch

import _launch_log as L


def _wgrad_log(T, K, N, dtype):
    from dehaze_hip import ops
    (W,), (b,) = L.weights(N, K, 1, False)
    W, b = W.requires_grad_(), b.requires_grad_()
    dy, x = L.rows(T, N, dtype), L.rows(T, K, dtype)
    with L.switches(*L.SETTINGS[0]), L.recorder() as log:
        try:
            ops.linear_wgrad(dy, 0, x, [(W, b)])
        except (RuntimeError, AssertionError) as e:
            log.append("raises " + type(e).__name__)
    return log


def test_fp32_tail_is_one_wgrad_launch():
    assert _wgrad_log(48, 32, 32, L.F32) == ["wgrad(32,32,48,32,32)"]
    assert _wgrad_log(16, 512, 2048, L.F32) == ["wgrad(2048,512,16,2048,512)"]          # batch 1 at the bottleneck of embed_dim 32
    assert _wgrad_log(64, 32, 32, L.F32) == ["wgrad(32,32,64,32,32)"]                   # (an aligned T: as before)


def test_fp32_tail_of_packed_qkv_is_one_multi_launch():
    from dehaze_hip import ops
    Ws, bs = L.weights(64, 64, 3, False)
    params = [(w.requires_grad_(), b.requires_grad_()) for w, b in zip(Ws, bs)]
    with L.switches(*L.SETTINGS[0]), L.recorder() as log:
        ops.linear_wgrad(L.rows(48, 192, L.F32), 0, L.rows(48, 64, L.F32), params)
    assert log == ["wgrad_multi(192,64,48,3,64,64)"]


def test_bf16_tail_still_raises():
    assert _wgrad_log(48, 64, 64, L.BF16) == ["raises RuntimeError"]
    assert _wgrad_log(48, 32, 32, L.BF16) == ["raises RuntimeError"]


def test_fp32_ragged_token_count_still_raises():
    assert _wgrad_log(40, 32, 32, L.F32) == ["raises RuntimeError"]
    assert _wgrad_log(8, 32, 32, L.F32) == ["raises RuntimeError"]


def test_library_refuses_what_is_no_multiple_of_16():
    """before any launch (safe without a GPU); the text names the new quantum"""
    from dehaze_hip import _lib
    lib = _lib.load()
    for T in (100, 8, 0):
        assert lib.dhz_linear_wgrad(8, 32, 8, 32, T, 32, 32, 8, None, None) == -22
        assert b"multiple of 16" in lib.dhz_last_error()
    assert lib.dhz_linear_wgrad_rs(8, 32, 8, 32, 64, 32, 32, 8, None, 8, 16, None) == -22
    assert b"rows_per_scale=16" in lib.dhz_last_error()
