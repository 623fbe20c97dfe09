"""dhz_linear_bwd_pair (csrc/linear_bwd_pair.hip): both entries are declared and exported, and the contract is checked before anything is
launched (safe without a GPU: every call below is refused)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_and_exported():
    from dehaze_hip import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    for name in ("dhz_linear_bwd_pair", "dhz_linear_bwd_pair_grid"):
        assert f"int {name}(" in header
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["dhz_linear_bwd_pair"]) == 15


def test_grid_query_answers_zero_for_refused_shapes():
    from dehaze_hip import _lib
    lib = _lib.load()
    assert lib.dhz_linear_bwd_pair_grid(48, 256, 64) == 0          # T % 32
    assert lib.dhz_linear_bwd_pair_grid(64, 512, 128) == 0         # C = 128: no instance
    assert lib.dhz_linear_bwd_pair_grid(64, 256, 32) == 0
    for N, K in ((128, 32), (256, 64), (192, 64)):
        assert lib.dhz_linear_bwd_pair_grid(32, N, K) == 1         # one stage: one workgroup
        assert lib.dhz_linear_bwd_pair_grid(64, N, K) == 2


def _call(**over):
    from dehaze_hip import _lib
    lib = _lib.load()
    a = dict(dy=64, ldy=256, x=64, ldx=64, hi=64, mid=64, lo=64, dx=64, T=64, nmat=1, nper=256, K=64, dw=[64], db=[64])
    a.update(over)
    arr = lambda v: None if v is None else ctypes.cast((ctypes.c_void_p * len(v))(*v), ctypes.c_void_p)      # noqa: E731
    rc = lib.dhz_linear_bwd_pair(a["dy"], a["ldy"], a["x"], a["ldx"], a["hi"], a["mid"], a["lo"], a["dx"], a["T"], a["nmat"], a["nper"],
                                 a["K"], arr(a["dw"]), arr(a["db"]), None)
    return rc, lib.dhz_last_error()


@pytest.mark.parametrize("over,word", [
    (dict(dy=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(mid=None), b"null pointer"), (dict(dx=None), b"null pointer"),
    (dict(dw=None), b"null pointer"), (dict(dw=[None]), b"null dw[0]"), (dict(nmat=3, nper=64, ldy=192, dw=[64, None, 64]), b"null dw[1]"),
    (dict(T=48), b"T=48"), (dict(T=0), b"T=0"),
    (dict(nper=512, K=128, ldy=512, ldx=128), b"N=512"), (dict(K=32), b"K=32"), (dict(nmat=3, nper=64, K=32, ldy=192), b"N=192"),
    (dict(nmat=5, nper=64), b"nmat=5"),
    (dict(ldy=258), b"ldy=258"), (dict(ldy=128), b"ldy=128"), (dict(ldx=66), b"ldx=66"), (dict(ldx=32), b"ldx=32"),
    (dict(dy=68), b"16-byte aligned"), (dict(lo=72), b"16-byte aligned"), (dict(dx=8), b"16-byte aligned")])
def test_bad_arguments_are_refused_with_a_message(over, word):
    rc, msg = _call(**over)
    assert rc == -22 and word in msg, (rc, msg)


def test_deterministic_mode_is_refused():
    from dehaze_hip import _lib
    lib = _lib.load()
    try:
        assert lib.dhz_set_deterministic(1) == 0
        rc, msg = _call()
        assert rc == -22 and b"deterministic" in msg, (rc, msg)
    finally:
        lib.dhz_set_deterministic(0)
