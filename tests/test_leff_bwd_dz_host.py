"""dhz_leff_dwconv_bwd_dy (csrc/leff_dwconv_dz.hip): the shape contract is checked before anything is launched (safe without a GPU)."""
import pytest


def _call(**over):
    from dehaze_hip import _lib
    lib = _lib.load()
    a = dict(dy=64, ldy=32, hi=64, mid=64, lo=64, u=64, tpre=64, wd=64, du=64, dw=64, db=64, scale=None, B=1, H=8, W=16, C=32, Ch=128)
    a.update(over)
    rc = lib.dhz_leff_dwconv_bwd_dy(a["dy"], a["ldy"], a["hi"], a["mid"], a["lo"], a["u"], a["tpre"], a["wd"], a["du"], a["dw"], a["db"],
                                    a["scale"], a["B"], a["H"], a["W"], a["C"], a["Ch"], None)
    return rc, lib.dhz_last_error()


@pytest.mark.parametrize("over,word", [(dict(C=48, ldy=48), b"C=48"), (dict(Ch=48), b"Ch=48"), (dict(tpre=None), b"null pointer"),
                                       (dict(mid=None), b"null pointer"), (dict(ldy=30), b"ldy=30")])
def test_bad_arguments_are_refused_with_a_message(over, word):
    rc, msg = _call(**over)
    assert rc == -22 and word in msg, (rc, msg)
