"""CPU tests of the padding-word entries (the padding mask of any-size evaluation as one uint64 per window): they are declared, exported
and bound, and their argument checks - which run before any launch, so without a GPU - refuse what the kernels do not cover with -22 and a
message that names the argument."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

PAD_ENTRIES = ("dhz_pad_window_bits", "dhz_ps_attn_fwd_dt_pad", "dhz_ps_attn_bwd_dt_pad", "dhz_ps_attn_fwd_w_pad", "dhz_ps_attn_bwd_w_pad",
               "dhz_fused_window_attn_fwd_pad")
P = 0x1000          # any non-null address: the checks under test return before a pointer is used


def _lib():
    from dehaze_hip import _lib
    return _lib


def _err():
    return _lib().load().dhz_last_error().decode()


def test_pad_entries_declared_exported_and_named_by_the_gpu_tests():
    L = _lib()
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    declared = set(re.findall(r"\b(dhz_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_pad_bits.py")).read()
    for name in PAD_ENTRIES:
        assert name in declared, f"{name} is not declared in include/dehaze_hip.h"
        assert hasattr(lib, name) and name in L.SIGNATURES, f"{name} is not exported / bound"
        assert re.search(r"\b%s\b" % name, gpu), f"tests/test_gpu_pad_bits.py does not name {name}"
    # every padding-word entry documents the ATen sequence it replaces
    for name in ("dhz_pad_window_bits", "dhz_ps_attn_fwd_dt_pad", "dhz_fused_window_attn_fwd_pad"):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "window_partition" in comment and "interpolate" in comment, name


def test_pad_window_bits_refusals():
    lib = _lib().load()
    f = lib.dhz_pad_window_bits
    assert f(None, P, 1, 32, 32, 32, 32, 8, None) == EINVAL and "null pointer" in _err() and "mask" in _err()
    assert f(P, None, 1, 32, 32, 32, 32, 8, None) == EINVAL and "bits" in _err()
    for win in (2, 5, 16):
        assert f(P, P, 1, 32, 32, 32, 32, win, None) == EINVAL and "4 or 8" in _err() and "window %d" % win in _err()
    # a block resolution that does not divide the image: nearest resampling at a whole ratio only
    assert f(P, P, 1, 40, 32, 16, 16, 8, None) == EINVAL and "Himg" in _err() and "40" in _err()
    assert f(P, P, 1, 32, 40, 16, 16, 8, None) == EINVAL and "Wimg" in _err()
    assert f(P, P, 1, 32, 32, 64, 64, 8, None) == EINVAL and "Himg" in _err()          # up-sampling is no whole ratio either
    # a map that is no whole number of windows
    assert f(P, P, 1, 24, 24, 12, 12, 8, None) == EINVAL and "win=8" in _err()
    assert f(P, P, 0, 32, 32, 32, 32, 8, None) == EINVAL and "B=0" in _err()


def _fwd_args(pad, B_, nW, win=None, q=P):
    #        q  k  v  ld  idx bias  mask  pad  out ldo rank B_  H  nW  d
    a = [q, P, P, 96, P, None, None, pad, P, 32, P, B_, 1, nW, 32]
    return a + ([win] if win is not None else []) + [0, None]


def _bwd_args(pad, B_, nW, win=None, q=P):
    #        q  k  v  ld  bias  mask  pad  rank dout ldo dq dk dv ldg dpart B_  H  nW  d
    a = [q, P, P, 96, None, None, pad, P, P, 32, P, P, P, 96, None, B_, 1, nW, 32]
    return a + ([win] if win is not None else []) + [0, None]


def test_chain_pad_entries_refuse_null_words_and_partial_images():
    lib = _lib().load()
    for name, args, win in (("dhz_ps_attn_fwd_dt_pad", _fwd_args, None), ("dhz_ps_attn_bwd_dt_pad", _bwd_args, None),
                            ("dhz_ps_attn_fwd_w_pad", _fwd_args, 8), ("dhz_ps_attn_bwd_w_pad", _bwd_args, 8),
                            ("dhz_ps_attn_fwd_w_pad", _fwd_args, 4), ("dhz_ps_attn_bwd_w_pad", _bwd_args, 4)):
        f = getattr(lib, name)
        assert f(*args(None, 8, 4, win)) == EINVAL and "pad is NULL" in _err(), name
        # B_ = 6 windows are no whole number of images of nW = 4 windows; nW = 0 says nothing about the images
        assert f(*args(P, 6, 4, win)) == EINVAL and "B_=6" in _err() and "nW=4" in _err(), name
        assert f(*args(P, 8, 0, win)) == EINVAL and "nW=0" in _err(), name
        # the checks of the entry without padding words still hold
        assert f(*args(P, 8, 4, win, q=None)) == EINVAL and "null pointer" in _err(), name
    for name, args in (("dhz_ps_attn_fwd_w_pad", _fwd_args), ("dhz_ps_attn_bwd_w_pad", _bwd_args)):
        for win in (2, 16):
            assert getattr(lib, name)(*args(P, 8, 4, win)) == EINVAL and "4 or 8" in _err(), name


def test_fused_pad_entry_refusals():
    lib = _lib().load()
    f = lib.dhz_fused_window_attn_fwd_pad
    #             six x  g  b  wqkv bqkv wo bo idx bias mask pad  dscale out B  H   W   C   shift
    base = lambda **k: [k.get("six", 0), k.get("x", P), P, P, P, P, P, P, P, None, k.get("mask"), k.get("pad", P), None, P, 2, 16, 16, k.get("C", 32),
                        k.get("shift", 0), None]
    assert f(*base(pad=None)) == EINVAL and "pad is NULL" in _err()
    assert f(*base(x=None)) == EINVAL and "null pointer" in _err()
    assert f(*base(C=48)) == EINVAL and "C=48" in _err()
    # the shift mask stays tied to a shift; the padding words are valid at any shift (no launch is attempted here: shift 0 with a mask)
    assert f(*base(mask=P, shift=0)) == EINVAL and "shifted windows" in _err()


def test_pad_route_switch_and_tensor_route_on_cpu():
    """DHZ_PAD_BITS is read once into ops.PAD_BITS; CPU tensors keep the tensor route: the staging leaves every block without words"""
    import My_model_1 as M1
    from dehaze_hip import fused, ops
    assert ops.PAD_BITS is (os.environ.get("DHZ_PAD_BITS", "1") != "0")
    model = M1.Uformer(img_size=128, embed_dim=16, win_size=8, token_projection='linear', token_mlp='leff').eval()
    x = torch.zeros(1, 3, 128, 128)
    assert model._stage_pad_bits(x, torch.zeros(1, 1, 128, 128)) is False
    assert all(b._staged_pad is None for st in model.stages() for b in st.blocks)
    assert model._stage_pad_bits(x, None) is False
    # the one predicate of the block dispatch and of the operand staging
    blk = model.encoderlayer_0.blocks[1]
    assert fused.takes_node(blk) and not fused.takes_node(blk, tensor_mask=True)
    assert not fused.takes_node(M1.LeWinTransformerBlock(dim=32, input_resolution=(16, 16), num_heads=1, win_size=4, shift_size=2))


def test_eval_batches_keep_order_and_split_on_size():
    """eval_any_resolution.py: consecutive items of equal image size share a forward of up to --batch_size; restore_any cuts every image of
    a batch back out of its canvas"""
    import eval_any_resolution as EA
    z = lambda h, w: (None, torch.zeros(1, 3, h, w), ["x"])
    items = [z(4, 5), z(4, 5), z(4, 5), z(6, 5), z(4, 5)]
    assert [len(b) for b in EA.batches_of_equal_size(items, 2)] == [2, 1, 1, 1]
    assert [len(b) for b in EA.batches_of_equal_size(items, 1)] == [1] * 5
    assert [len(b) for b in EA.batches_of_equal_size(items, 8)] == [3, 1, 1]
    assert [it for b in EA.batches_of_equal_size(items, 2) for it in b] == items

    class Twice(torch.nn.Module):
        def forward(self, x, m):
            assert x.shape == (2, 3, 128, 128) and m.shape == (2, 1, 128, 128) and float(m.sum()) == 2 * (128 * 128 - 100 * 70)
            return 2 * x
    x = torch.rand(2, 3, 100, 70)
    assert torch.equal(EA.restore_any(Twice(), x, 128), 2 * x)
