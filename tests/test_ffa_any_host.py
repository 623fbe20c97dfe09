"""No GPU: the `_any` entries of csrc/ffa_attn.hip and csrc/conv3x3_wgrad.hip (maps of any size) are declared in the header, exported and
bound; their argument checks answer DHZ_EINVAL with a message naming the entry before any launch; the workspace queries are the
documented formulas on ragged shapes and equal the old queries on regular ones, which still refuse what they refused;
dehaze_hip.ffa.blocked_shape_ok; FFA_test.py's options."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFA_ANY = ("dhz_ffa_workspace_bytes_any", "dhz_ffa_ca_fwd_any", "dhz_ffa_gate_pa_fwd_any", "dhz_ffa_gate_pa_bwd_a_any", "dhz_ffa_ca_bwd_any",
           "dhz_ffa_gate_pa_bwd_b_any", "dhz_ffa_add_any")
WGRAD_ANY = ("dhz_conv3x3_wgrad_any", "dhz_conv3x3_wgrad_workspace_bytes_any", "dhz_conv3x3_wgrad_parts_any")
EINVAL = -22
FAKE = 4096          # a non-null, 16-byte aligned "device pointer": every check below fails before anything would touch it
ODD = 4100           # the same, not 16-byte aligned


def test_entries_declared_exported_bound():
    from dehaze_hip import _lib
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = _lib.load()
    for name in FFA_ANY + WGRAD_ANY:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dehaze_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-4]]               # the argument list of the entry without `_any`
        assert getattr(lib, name).restype == getattr(lib, name[:-4]).restype
    assert lib.dhz_abi_version() == 1


def ca_fwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=17, W=19, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes_any(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_ca_fwd_any(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, FAKE, out, ws, ws_bytes, B, H, W, G, None)


def gate_fwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=17, W=19, G=1):
    return lib.dhz_ffa_gate_pa_fwd_any(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, None, out, B, H, W, G, None)


def bwd_a(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=17, W=19, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes_any(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_gate_pa_bwd_a_any(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, FAKE, out, ws, ws_bytes, B, H, W, G, None)


def ca_bwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=17, W=19, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes_any(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_ca_bwd_any(ws, ws_bytes, Wa, FAKE, FAKE, FAKE, FAKE, out, *([FAKE] * 8), B, H, W, G, None)


def bwd_b(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=17, W=19, G=1):
    return lib.dhz_ffa_gate_pa_bwd_b_any(Wa, FAKE, out, m0, m1, m2, B, H, W, G, None)


ENTRIES = {"dhz_ffa_ca_fwd_any": ca_fwd, "dhz_ffa_gate_pa_fwd_any": gate_fwd, "dhz_ffa_gate_pa_bwd_a_any": bwd_a, "dhz_ffa_ca_bwd_any": ca_bwd,
           "dhz_ffa_gate_pa_bwd_b_any": bwd_b}
COMMON = [(dict(B=0), "B=0"), (dict(H=0), "H=0"), (dict(W=0), "W=0"), (dict(H=-16), "H=-16"), (dict(G=2), "G=2"), (dict(G=0), "G=0"),
          (dict(H=8192, W=4096), "too large"), (dict(Wa=None), "null"), (dict(out=None), "null")]
MAPS = [(dict(m0=None), "null"), (dict(G=3, m2=None), "null"), (dict(m0=ODD), "aligned"), (dict(G=3, m1=ODD), "aligned")]
WS = [(dict(ws=None), "workspace"), (dict(ws_bytes=64), "workspace"), (dict(ws=ODD), "aligned")]
CASES = [(e, kw, word) for e in ENTRIES for kw, word in COMMON]
CASES += [(e, kw, word) for e in ENTRIES if e != "dhz_ffa_ca_bwd_any" for kw, word in MAPS]
CASES += [(e, kw, word) for e in ("dhz_ffa_ca_fwd_any", "dhz_ffa_gate_pa_bwd_a_any", "dhz_ffa_ca_bwd_any") for kw, word in WS]
CASES += [("dhz_ffa_gate_pa_fwd_any", dict(out=ODD), "aligned"), ("dhz_ffa_gate_pa_bwd_a_any", dict(out=ODD), "aligned"),
          ("dhz_ffa_gate_pa_bwd_b_any", dict(Wa=ODD), "aligned")]


@pytest.mark.parametrize("entry,kw,word", CASES, ids=[f"{e[8:]}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for e, kw, _ in CASES])
def test_any_attention_entries_refuse_with_a_message(entry, kw, word):
    from dehaze_hip import _lib
    lib = _lib.load()
    assert lib.dhz_get_deterministic() == 0
    assert ENTRIES[entry](lib, **kw) == EINVAL
    msg = lib.dhz_last_error().decode()
    assert entry in msg and word in msg, msg
    if word == "workspace" and "ws" in kw:
        assert "dhz_ffa_workspace_bytes_any" in msg, msg


def wgrad(lib, x=FAKE, dy=FAKE, dw=FAKE, ws=FAKE, ws_bytes=None, B=2, H=18, W=20, Cin=32, Kout=64):
    if ws_bytes is None:
        ws_bytes = lib.dhz_conv3x3_wgrad_workspace_bytes_any(B, H, W, Cin, Kout) or 1 << 20
    return lib.dhz_conv3x3_wgrad_any(x, dy, dw, FAKE, ws, ws_bytes, B, H, W, Cin, Kout, None)


@pytest.mark.parametrize("kw,word", [(dict(B=0), "B=0"), (dict(H=0), "H=0"), (dict(W=-3), "W=-3"), (dict(Cin=48), "Cin=48"),
                                     (dict(Kout=16), "Kout=16"), (dict(Cin=544), "Cin=544"), (dict(x=None), "null"), (dict(dy=None), "null"),
                                     (dict(dw=None), "null"), (dict(ws=None), "workspace"), (dict(ws_bytes=64), "workspace"),
                                     (dict(B=1 << 20, H=38, W=52), "B=1048576")],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_wgrad_any_refuses_with_a_message(kw, word):
    from dehaze_hip import _lib
    lib = _lib.load()
    assert lib.dhz_get_deterministic() == 0
    assert wgrad(lib, **kw) == EINVAL
    msg = lib.dhz_last_error().decode()
    assert "dhz_conv3x3_wgrad_any" in msg and word in msg, msg


def test_add_any_refuses_with_a_message():
    from dehaze_hip import _lib
    lib = _lib.load()
    for args, word in [((None, FAKE, FAKE, 62), "null"), ((FAKE, None, FAKE, 62), "null"), ((FAKE, FAKE, None, 62), "null"),
                       ((FAKE, FAKE, FAKE, 0), "n=0"), ((FAKE, FAKE, FAKE, -2), "n=-2"), ((FAKE, ODD, FAKE, 62), "aligned")]:
        assert lib.dhz_ffa_add_any(*args, None) == EINVAL
        msg = lib.dhz_last_error().decode()
        assert "dhz_ffa_add_any" in msg and word in msg, msg
    assert lib.dhz_ffa_add(FAKE, FAKE, FAKE, 62, None) == EINVAL        # the old entry's refusal of n % 4 != 0 stands


def test_deterministic_mode_names_the_bytes_it_needs():
    from dehaze_hip import _lib
    lib = _lib.load()
    try:
        _lib.call("dhz_set_deterministic", 1)
        _lib.call("dhz_set_det_workspace", None, 0)
        assert bwd_a(lib) == EINVAL                          # its own workspace is not a way round the mode's
        assert str(lib.dhz_ffa_workspace_bytes_any(2, 17, 19, 1)) in lib.dhz_last_error().decode()
        assert wgrad(lib) == EINVAL
        assert str(lib.dhz_conv3x3_wgrad_workspace_bytes_any(2, 18, 20, 32, 64)) in lib.dhz_last_error().decode()
    finally:
        _lib.call("dhz_set_deterministic", 0)


def test_ffa_workspace_query_is_the_documented_formula():
    from dehaze_hip import _lib
    lib = _lib.load()
    ragged = [(1, 5, 7, 1), (2, 17, 19, 3), (3, 33, 16, 1), (2, 42, 52, 3), (1, 460, 620, 1), (4, 250, 250, 3), (1, 1, 1, 1)]
    regular = [(1, 16, 16, 1), (2, 16, 32, 3), (2, 48, 80, 3), (2, 240, 240, 1)]
    base = [lib.dhz_ffa_workspace_bytes_any(*s) for s in ragged + regular]
    for nbytes, (B, H, W, G) in zip(base, ragged + regular):
        chunks = (H * W + 127) // 128                        # backward-a workgroups, their groups of 16, one record per image
        n, hc = 64 * G, 8 if G == 1 else 4
        bwd = B * ((chunks + (chunks + 15) // 16) * (n + 532) + 2 * n * hc + n + hc + 532)
        fwd = B * G * ((H * W + 1023) // 1024) * 64          # pooling partials
        assert nbytes == 4 * max(bwd, fwd), (B, H, W, G)
    for s in regular:
        assert lib.dhz_ffa_workspace_bytes_any(*s) == lib.dhz_ffa_workspace_bytes(*s) > 0
    for s in ragged:
        assert lib.dhz_ffa_workspace_bytes(*s) == 0          # the old query still refuses them
    try:
        _lib.call("dhz_set_reserved_cus", 100)
        _lib.call("dhz_set_deterministic", 1)
        assert [lib.dhz_ffa_workspace_bytes_any(*s) for s in ragged + regular] == base
    finally:
        _lib.call("dhz_set_deterministic", 0)
        _lib.call("dhz_set_reserved_cus", 0)
    for bad in [(0, 16, 16, 1), (2, 0, 16, 1), (2, 16, -1, 1), (2, 17, 19, 2), (1, 8192, 4096, 1)]:
        assert lib.dhz_ffa_workspace_bytes_any(*bad) == 0
    for bad in [(0, 16, 16, 1), (2, 24, 16, 1), (2, 16, 40, 1), (2, 16, 16, 2)]:
        assert lib.dhz_ffa_workspace_bytes(*bad) == 0


def test_wgrad_queries_are_the_documented_formulas():
    from dehaze_hip import _lib
    lib = _lib.load()
    ragged = [(1, 5, 7, 32, 32), (2, 18, 20, 32, 64), (1, 16, 24, 32, 32), (1, 22, 32, 32, 32), (3, 38, 52, 64, 64), (2, 12, 12, 32, 32),
              (1, 460, 620, 64, 64), (4, 250, 250, 64, 64)]
    for B, H, W, Cin, Kout in ragged:
        chunks = B * ((H + 3) // 4) * ((W + 15) // 16)
        tiles = (Kout // 32) * (Cin // 32)
        slabs = min((512 + tiles - 1) // tiles, max(chunks // 4, 1))
        assert lib.dhz_conv3x3_wgrad_parts_any(B, H, W, Cin, Kout) == slabs, (B, H, W)
        assert lib.dhz_conv3x3_wgrad_workspace_bytes_any(B, H, W, Cin, Kout) == slabs * (Kout * Cin * 9 + Kout) * 4
        assert lib.dhz_conv3x3_wgrad_parts(B, H, W, Cin, Kout) == 0 and lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout) == 0
    for s in [(2, 16, 32, 32, 64), (3, 8, 8, 64, 32), (4, 32, 32, 32, 32), (10, 16, 16, 64, 64), (2, 8, 8, 512, 32)]:
        assert lib.dhz_conv3x3_wgrad_parts_any(*s) == lib.dhz_conv3x3_wgrad_parts(*s) > 0
        assert lib.dhz_conv3x3_wgrad_workspace_bytes_any(*s) == lib.dhz_conv3x3_wgrad_workspace_bytes(*s) > 0
    for bad in [(0, 18, 20, 32, 32), (2, 0, 20, 32, 32), (2, 18, 20, 48, 32), (2, 18, 20, 32, 16), (2, 18, 20, 32, 544), (1 << 20, 38, 52, 32, 32)]:
        assert lib.dhz_conv3x3_wgrad_parts_any(*bad) == 0 and lib.dhz_conv3x3_wgrad_workspace_bytes_any(*bad) == 0
    assert lib.dhz_conv3x3_wgrad_parts(2, 12, 12, 32, 32) == 0          # the old entry's refusal of H = 12 stands


def test_blocked_shape_ok_truth_table(monkeypatch):
    from dehaze_hip import ffa
    assert ffa.ANY                                           # the default
    table = {(16, 16): True, (32, 48): True, (240, 240): True, (16, 32): True, (0, 16): False, (8, 8): False,
             (24, 40): False, (31, 52): False, (52, 31): False, (16, 40): False, (24, 24): False,
             (32, 33): True, (38, 52): True, (33, 32): True, (460, 620): True, (413, 550): True, (250, 250): True, (32, 40): True}
    for (H, W), want in table.items():
        assert ffa.blocked_shape_ok(H, W) is want, (H, W)
    monkeypatch.setattr(ffa, "ANY", False)                   # DHZ_FFA_ANY=0
    for (H, W), want in table.items():
        assert ffa.blocked_shape_ok(H, W) is (want and H % 16 == 0 and W % 16 == 0), (H, W)
    assert "32" in ffa.blocked_shape_ok.__doc__ and "LossNetwork" in ffa.blocked_shape_ok.__doc__


def test_ffa_test_parser_defaults():
    import FFA_test
    a = FFA_test.resolve(FFA_test.build_parser().parse_args([]))
    assert (a.task, a.test_imgs, a.gps, a.blocks) == ("its", "test_imgs", 3, 19)
    assert a.weights == os.path.join("trained_models", "its_train_ffa_3_19.pk") and a.out_dir == "pred_FFA_its/"
    assert a.gt_dir == "" and a.normalize is False and a.synthetic == 0
    b = FFA_test.resolve(FFA_test.build_parser().parse_args(["--task", "ots", "--blocks", "2", "--weights", "x.pk", "--out_dir", "o", "--normalize",
                                                             "--synthetic", "3", "--height", "46", "--width", "62", "--gt_dir", "g"]))
    assert (b.task, b.blocks, b.weights, b.out_dir, b.normalize, b.synthetic, b.height, b.width, b.gt_dir) == \
        ("ots", 2, "x.pk", "o", True, 3, 46, 62, "g")
    assert FFA_test.resolve(FFA_test.build_parser().parse_args(["--task", "ots"])).out_dir == "pred_FFA_ots/"
    assert FFA_test.MEAN == (0.64, 0.6, 0.58) and FFA_test.STD == (0.14, 0.15, 0.152)


def test_ffa_test_lists_images_and_pairs_clear_images(tmp_path):
    import FFA_test
    assert all(FFA_test.is_image(n) for n in ("1400_1.png", "a.JPG", "b.jpeg", "c.bmp"))
    assert not any(FFA_test.is_image(n) for n in ("notes.txt", "png", "x.pk", "d.png.bak"))
    for n in ("1400.png", "1401.jpg", "1401_3.png", "readme.txt"):
        (tmp_path / n).write_bytes(b"")
    index = FFA_test.gt_index(str(tmp_path))
    assert sorted(index) == ["1400", "1401", "1401_3"]
    assert FFA_test.find_gt(index, "1400_1.png").endswith("1400.png")        # the SOTS convention
    assert FFA_test.find_gt(index, "1401_3.jpg").endswith("1401_3.png")      # the exact stem wins over the prefix
    assert FFA_test.find_gt(index, "1401_2.jpg").endswith("1401.jpg")
    with pytest.raises(SystemExit, match="1500_1.png"):
        FFA_test.find_gt(index, "1500_1.png", str(tmp_path))
