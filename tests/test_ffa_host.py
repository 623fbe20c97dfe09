"""No GPU: the FFA-Net attention entries (csrc/ffa_attn.hip) are declared in the header, exported by the library and bound in
_lib.SIGNATURES; their argument checks answer DHZ_EINVAL with a message naming the entry before any launch; the workspace query is a
function of the shapes alone; the FFA module's keys, shapes, init statistics and CPU forward equal the reference fixture
tests/golden/ffa_blocks2.npz; utils.get_arch builds it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhz_ffa_workspace_bytes", "dhz_ffa_ca_fwd", "dhz_ffa_gate_pa_fwd", "dhz_ffa_gate_pa_bwd_a", "dhz_ffa_ca_bwd",
       "dhz_ffa_gate_pa_bwd_b", "dhz_ffa_add", "dhz_ffa_relu_bwd_add")
EINVAL = -22
FAKE = 4096          # a non-null, 16-byte aligned "device pointer": every check below fails before anything would touch it
ODD = 4100           # the same, not 16-byte aligned


def test_entries_declared_exported_bound():
    from dehaze_hip import _lib
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dehaze_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert "FFA:105-108" in header and "FFA:54-56" in header


def ca_fwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=32, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_ca_fwd(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, FAKE, out, ws, ws_bytes, B, H, W, G, None)


def gate_fwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=32, G=1):
    return lib.dhz_ffa_gate_pa_fwd(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, None, out, B, H, W, G, None)


def bwd_a(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=32, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_gate_pa_bwd_a(m0, m1, m2, Wa, FAKE, FAKE, FAKE, FAKE, FAKE, out, ws, ws_bytes, B, H, W, G, None)


def ca_bwd(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=32, G=1):
    if ws_bytes is None:
        ws_bytes = lib.dhz_ffa_workspace_bytes(B, H, W, G) or 1 << 20
    return lib.dhz_ffa_ca_bwd(ws, ws_bytes, Wa, FAKE, FAKE, FAKE, FAKE, out, *([FAKE] * 8), B, H, W, G, None)


def bwd_b(lib, m0=FAKE, m1=FAKE, m2=FAKE, Wa=FAKE, out=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=32, G=1):
    return lib.dhz_ffa_gate_pa_bwd_b(Wa, FAKE, out, m0, m1, m2, B, H, W, G, None)


ENTRIES = {"dhz_ffa_ca_fwd": ca_fwd, "dhz_ffa_gate_pa_fwd": gate_fwd, "dhz_ffa_gate_pa_bwd_a": bwd_a, "dhz_ffa_ca_bwd": ca_bwd,
           "dhz_ffa_gate_pa_bwd_b": bwd_b}
COMMON = [(dict(B=0), "B=0"), (dict(H=24), "H=24"), (dict(W=40), "W=40"), (dict(H=0), "H=0"), (dict(G=2), "G=2"), (dict(G=0), "G=0"),
          (dict(Wa=None), "null"), (dict(out=None), "null")]
MAPS = [(dict(m0=None), "null"), (dict(G=3, m2=None), "null"), (dict(m0=ODD), "aligned"), (dict(G=3, m1=ODD), "aligned")]
WS = [(dict(ws=None), "workspace"), (dict(ws_bytes=64), "workspace"), (dict(ws=ODD), "aligned")]
CASES = [(e, kw, word) for e in ENTRIES for kw, word in COMMON]
CASES += [(e, kw, word) for e in ENTRIES if e != "dhz_ffa_ca_bwd" for kw, word in MAPS]
CASES += [(e, kw, word) for e in ("dhz_ffa_ca_fwd", "dhz_ffa_gate_pa_bwd_a", "dhz_ffa_ca_bwd") for kw, word in WS]
CASES += [("dhz_ffa_gate_pa_fwd", dict(out=ODD), "aligned"), ("dhz_ffa_gate_pa_bwd_a", dict(out=ODD), "aligned"),
          ("dhz_ffa_gate_pa_bwd_b", dict(Wa=ODD), "aligned")]


@pytest.mark.parametrize("entry,kw,word", CASES, ids=[f"{e[8:]}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for e, kw, _ in CASES])
def test_attention_entries_refuse_with_a_message(entry, kw, word):
    from dehaze_hip import _lib
    lib = _lib.load()
    assert lib.dhz_get_deterministic() == 0
    assert ENTRIES[entry](lib, **kw) == EINVAL
    msg = lib.dhz_last_error().decode()
    assert entry in msg and word in msg, msg


def test_elementwise_entries_refuse_with_a_message():
    from dehaze_hip import _lib
    lib = _lib.load()
    for args, word in [((None, FAKE, FAKE, 64), "null"), ((FAKE, None, FAKE, 64), "null"), ((FAKE, FAKE, None, 64), "null"),
                       ((FAKE, FAKE, FAKE, 0), "n=0"), ((FAKE, FAKE, FAKE, 62), "n=62"), ((FAKE, ODD, FAKE, 64), "aligned")]:
        assert lib.dhz_ffa_add(*args, None) == EINVAL
        msg = lib.dhz_last_error().decode()
        assert "dhz_ffa_add" in msg and word in msg, msg
    for args, word in [((None, FAKE, FAKE, FAKE, FAKE, 64), "null"), ((FAKE, FAKE, FAKE, FAKE, None, 64), "null"),
                       ((FAKE, FAKE, FAKE, FAKE, FAKE, -4), "n=-4"), ((FAKE, FAKE, FAKE, FAKE, FAKE, 6), "n=6"),
                       ((FAKE, FAKE, FAKE, ODD, FAKE, 64), "aligned")]:
        assert lib.dhz_ffa_relu_bwd_add(*args, None) == EINVAL
        msg = lib.dhz_last_error().decode()
        assert "dhz_ffa_relu_bwd_add" in msg and word in msg, msg


def test_deterministic_mode_names_the_bytes_it_needs():
    from dehaze_hip import _lib
    lib = _lib.load()
    try:
        _lib.call("dhz_set_deterministic", 1)
        _lib.call("dhz_set_det_workspace", None, 0)
        assert bwd_a(lib) == EINVAL                          # its own workspace is not a way round the mode's
        assert str(lib.dhz_ffa_workspace_bytes(2, 16, 32, 1)) in lib.dhz_last_error().decode()
    finally:
        _lib.call("dhz_set_deterministic", 0)


def test_workspace_query_depends_on_the_shapes_alone():
    from dehaze_hip import _lib
    lib = _lib.load()
    shapes = [(1, 16, 16, 1), (2, 16, 32, 3), (3, 32, 16, 1), (2, 48, 80, 3), (2, 240, 240, 1), (8, 128, 128, 3)]
    base = [lib.dhz_ffa_workspace_bytes(*s) for s in shapes]
    for nbytes, (B, H, W, G) in zip(base, shapes):
        chunks = H * W // 128                                # backward-a workgroups, their groups of 16, one record per image
        n, hc = 64 * G, 8 if G == 1 else 4
        assert nbytes == 4 * B * ((chunks + (chunks + 15) // 16) * (n + 532) + 2 * n * hc + n + hc + 532)
    try:
        _lib.call("dhz_set_reserved_cus", 100)
        _lib.call("dhz_set_deterministic", 1)
        assert [lib.dhz_ffa_workspace_bytes(*s) for s in shapes] == base
    finally:
        _lib.call("dhz_set_deterministic", 0)
        _lib.call("dhz_set_reserved_cus", 0)
    for bad in [(0, 16, 16, 1), (2, 24, 16, 1), (2, 16, 40, 1), (2, 16, 16, 2)]:
        assert lib.dhz_ffa_workspace_bytes(*bad) == 0


# ---- the module: surface and CPU path against the reference fixture (tests/golden/gen_golden_ffa.py)
GOLD = os.path.join(ROOT, "tests", "golden", "ffa_blocks2.npz")
MODEL_SEED = 41
GATE_SCALE = 4.0


def seeded_ffa(scaled=True, blocks=2):
    import random
    import numpy as np
    import torch
    from dehaze_hip.ffa import FFA
    random.seed(MODEL_SEED)
    np.random.seed(MODEL_SEED)
    torch.manual_seed(MODEL_SEED)
    net = FFA(gps=3, blocks=blocks)
    if scaled:                                               # as the generator's scale_gates
        with torch.no_grad():
            for n, p in net.named_parameters():
                if {"ca", "pa"} & set(n.split(".")):
                    p.mul_(GATE_SCALE)
    return net


def test_ffa_surface_equals_the_reference():
    import numpy as np
    g = np.load(GOLD)
    net = seeded_ffa(scaled=False)
    named = list(net.named_parameters())
    assert [n for n, _ in named] == list(g["names"])
    assert [",".join(map(str, p.shape)) for _, p in named] == list(g["shapes"])
    assert list(net.state_dict().keys()) == list(g["names"])           # no buffers: checkpoints interchange
    assert not list(net.buffers())
    stats = np.array([[p.mean().item(), p.std().item() if p.numel() > 1 else float("nan"), p.abs().max().item()] for _, p in named])
    assert np.allclose(stats, g["init_stats"], rtol=1e-6, atol=1e-9, equal_nan=True)   # same init stream, same draws (std of one element: nan)
    for attr in ("pre", "g1", "g2", "g3", "ca", "palayer", "post"):
        assert hasattr(net, attr)
    blk = net.g1.gp[0]
    for attr in ("conv1", "act1", "conv2", "calayer", "palayer"):
        assert hasattr(blk, attr)
    assert hasattr(blk.calayer, "ca") and hasattr(blk.palayer, "pa")


def test_ffa_refuses_other_group_counts():
    from dehaze_hip.ffa import FFA
    with pytest.raises(AssertionError):
        FFA(gps=2, blocks=1)


def test_ffa_cpu_forward_equals_the_reference():
    import numpy as np
    import torch
    g = np.load(GOLD)
    net = seeded_ffa()
    with torch.no_grad():
        y = net(torch.from_numpy(g["x"]))
    assert torch.allclose(y, torch.from_numpy(g["y"]), atol=1e-6, rtol=1e-5), (y - torch.from_numpy(g["y"])).abs().max()


def test_get_arch_builds_ffa(monkeypatch):
    monkeypatch.delenv("DHZ_FFA_BLOCKS", raising=False)
    import argparse
    import utils
    from dehaze_hip.ffa import FFA
    net = utils.get_arch(argparse.Namespace(arch="FFA", embed_dim=32, ffa_blocks=2))
    assert isinstance(net, FFA) and len(net.g1.gp) == 3 and len(net.g3.gp) == 3
    net = utils.get_arch(argparse.Namespace(arch="FFA", embed_dim=16))
    assert isinstance(net, FFA) and len(net.g2.gp) == 20
    monkeypatch.setenv("DHZ_FFA_BLOCKS", "3")                 # a script without --ffa_blocks (test_long_GPU.py)
    assert len(utils.get_arch(argparse.Namespace(arch="FFA", embed_dim=16)).g1.gp) == 4
    assert len(utils.get_arch(argparse.Namespace(arch="FFA", embed_dim=16, ffa_blocks=2)).g1.gp) == 3      # the option wins
    with pytest.raises(Exception, match="Arch error!"):
        utils.get_arch(argparse.Namespace(arch="FFA2", embed_dim=32))
