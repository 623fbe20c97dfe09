"""No GPU: the dense 3x3 weight gradient (dhz_conv3x3_wgrad) and the LeakyReLU store (dhz_winograd_conv3x3_act) are declared in the
header, exported by the library and bound in _lib.SIGNATURES; their argument checks answer DHZ_EINVAL with a message before any launch;
the workspace query is a function of the shapes alone; the UNet module's keys, shapes, init statistics and CPU forward equal the
reference fixture tests/golden/unet_m1_dim32.npz."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dhz_conv3x3_wgrad", "dhz_conv3x3_wgrad_workspace_bytes", "dhz_conv3x3_wgrad_parts", "dhz_winograd_conv3x3_act")
EINVAL = -22
FAKE = 4096          # a non-null "device pointer": every check below fails before anything would touch it


def test_entries_declared_exported_bound():
    from dehaze_hip import _lib
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dehaze_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert "M1:28-40" in header


def wgrad(lib, x=FAKE, dy=FAKE, dw=FAKE, db=FAKE, ws=FAKE, ws_bytes=None, B=2, H=16, W=16, Cin=32, Kout=32):
    if ws_bytes is None:
        ws_bytes = lib.dhz_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Kout)
    return lib.dhz_conv3x3_wgrad(x, dy, dw, db, ws, ws_bytes, B, H, W, Cin, Kout, None)


@pytest.mark.parametrize("kw,word", [
    (dict(Cin=48), "Cin=48"),
    (dict(Kout=16), "Kout=16"),
    (dict(H=12, W=16), "H=12"),
    (dict(H=8, W=16), "H=8"),
    (dict(Cin=544), "Cin=544"),
    (dict(B=0), "B=0"),
    (dict(x=None), "null"),
    (dict(dy=None), "null"),
    (dict(dw=None), "null"),
    (dict(ws=None), "workspace"),
    (dict(ws_bytes=2 * (32 * 32 * 9 + 32) * 4 - 4), "workspace"),
])
def test_wgrad_refuses_with_a_message(kw, word):
    from dehaze_hip import _lib
    lib = _lib.load()
    assert lib.dhz_get_deterministic() == 0
    assert wgrad(lib, **kw) == EINVAL
    msg = lib.dhz_last_error().decode()
    assert "dhz_conv3x3_wgrad" in msg and word in msg, msg


def test_wgrad_deterministic_mode_names_the_bytes_it_needs():
    from dehaze_hip import _lib
    lib = _lib.load()
    try:
        _lib.call("dhz_set_deterministic", 1)
        _lib.call("dhz_set_det_workspace", None, 0)
        assert wgrad(lib) == EINVAL                       # its own workspace is not a way round the mode's
        need = lib.dhz_conv3x3_wgrad_workspace_bytes(2, 16, 16, 32, 32)
        assert str(need) in lib.dhz_last_error().decode()
    finally:
        _lib.call("dhz_set_deterministic", 0)


def test_workspace_query_depends_on_the_shapes_alone():
    from dehaze_hip import _lib
    lib = _lib.load()
    shapes = [(2, 16, 16, 32, 32), (1, 16, 16, 32, 64), (3, 8, 8, 64, 32), (2, 8, 8, 512, 32), (4, 32, 32, 32, 32), (32, 128, 128, 32, 32),
              (32, 8, 8, 512, 512)]
    base = [(lib.dhz_conv3x3_wgrad_workspace_bytes(*s), lib.dhz_conv3x3_wgrad_parts(*s)) for s in shapes]
    for (nbytes, parts), (B, H, W, Cin, Kout) in zip(base, shapes):
        assert parts >= 1 and nbytes == parts * (Kout * Cin * 9 + Kout) * 4
    assert base[0][1] == 2 and base[4][1] == 16           # 8 chunks -> 2 slabs; 64 chunks -> 16 slabs of 4
    try:
        _lib.call("dhz_set_reserved_cus", 100)
        _lib.call("dhz_set_deterministic", 1)
        assert [(lib.dhz_conv3x3_wgrad_workspace_bytes(*s), lib.dhz_conv3x3_wgrad_parts(*s)) for s in shapes] == base
    finally:
        _lib.call("dhz_set_deterministic", 0)
        _lib.call("dhz_set_reserved_cus", 0)
    for bad in [(2, 16, 16, 48, 32), (2, 12, 16, 32, 32), (0, 16, 16, 32, 32)]:
        assert lib.dhz_conv3x3_wgrad_workspace_bytes(*bad) == 0 and lib.dhz_conv3x3_wgrad_parts(*bad) == 0


def test_leaky_store_refuses_bad_arguments():
    from dehaze_hip import _lib
    lib = _lib.load()
    f = lib.dhz_winograd_conv3x3_act
    assert f(None, FAKE, None, 0, None, None, FAKE, 1, 16, 16, 32, 32, None) == EINVAL
    assert f(FAKE, FAKE, None, 0, None, None, FAKE, 1, 12, 16, 32, 32, None) == EINVAL
    assert f(FAKE, FAKE, None, 0, None, None, FAKE, 1, 16, 16, 32, 16, None) == EINVAL
    assert f(FAKE, FAKE, None, 1, None, None, FAKE, 1, 16, 16, 32, 32, None) == EINVAL        # backward without the saved activation
    assert f(FAKE, FAKE, FAKE, 1, FAKE, None, FAKE, 1, 16, 16, 32, 32, None) == EINVAL        # backward with a bias
    assert f(FAKE, FAKE, None, 0, FAKE, None, FAKE, 1, 16, 16, 32, 32, None) == EINVAL        # forward with a mask
    assert "dhz_winograd_conv3x3_act" in lib.dhz_last_error().decode()


# ---- the module: surface and CPU path against the reference fixture (tests/golden/gen_golden_unet.py)
GOLD = os.path.join(ROOT, "tests", "golden", "unet_m1_dim32.npz")
MODEL_SEED = 41


def seeded_unet():
    import random
    import numpy as np
    import torch
    from dehaze_hip.unet import UNet
    random.seed(MODEL_SEED)
    np.random.seed(MODEL_SEED)
    torch.manual_seed(MODEL_SEED)
    return UNet(dim=32)


def test_unet_surface_equals_the_reference():
    import numpy as np
    g = np.load(GOLD)
    net = seeded_unet()
    named = list(net.named_parameters())
    assert [n for n, _ in named] == list(g["names"])
    assert [",".join(map(str, p.shape)) for _, p in named] == list(g["shapes"])
    assert list(net.state_dict().keys()) == list(g["names"])           # no buffers: checkpoints interchange
    stats = np.array([[p.mean().item(), p.std().item(), p.abs().max().item()] for _, p in named])
    assert np.allclose(stats, g["init_stats"], rtol=1e-6, atol=1e-9)   # same init stream, same draws


def test_unet_cpu_forward_equals_the_reference():
    import numpy as np
    import torch
    g = np.load(GOLD)
    net = seeded_unet()
    with torch.no_grad():
        y = net(torch.from_numpy(g["x"]))
    assert torch.allclose(y, torch.from_numpy(g["y"]), atol=1e-6, rtol=1e-5), (y - torch.from_numpy(g["y"])).abs().max()
