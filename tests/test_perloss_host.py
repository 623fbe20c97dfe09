"""CPU-side checks of FFA-Net's own recipe (PerceptualLoss.py, dehaze_hip/perceptual.py, csrc/perceptual.hip, FFA_main.py): the new entries
are declared, exported, bound and refuse bad arguments without a device; the cosine schedule is the reference's formula; the library
path of LossNetwork equals the reference fixture tests/golden/ffa_perloss.npz (tests/golden/gen_golden_perloss.py) in float64; weight
files and `.pk` checkpoints load; a default VggEngine is still VGG19[:30]."""
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ffa_perloss.npz")
EINVAL = -22


def quiet_loss_network(**kw):
    from PerceptualLoss import LossNetwork
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LossNetwork(**kw)


def test_entries_are_declared_exported_and_bound():
    from dehaze_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    for name, nargs in (("dhz_mse_pair_fwd", 5), ("dhz_mse_pair_bwd", 7), ("dhz_maxpool2x2_blocked_bwd_add", 8)):
        m = re.search(r"\bint %s\(([^)]*)\)" % name, hdr)
        assert m, f"{name} is not declared in include/dehaze_hip.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
        assert hasattr(lib, name)


def test_entries_refuse_bad_arguments_without_a_device():
    from dehaze_hip import _lib
    lib = _lib.load()
    A, G, S, D = 4096, 8192, 12288, 16384                    # 16-byte aligned stand-ins: nothing is launched, nothing is read

    def refused(rc):
        assert rc == EINVAL, rc
        msg = lib.dhz_last_error()
        assert msg and len(msg) > 0
        return msg

    for a, g, s in ((None, G, S), (A, None, S), (A, G, None)):
        assert b"null" in refused(lib.dhz_mse_pair_fwd(a, g, s, 8, None))
    for a, g, gm, d in ((None, G, S, D), (A, None, S, D), (A, G, None, D), (A, G, S, None)):
        assert b"null" in refused(lib.dhz_mse_pair_bwd(a, g, gm, d, 8, 0, None))
    for count in (0, 6, -4):
        assert b"multiple of 4" in refused(lib.dhz_mse_pair_fwd(A, G, S, count, None))
        assert b"multiple of 4" in refused(lib.dhz_mse_pair_bwd(A, G, S, D, count, 1, None))
    for a, g in ((A + 4, G), (A, G + 8)):
        assert b"aligned" in refused(lib.dhz_mse_pair_fwd(a, g, S, 8, None))
    for a, g, d in ((A + 4, G, D), (A, G + 8, D), (A, G, D + 12)):
        assert b"aligned" in refused(lib.dhz_mse_pair_bwd(a, g, S, d, 8, 0, None))
    # the pooling backward with the tap's gradient
    assert b"null" in refused(lib.dhz_maxpool2x2_blocked_bwd_add(A, G, None, D, 4, 16, 16, None))
    assert b"even" in refused(lib.dhz_maxpool2x2_blocked_bwd_add(A, G, S, D, 4, 15, 16, None))
    assert b"even" in refused(lib.dhz_maxpool2x2_blocked_bwd_add(A, G, S, D, 0, 16, 16, None))
    assert b"aligned" in refused(lib.dhz_maxpool2x2_blocked_bwd_add(A, G, S + 4, D, 4, 16, 16, None))


def test_cosine_schedule_is_the_reference_formula():
    from dehaze_hip.train import lr_schedule_cosdecay
    T, lr0 = 100000, 1e-4
    for t in (0, 1, T // 2, T):
        want = 0.5 * (1 + math.cos(t * math.pi / T)) * lr0                  # FFA_model/main.py:52-54
        assert lr_schedule_cosdecay(t, T, lr0) == want
    assert lr_schedule_cosdecay(0, T, lr0) == lr0
    assert abs(lr_schedule_cosdecay(T // 2, T, lr0) - lr0 / 2) < 1e-19
    assert lr_schedule_cosdecay(T, T, lr0) == 0.0
    assert lr_schedule_cosdecay(1, T, lr0) < lr0


@pytest.mark.parametrize("case", [0, 1])
def test_library_path_equals_the_reference_fixture_in_float64(case):
    z = np.load(GOLD)
    net = quiet_loss_network().double()
    assert net.pretrained is False and not any(p.requires_grad for p in net.parameters())
    x = torch.from_numpy(z[f"x_{case}"]).double().requires_grad_(True)
    gt = torch.from_numpy(z[f"gt_{case}"]).double()
    loss = net(x, gt)
    loss.backward()
    want, gwant = float(z[f"loss_{case}"]), torch.from_numpy(z[f"grad_{case}"])
    assert loss.dim() == 0 and abs(loss.item() - want) <= 1e-10 * abs(want), (loss.item(), want)
    assert (x.grad - gwant).abs().max().item() <= 1e-10 * gwant.abs().max().item()
    feats = net.output_features(x.detach())
    assert [tuple(f.shape[1:]) for f in feats] == [(64, x.shape[2], x.shape[3]), (128, x.shape[2] // 2, x.shape[3] // 2),
                                                   (256, x.shape[2] // 4, x.shape[3] // 4)]
    norms = np.array([f.norm().item() for f in feats])
    assert np.allclose(norms, z[f"tapnorm_{case}"], rtol=1e-10, atol=0)


def test_perloss_is_the_reference_name_and_takes_a_sequential():
    import PerceptualLoss
    from dehaze_hip.perceptual import seeded_vgg16_init_, vgg16_feature_layers
    assert PerceptualLoss.PerLoss is PerceptualLoss.LossNetwork
    layers = vgg16_feature_layers()
    assert len(layers) == 16
    seeded_vgg16_init_(layers)
    seq = torch.nn.Sequential(*layers)
    net = PerceptualLoss.PerLoss(seq)                     # the reference's call: a supplied model is used as it is, without a warning
    assert net.vgg_layers is seq and net.layer_name_mapping == {'3': "relu1_2", '8': "relu2_2", '15': "relu3_3"}
    own = quiet_loss_network()
    for a, b in zip(net.state_dict().values(), own.state_dict().values()):
        assert torch.equal(a, b)                          # the seeded draw: 7 convolutions in order, a seed of its own
    g = torch.Generator().manual_seed(3)
    x, gt = torch.rand(1, 3, 16, 16, generator=g), torch.rand(1, 3, 16, 16, generator=g)
    assert torch.equal(net(x, gt), own(x, gt))


def test_torchvision_keyed_state_dict_loads_into_the_right_layers(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(11)
    cfg = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256)]
    sd = {}
    for n, cin, cout in cfg:
        sd[f"features.{n}.weight"] = torch.randn(cout, cin, 3, 3, generator=g)
        sd[f"features.{n}.bias"] = torch.randn(cout, generator=g)
    sd["features.17.weight"] = torch.randn(512, 256, 3, 3, generator=g)          # the rest of a whole vgg16 file is ignored
    sd["classifier.0.bias"] = torch.randn(4096, generator=g)
    path = str(tmp_path / "vgg16.pth")
    torch.save(sd, path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # a weight file: no seeded-random warning
        from PerceptualLoss import LossNetwork
        a = LossNetwork(weights=path)
        monkeypatch.setenv("DEHAZE_VGG16_WEIGHTS", path)
        b = LossNetwork()
    for net in (a, b):
        assert net.pretrained is True and not any(p.requires_grad for p in net.parameters())
        for n, _, _ in cfg:
            assert torch.equal(net.vgg_layers[n].weight, sd[f"features.{n}.weight"])
            assert torch.equal(net.vgg_layers[n].bias, sd[f"features.{n}.bias"])
    del sd["features.12.bias"]
    torch.save(sd, path)
    with pytest.raises(KeyError):
        LossNetwork(weights=path)


def test_pk_checkpoint_with_module_prefix_loads_into_ffa(tmp_path):
    import utils
    from dehaze_hip.ffa import FFA
    torch.manual_seed(5)
    src = FFA(gps=3, blocks=1)
    torch.manual_seed(6)
    dst = FFA(gps=3, blocks=1)
    path = str(tmp_path / "My_NH_ffa_3_1_best.pk")
    torch.save({'step': 7, 'max_psnr': 11.5, 'max_ssim': 0.4, 'ssims': [0.4], 'psnrs': [11.5], 'losses': [0.3] * 7,
                'model': {'module.' + k: v for k, v in src.state_dict().items()}}, path)
    utils.load_checkpoint(dst, path, map_location="cpu")
    for (k, a), b in zip(src.state_dict().items(), dst.state_dict().values()):
        assert torch.equal(a, b), k
    torch.save({'step': 7, 'model': src.state_dict()}, path)                     # without the prefix too
    torch.manual_seed(8)
    dst2 = FFA(gps=3, blocks=1)
    utils.load_checkpoint(dst2, path, map_location="cpu")
    assert all(torch.equal(a, b) for a, b in zip(src.state_dict().values(), dst2.state_dict().values()))


def test_default_engine_is_still_vgg19():
    from dehaze_hip import vgg
    from dehaze_hip.perceptual import POOL_AFTER16, TAPS16
    import My_CR
    assert vgg.CONVS == ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 256), (256, 512),
                         (512, 512), (512, 512), (512, 512), (512, 512))
    assert vgg.POOL_AFTER == (1, 3, 7, 11) and vgg.TAPS == (0, 2, 4, 8, 12)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        v19 = My_CR.Vgg19()
    eng = vgg.VggEngine([m for m in v19.modules() if isinstance(m, torch.nn.Conv2d)])
    assert eng.conv_shapes == vgg.CONVS and eng.pool_after == vgg.POOL_AFTER and eng.taps == vgg.TAPS
    net = quiet_loss_network()
    e16 = vgg.VggEngine([m for m in net.vgg_layers if isinstance(m, torch.nn.Conv2d)], POOL_AFTER16, TAPS16)
    assert e16.conv_shapes == vgg.CONVS[:7] and e16.pool_after == (1, 3) and e16.taps == (1, 3, 6)
    with pytest.raises(ValueError):
        vgg.VggEngine(e16.convs, (1, 3), (1, 3))          # the last tap must be the last convolution
    assert vgg.engine16_shape_ok(32, 32) and vgg.engine16_shape_ok(48, 80) and vgg.engine16_shape_ok(240, 240)
    assert not vgg.engine16_shape_ok(16, 32) and not vgg.engine16_shape_ok(24, 40) and not vgg.engine16_shape_ok(40, 64)


def test_ffa_main_options_are_the_reference_ones():
    import FFA_main
    opt = FFA_main.parse([])
    assert (opt.steps, opt.eval_step, opt.lr, opt.bs, opt.crop_size, opt.gps, opt.blocks) == (100000, 5000, 1e-4, 4, 240, 3, 20)
    assert opt.perloss is False and opt.no_lr_sche is False and opt.resume is False
    assert opt.model_path == './FFA_pretrain_weight/My_NH_ffa_3_20'
    opt = FFA_main.parse(["--perloss", "--no_lr_sche", "--resume", "--blocks", "19", "--model_dir", "out/", "--synthetic", "4",
                          "--val_synthetic", "2", "--deterministic"])
    assert opt.perloss and opt.no_lr_sche and opt.resume is True and opt.model_path == 'out/My_NH_ffa_3_19'
    assert FFA_main.parse(["--resume", "x.pk"]).resume == "x.pk"
