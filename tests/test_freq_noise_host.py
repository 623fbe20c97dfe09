"""CPU-side checks of the frequency-band noise (dehaze_hip/freq_noise.py, adversarial.py, My_robustness.py, the argument contract of
dhz_band_noise).  The fixture tests/golden/freq_noise.npz holds what the reference's ops/adversarial.py FreqAttack(Random(eps), f, s)
returns in fp32 on the CPU for n = 8, 16, 34 and the eleven band centres linspace(0, pi, 11) (tests/golden/gen_golden_freq_noise.py).

The fixture's own gap, per side: gap = max over the eleven bands of |fixture x_adv - (x.double() + ref64).float()|, ref64 the float64
restatement of the reference's formula (numpy.fft, shift, mask, unshift, inverse, real part) from eps * sign(draw).  It is the distance of
the reference's fp32 result from the correctly rounded one (one or two fp32 roundings of x: the reference forms x + eps r - x in fp32).
A route that computes the same quantity is held to 2 * gap of the fixture."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd")
ENTRIES = ("dhz_band_noise_workspace_bytes", "dhz_band_noise")
SIDES = (8, 16, 34)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "freq_noise.npz"))


def band64(d, w1, w2):
    """the reference's formula in float64: d [..., n, n] -> the part of d inside the band of widths (w1, w2)"""
    n = d.shape[-1]
    mask = np.zeros((n, n))
    mask[(n - w1) // 2:(n + w1) // 2, (n - w1) // 2:(n + w1) // 2] = 1.0
    mask[(n - w2) // 2:(n + w2) // 2, (n - w2) // 2:(n + w2) // 2] -= 1.0
    spec = np.roll(np.fft.fft2(d), (n // 2, n // 2), axis=(-2, -1)) * mask
    return np.fft.ifft2(np.roll(spec, (n // 2, n // 2), axis=(-2, -1))).real


def fixture_gap(golden, n):
    """(gap of side n, the correctly rounded x_adv per band)"""
    x = golden[f"n{n}_x"].astype(np.float64)
    d = float(golden["eps"]) * np.sign(golden[f"n{n}_draw"].astype(np.float64))
    exact = [(x + band64(d, int(w1), int(w2))).astype(np.float32) for w1, w2 in golden[f"n{n}_w"]]
    gap = max(np.abs(fx.astype(np.float64) - e).max() for fx, e in zip(golden[f"n{n}_x_adv"], exact))
    return gap, exact


def test_entries_are_declared_exported_and_bound():
    from dehaze_hip import _lib
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib._RESTYPE["dhz_band_noise_workspace_bytes"] is ctypes.c_size_t
    sig = _lib.SIGNATURES["dhz_band_noise"]
    assert sig[:4] == [ctypes.c_void_p] * 4 and sig[4:8] == [ctypes.c_int] * 4 and sig[8] is ctypes.c_double and sig[9] is ctypes.c_int
    assert sig[10] is ctypes.c_void_p and sig[11] is ctypes.c_size_t and sig[12] is ctypes.c_void_p and len(sig) == 13


def test_workspace_bytes():
    from dehaze_hip import _lib
    wb = _lib.load().dhz_band_noise_workspace_bytes
    for M, n in ((1, 2), (6, 8), (7, 34), (96, 128), (3, 512), (65535, 2), (8191, 512)):
        assert wb(M, n) == (4 * n + 4 * M * n * n) * 8, (M, n)                  # the four vectors, the four row products
    for bad in ((0, 16), (-1, 16), (65536, 2), (1, 0), (1, 7), (1, 514), (1, 1024), (1, -2), (8192, 512)):    # 8192 * 512^2 = 2^31
        assert wb(*bad) == 0, bad


def test_entry_rejects_bad_arguments_without_gpu():
    """DHZ_EINVAL with a dhz_last_error() string before any launch (safe on a GPU-less host; the pointers are never dereferenced)"""
    from dehaze_hip import _lib
    lib = _lib.load()
    P, Q, R, N, W = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # aligned, far apart

    def band(out=P, noise=N, x=Q, delta=R, M=3, n=16, w1=8, w2=4, scale=1.0, take_sign=0, ws=W, ws_bytes=None):
        need = lib.dhz_band_noise_workspace_bytes(M, n)
        return lib.dhz_band_noise(out, noise, x, delta, M, n, w1, w2, scale, take_sign, ws, need if ws_bytes is None else ws_bytes, None)

    def refused(rc, what):
        msg = lib.dhz_last_error()
        return rc == -22 and msg and what in msg and b"dhz_band_noise" in msg

    for n in (1, 3, 7, 129, 511):
        assert refused(band(n=n, w1=0, w2=0, ws_bytes=1 << 30), b"odd"), n
    for n in (0, -2, 514, 1024):
        assert refused(band(n=n, w1=0, w2=0, ws_bytes=1 << 30), b"out of range"), n
    for M in (0, -1, 65536):
        assert refused(band(M=M, ws_bytes=1 << 30), b"bad sizes"), M
    assert refused(band(M=8192, n=512, ws_bytes=1 << 40), b"2^31")
    for kw in (dict(w1=7), dict(w2=3), dict(w1=18), dict(w1=-2), dict(w2=-2), dict(w1=16, w2=18)):
        assert refused(band(**kw), b"bad widths"), kw
    assert refused(band(w1=4, w2=8), b"exceeds")
    assert refused(band(take_sign=2), b"take_sign")
    for kw in (dict(out=None), dict(x=None), dict(delta=None)):
        assert refused(band(**kw), b"null pointer"), kw
    need = lib.dhz_band_noise_workspace_bytes(3, 16)
    assert need == (64 + 4 * 3 * 256) * 8
    assert refused(band(ws=None), b"workspace missing") and str(need).encode() in lib.dhz_last_error()
    assert refused(band(ws_bytes=need - 1), b"too small") and str(need).encode() in lib.dhz_last_error()     # names the bytes needed
    assert refused(band(ws_bytes=0), b"too small")
    assert refused(band(ws=W + 4), b"aligned") and refused(band(noise=N + 4), b"aligned") and refused(band(x=Q + 2), b"aligned")
    size = 3 * 16 * 16 * 4
    for kw in (dict(out=Q), dict(out=R), dict(out=Q + size - 4), dict(out=R - size + 4)):
        assert refused(band(**kw), b"aliases"), kw
    assert not refused(band(out=Q + size, ws_bytes=0), b"aliases")                # adjacent is no overlap (refused for the workspace instead)


def test_band_widths_equal_the_reference(golden):
    from dehaze_hip import freq_noise
    for n in SIDES:
        got = [freq_noise.band_widths(float(f), float(golden["s"]), n) for f in golden["fs"]]
        assert got == [tuple(w) for w in golden[f"n{n}_w"].tolist()], n
        assert all(w1 % 2 == 0 and w2 % 2 == 0 and 0 <= w2 <= w1 <= n for w1, w2 in got)
    assert freq_noise.band_widths(0.0, 0.2, 128) == (8, 0) and freq_noise.band_widths(np.pi, 0.2, 128) == (128, 118)


@pytest.mark.parametrize("n", SIDES)
def test_aten_route_on_cpu_is_the_reference(n, golden, monkeypatch):
    """the DHZ_FREQ_NOISE=0 arm / the CPU route from the draw and eps: within 2 * the fixture's own gap of the fixture, whatever the switch"""
    from dehaze_hip import freq_noise
    gap, exact = fixture_gap(golden, n)
    assert 0 < gap <= 4 * 2.0 ** -24, gap                   # a few fp32 roundings of x < 1
    x, draw = torch.from_numpy(golden[f"n{n}_x"]), torch.from_numpy(golden[f"n{n}_draw"])
    eps = float(golden["eps"])
    for kernels in (True, False):
        monkeypatch.setattr(freq_noise, "KERNELS", kernels)
        for i, (w1, w2) in enumerate(golden[f"n{n}_w"].tolist()):
            out = freq_noise.band_noise(x, draw, w1, w2, scale=eps, take_sign=True)
            assert out.dtype == torch.float32 and out.shape == x.shape
            err = np.abs(out.numpy().astype(np.float64) - golden[f"n{n}_x_adv"][i]).max()
            assert err <= 2 * gap, (i, err, gap)
            if w1 == w2:
                assert torch.equal(out, x)
    # float64 in: the restatement to rounding, noise returned in the input's precision
    x64, d64 = x.double(), draw.double()
    w1, w2 = golden[f"n{n}_w"][5].tolist()
    out, noise = freq_noise.band_noise(x64, d64, w1, w2, scale=eps, take_sign=True, return_noise=True)
    ref = band64(eps * np.sign(d64.numpy()), w1, w2)
    assert noise.dtype == torch.float64 and np.abs(noise.numpy() - ref).max() <= 1e-9 * eps
    assert np.array_equal(out.numpy(), x64.numpy() + noise.numpy())
    # non-contiguous inputs, and delta taken as it is
    xt = x.transpose(2, 3)
    out = freq_noise.band_noise(xt, draw.transpose(2, 3), w1, w2, scale=0.5)
    assert np.abs(out.numpy() - (xt.numpy() + 0.5 * band64(draw.transpose(2, 3).double().numpy(), w1, w2))).max() <= 1e-5


def test_random_reproduces_the_fixture_draw_and_freqattack_the_fixture(golden):
    import adversarial
    from dehaze_hip import freq_noise
    for n in SIDES:
        x, ys = torch.from_numpy(golden[f"n{n}_x"]), torch.zeros(2)
        seed, eps = int(golden[f"n{n}_seed"]), float(golden["eps"])
        rnd = adversarial.Random(eps=eps, gpu=False)
        torch.manual_seed(seed)
        assert torch.equal(rnd.draw(x), torch.from_numpy(golden[f"n{n}_draw"]))                     # bit for bit
        torch.manual_seed(seed)
        x_adv, ys2 = rnd(x, ys)
        assert torch.equal(x_adv, x + eps * torch.from_numpy(golden[f"n{n}_draw"]).sign()) and torch.equal(ys2, ys)
        gap, _ = fixture_gap(golden, n)
        for i in (2, 5, 10):
            f = float(golden["fs"][i])
            torch.manual_seed(seed)
            out, _ = adversarial.FreqAttack(rnd, f=f, s=float(golden["s"]))(x, ys)                  # the Random shortcut: draw and eps
            assert np.abs(out.numpy().astype(np.float64) - golden[f"n{n}_x_adv"][i]).max() <= 2 * gap
            # a general attack goes through x_adv - x, as the reference does
            torch.manual_seed(seed)
            out2, _ = adversarial.FreqAttack(lambda a, b: rnd(a, b), f=f, s=float(golden["s"]))(x, ys)
            assert np.abs(out2.numpy().astype(np.float64) - golden[f"n{n}_x_adv"][i]).max() <= 2 * gap
    assert "FGSM" in adversarial.__doc__ and "PGD" in adversarial.__doc__
    assert not hasattr(adversarial, "FGSM") and not hasattr(adversarial, "PGD")
    assert freq_noise.KERNELS == (os.environ.get("DHZ_FREQ_NOISE", "1") != "0")


def test_bad_shapes_raise_value_error_on_both_routes(monkeypatch):
    from dehaze_hip import freq_noise
    for kernels in (True, False):
        monkeypatch.setattr(freq_noise, "KERNELS", kernels)
        for shape, what in (((1, 3, 7, 7), "n=7"), ((1, 3, 8, 10), "square"), ((3, 8, 8), "square"), ((1, 3, 0, 0), "n=0")):
            x = torch.zeros(shape)
            with pytest.raises(ValueError, match=what) as e:
                freq_noise.band_noise(x, x.clone(), 0, 0)
            assert str(tuple(shape)) in str(e.value)
        x = torch.zeros(1, 3, 8, 8)
        for w1, w2 in ((3, 0), (10, 0), (4, 6), (4, -2)):
            with pytest.raises(ValueError, match="w"):
                freq_noise.band_noise(x, x.clone(), w1, w2)
        with pytest.raises(ValueError, match="does not match"):
            freq_noise.band_noise(x, torch.zeros(1, 3, 8, 6), 2, 0)


def test_script_refuses_what_it_does_not_take(tmp_path):
    import My_robustness as S
    for argv, what in (([], "one of them"), (["--synthetic", "2", "--input_dir", "x"], "one of them"),
                       (["--synthetic", "2", "--batch_size", "0"], "batch_size"), (["--synthetic", "2", "--bands", "0"], "bands"),
                       (["--synthetic", "2", "--train_ps", "72"], "multiple of 64"),
                       (["--synthetic", "2", "--arch", "UNet", "--train_ps", "72"], "multiple of 16"),
                       (["--input_dir", str(tmp_path / "nowhere")], "no gt/")):
        with pytest.raises(SystemExit, match=what):
            S.main(argv)
    (tmp_path / "half" / "hazy").mkdir(parents=True)
    with pytest.raises(SystemExit, match="no gt/"):
        S.main(["--input_dir", str(tmp_path / "half")])
    (tmp_path / "half" / "gt").mkdir()
    with pytest.raises(SystemExit, match="no images"):
        S.main(["--input_dir", str(tmp_path / "half")])
    from PIL import Image
    rng = np.random.default_rng(0)
    for name, side in (("a.png", 96), ("b.png", 96)):
        Image.fromarray(rng.integers(0, 256, (side, side, 3), dtype=np.uint8)).save(tmp_path / "half" / "hazy" / name)
    with pytest.raises(SystemExit, match="no ground truth for a.png"):
        S.main(["--input_dir", str(tmp_path / "half")])
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)).save(tmp_path / "half" / "gt" / name)
    opt = type("O", (), dict(arch="Uformer", win_size=8, train_ps=128, synthetic=0, input_dir=str(tmp_path / "half"), batch_size=2, seed=0))()
    with pytest.raises(SystemExit, match="multiple of 128"):                       # a side the model does not take
        list(S.batches(opt, torch.device("cpu")))
    opt.arch = "UNet"                                                              # 96 = 6 * 16: the UNet takes it
    (gt, hazy), = list(S.batches(opt, torch.device("cpu")))
    assert gt.shape == hazy.shape == (2, 3, 96, 96) and gt.dtype == torch.float32 and 0 <= float(hazy.min()) and float(hazy.max()) <= 1
    p = lambda **kw: type("O", (), {"arch": "Uformer", "win_size": 8, "train_ps": 128, **kw})()          # noqa: E731
    assert S.side_multiple(p()) == 128 and S.side_multiple(p(train_ps=64)) == 64 and S.side_multiple(p(win_size=4)) == 64
    assert S.side_multiple(p(arch="Uformer16", win_size=4)) == 128 and S.side_multiple(p(arch="UNet")) == 16 and S.side_multiple(p(arch="FFA")) == 2
    with pytest.raises(SystemExit, match="dense"):
        S.build_model(type("O", (), dict(arch="UNet", attention="dense"))())


def test_csv_header_and_rows(tmp_path):
    import csv
    import My_robustness as S
    rows = [dict(band="clean", f="", w1="", w2="", images=4, psnr=20.5, ssim=0.75, d_psnr=0.0, d_ssim=0.0)]
    rows += [dict(band=b, f=b * np.pi / 2, w1=w[0], w2=w[1], images=4, psnr=20.5 - b / 3, ssim=0.75 - b / 7, d_psnr=-b / 3, d_ssim=-b / 7)
             for b, w in enumerate(((8, 0), (68, 58), (128, 118)))]
    path = S.write_csv(str(tmp_path / "sub" / "run"), rows)
    assert path == str(tmp_path / "sub" / "run") + "_robustness.csv"
    back = list(csv.reader(open(path, newline="")))
    assert back[0] == ["band", "f", "w1", "w2", "images", "psnr", "ssim", "d_psnr", "d_ssim"] == S.HEADER
    assert len(back) == 1 + 4 and back[1][:4] == ["clean", "", "", ""] and [r[0] for r in back[2:]] == ["0", "1", "2"]
    for rec, r in zip(back[1:], rows):
        assert [float(v) for v in rec[5:]] == [r["psnr"], r["ssim"], r["d_psnr"], r["d_ssim"]]            # bit-exact floats
        assert int(rec[4]) == 4


def test_default_paths_do_not_import_the_new_module():
    code = ("import sys; sys.path[:0] = [%r, %r]; import dehaze_hip; assert 'dehaze_hip.freq_noise' not in sys.modules; "
            "import My_train, FFA_main, My_model_1, My_model, losses, metrics, loss_landscape, My_fourier_analysis; "
            "import dehaze_hip.train, dehaze_hip.model, dehaze_hip.analysis; "
            "assert 'dehaze_hip.freq_noise' not in sys.modules and 'adversarial' not in sys.modules; "
            "import My_robustness; assert 'dehaze_hip.freq_noise' in sys.modules" % (PKG, ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "freq_noise" not in open(os.path.join(ROOT, "bench.py")).read()
