"""CPU-side checks of the Fourier / variance analysis (dehaze_hip/analysis.py, the argument contract of dhz_fourier_diag, the tap plan,
the CSV tables).  The reference everywhere is a float64 numpy restatement of the reference's notebooks (fourier_analysis.ipynb,
featuremap_variance.ipynb): np.fft.fft2 -> log(abs + 1e-6) -> roll by n / 2 -> diag()[n/2:], and var(ddof=1)."""
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
ENTRIES = ("dhz_fourier_diag_workspace_bytes", "dhz_fourier_diag")


def notebook(lat):
    """lat [B, C, n, n] float64 -> (A [B, C, n/2], V [B, C]) as the notebooks compute them, per map (before their mean)"""
    n = lat.shape[-1]
    amp = np.log(np.abs(np.fft.fft2(lat)) + 1e-6)
    amp = np.roll(amp, (n // 2, n // 2), axis=(-2, -1))
    A = np.stack([[np.diag(m)[n // 2:] for m in img] for img in amp])
    return A, lat.var(axis=(-2, -1), ddof=1)


def test_entries_are_declared_exported_and_bound():
    from dehaze_hip import _lib
    header = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        proto = re.search(r"\b%s\(([^;]*?)\);" % name, header, re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib._RESTYPE["dhz_fourier_diag_workspace_bytes"] is ctypes.c_size_t
    assert _lib.SIGNATURES["dhz_fourier_diag"][5:10] == [ctypes.c_int] * 5 and _lib.SIGNATURES["dhz_fourier_diag"][11] is ctypes.c_size_t


def test_workspace_bytes():
    from dehaze_hip import _lib
    wb = _lib.load().dhz_fourier_diag_workspace_bytes
    # rows are cut into chunks of at least 8; per (image, chunk): n C doubles of g and 2 C doubles of variance sums
    for layout in (0, 1):
        assert wb(1, 1, 2, layout) == (2 + 2) * 8
        assert wb(3, 48, 8, layout) == 3 * 48 * (8 + 2) * 8
        assert wb(1, 3, 66, layout) == 9 * 3 * (66 + 2) * 8                     # 66 rows: eight chunks of 8 and one of 2
        assert wb(2, 5, 130, layout) == 17 * 2 * 5 * (130 + 2) * 8
        for bad in ((0, 3, 16), (1, 0, 16), (1, 3, 0), (1, 3, 7), (1, 3, 2050), (1, 3, 2049), (65536, 1, 2), (1, 65536, 2), (-1, 3, 16)):
            assert wb(*bad, layout) == 0, bad
        assert wb(1, 1, 2048, layout) > 0
    assert wb(1, 3, 16, 2) == 0 and wb(1, 3, 16, -1) == 0
    # many maps: the rows of a map stay whole (tokens count 32-channel tiles, NCHW maps)
    assert wb(64, 512, 32, 0) == 64 * 512 * (32 + 2) * 8 and wb(32, 32, 128, 1) == 32 * 32 * (128 + 2) * 8
    assert wb(32, 32, 128, 0) == 16 * 32 * 32 * (128 + 2) * 8                   # 32 (image, tile) pairs: 16 chunks of 8 rows


def test_entry_rejects_bad_arguments_without_gpu():
    """DHZ_EINVAL with a dhz_last_error() string before any launch (safe on a GPU-less host; the pointers are never dereferenced)"""
    from dehaze_hip import _lib
    lib = _lib.load()
    P = 4096                                    # any aligned non-null value

    def diag(A=P, V=P, sumA=P, sumV=P, x=P, B=1, C=3, n=16, layout=0, dtype=0, ws=P, ws_bytes=None):
        need = lib.dhz_fourier_diag_workspace_bytes(B, C, n, layout)
        return lib.dhz_fourier_diag(A, V, sumA, sumV, x, B, C, n, layout, dtype, ws, need if ws_bytes is None else ws_bytes, None)

    def refused(rc, what):
        msg = lib.dhz_last_error()
        return rc == -22 and msg and what in msg and b"dhz_fourier_diag" in msg

    for n in (1, 3, 7, 129, 2047):
        assert refused(diag(n=n, ws_bytes=1 << 30), b"odd"), n
    for n in (0, -2, 2050, 4096):
        assert refused(diag(n=n, ws_bytes=1 << 30), b"out of range"), n
    for layout in (-1, 2, 7):
        assert refused(diag(layout=layout, ws_bytes=1 << 30), b"layout"), layout
    for dtype in (-1, 2, 3):
        assert refused(diag(dtype=dtype), b"dtype"), dtype
    for kw in (dict(B=0), dict(C=0), dict(B=-1), dict(B=65536), dict(C=65536)):
        assert refused(diag(ws_bytes=1 << 30, **kw), b"bad sizes"), kw
    for kw in (dict(A=None), dict(V=None), dict(sumA=None), dict(sumV=None), dict(x=None)):
        assert refused(diag(**kw), b"null pointer"), kw
    need = lib.dhz_fourier_diag_workspace_bytes(1, 3, 16, 0)
    assert need == 2 * 3 * (16 + 2) * 8
    assert refused(diag(ws=None), b"workspace missing") and str(need).encode() in lib.dhz_last_error()
    assert refused(diag(ws_bytes=need - 1), b"too small") and str(need).encode() in lib.dhz_last_error()      # names the bytes needed
    assert refused(diag(ws_bytes=0), b"too small")
    assert refused(diag(ws=P + 4), b"aligned") and refused(diag(A=P + 4), b"aligned") and refused(diag(x=P + 2), b"aligned")
    assert refused(diag(x=P + 1, dtype=1), b"aligned")


@pytest.mark.parametrize("n", [2, 4, 6, 8, 66])
def test_aten_formula_on_cpu_is_the_notebook(n, monkeypatch):
    """the DHZ_FOURIER=0 arm / the CPU route: float64 in, the numpy restatement to 1e-12, in both layouts, per map and summed"""
    from dehaze_hip import analysis
    g = torch.Generator().manual_seed(n)
    lat = torch.randn(2, 3, n, n, generator=g, dtype=torch.float64)
    A_ref, V_ref = notebook(lat.numpy())
    for kernels in (True, False):                 # CPU tensors take the formula whatever the switch says
        monkeypatch.setattr(analysis, "KERNELS", kernels)
        for layout, x in (("nchw", lat), ("tokens", lat.permute(0, 2, 3, 1).reshape(2, n * n, 3))):
            A, V = analysis.diag_log_amplitude(x, layout, per_map=True)
            assert A.dtype == V.dtype == torch.float64 and A.shape == (2, 3, n // 2) and V.shape == (2, 3)
            assert np.abs(A.numpy() - A_ref).max() <= 1e-12 and np.abs(V.numpy() / V_ref - 1).max() <= 1e-12
            sA, sV = analysis.diag_log_amplitude(x, layout)
            assert sA.shape == (n // 2,) and sV.dim() == 0
            assert np.abs(sA.numpy() - A_ref.sum((0, 1))).max() <= 1e-12 * 6 * np.abs(A_ref).max() + 1e-12
            assert abs(sV.item() / V_ref.sum() - 1) <= 1e-12
    # the diagonal identity the kernel rests on, in numpy: F[k][k] = sum_s g[s] exp(-2 pi i k s / n), g[s] = sum over (y + x) mod n = s
    f = lat[0, 0].numpy()
    s = (np.arange(n)[:, None] + np.arange(n)[None, :]) % n
    gvec = np.array([f[s == r].sum() for r in range(n)])
    k = np.arange(n // 2)
    Fd = (gvec[None, :] * np.exp(-2j * np.pi * ((k[:, None] * np.arange(n)[None, :]) % n) / n)).sum(1)
    assert np.abs(np.log(np.abs(Fd) + 1e-6) - A_ref[0, 0]).max() <= 1e-12


def test_fp32_and_bf16_cpu_inputs_and_the_fixed_order_sum():
    from dehaze_hip import analysis
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(2, 5, 8, 8, generator=g)
    A_ref, V_ref = notebook(lat.double().numpy())
    A, V = analysis.diag_log_amplitude(lat, "nchw", per_map=True)
    assert A.dtype == torch.float64 and np.abs(A.numpy() - A_ref).max() <= 1e-3 and np.abs(V.numpy() / V_ref - 1).max() <= 1e-5
    Ab, Vb = analysis.diag_log_amplitude(lat.bfloat16(), "nchw", per_map=True)
    A_refb, V_refb = notebook(lat.bfloat16().double().numpy())
    assert np.abs(Ab.numpy() - A_refb).max() <= 1e-3 and np.abs(Vb.numpy() / V_refb - 1).max() <= 1e-5
    # fixed_order_sum restates the kernel's order: partial j = maps j, j + 16, ..., then the partials in order
    v = torch.randn(3, 11, 4, generator=g, dtype=torch.float64)
    flat = v.reshape(33, 4).numpy()
    want = np.zeros(4)
    parts = [np.zeros(4) for _ in range(16)]
    for m in range(33):
        parts[m % 16] = parts[m % 16] + flat[m]
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    assert np.array_equal(analysis.fixed_order_sum(v).numpy(), want)
    assert analysis.fixed_order_sum(v[..., 0]).shape == ()


def test_bad_shapes_and_dtypes_raise_value_error_naming_the_shape():
    from dehaze_hip import analysis
    for x, layout, what in ((torch.zeros(1, 15, 4), "tokens", "15 tokens"), (torch.zeros(2, 9, 4), "tokens", "n=3"),
                            (torch.zeros(2, 4, 5, 5), "nchw", "n=5"), (torch.zeros(2, 4, 4, 6), "nchw", "square"),
                            (torch.zeros(2, 16), "tokens", "[B, n*n, C]"), (torch.zeros(1, 16, 4, dtype=torch.float16), "tokens", "dtype"),
                            (torch.zeros(1, 16, 4, dtype=torch.int32), "tokens", "dtype"), (torch.zeros(1, 16, 4), "nhwc", "layout")):
        with pytest.raises(ValueError, match=re.escape(what)) as e:
            analysis.diag_log_amplitude(x, layout)
        assert layout == "nhwc" or str(tuple(x.shape)) in str(e.value), str(e.value)


@pytest.mark.parametrize("module,kw", [("My_model_1", {}), ("My_model", {}), ("My_model_1", dict(embed_dim=16, token_mlp="leff", img_size=64,
                                                                                                  depths=[1, 2, 1, 2, 1, 2, 1, 2, 1]))])
def test_tap_plan_from_the_module_tree(module, kw):
    """1 + 2 (number of blocks) + 8 taps with the right kinds and sides, without a forward"""
    import importlib
    from dehaze_hip import analysis
    from dehaze_hip.model import LeWinTransformerBlock
    model = importlib.import_module(module).Uformer(**kw)
    plan = analysis.tap_plan(model)
    nblocks = sum(isinstance(m, LeWinTransformerBlock) for m in model.modules())
    assert len(plan) == 1 + 2 * nblocks + 8 and (kw or nblocks == 18)
    E, S = model.embed_dim, model.reso
    assert plan[0] == ("input_proj", "proj", S, E)
    kinds = [k for _, k, _, _ in plan]
    assert kinds.count("pool") == 4 and kinds.count("up") == 4 and kinds.count("msa") == kinds.count("mlp") == nblocks
    assert all(k in analysis.KINDS for k in kinds)
    # forward order: proj, then per encoder stage its (msa, mlp) pairs and the pool; the bottleneck; per decoder stage the up and its pairs
    depths = kw.get("depths", [2] * 9)
    want = ["proj"]
    sides, chans = [S], [E]
    for s in range(4):
        want += ["msa", "mlp"] * depths[s] + ["pool"]
        sides += [S >> s] * (2 * depths[s]) + [S >> (s + 1)]
        chans += [E << s] * (2 * depths[s]) + [E << (s + 1)]
    want += ["msa", "mlp"] * depths[4]
    sides += [S >> 4] * (2 * depths[4])
    chans += [E << 4] * (2 * depths[4])
    for s in range(4):
        want += ["up"] + ["msa", "mlp"] * depths[5 + s]
        sides += [S >> (3 - s)] * (1 + 2 * depths[5 + s])
        chans += [E << (4 - s)] * (1 + 2 * depths[5 + s])
    assert kinds == want and [n for _, _, n, _ in plan] == sides and [c for _, _, _, c in plan] == chans
    names = [n for n, _, _, _ in plan]
    assert len(set(names)) == len(names) and names[1] == "encoderlayer_0.blocks.0.msa" and names[2] == "encoderlayer_0.blocks.0.mlp"
    for name, kind, _, _ in plan:                 # every name resolves in the module tree
        model.get_submodule(name[:-4] if kind in ("msa", "mlp") else name)
    with pytest.raises(TypeError):
        analysis.tap_plan(torch.nn.Linear(2, 2))


def test_taps_on_cpu_collect_in_plan_order_and_leave_nothing_behind():
    """The model's forward needs the device, so the taps are driven by hand here (tests/test_gpu_fourier.py runs forwards): inside the
    context every planned tap has its hook or `_tap`; fed float64 latents of the planned shapes twice, the collector returns the notebook's
    means over both batches; afterwards no hook and no `_tap` is left."""
    import My_model_1
    from dehaze_hip import analysis
    from dehaze_hip.model import LeWinTransformerBlock
    model = My_model_1.Uformer(img_size=32, embed_dim=4, depths=[1] * 9, num_heads=[1] * 9)
    plan = analysis.tap_plan(model)
    g = torch.Generator().manual_seed(1)
    fed = [[torch.randn(2, n * n, C, generator=g, dtype=torch.float64) for _ in range(2)] for _, _, n, C in plan]
    assert not any(m._forward_hooks for m in model.modules())
    with analysis.taps(model) as col:
        calls = []
        for name, kind, _, _ in plan:
            if kind == "msa":
                calls.append(model.get_submodule(name[:-4])._tap)
            else:
                hooks = list(model.get_submodule(name[:-4] if kind == "mlp" else name)._forward_hooks.values())
                assert len(hooks) == 1, name
                calls.append(lambda x, h=hooks[0]: h(None, (), x))
        for rnd in range(2):
            for call, xs in zip(calls, fed):
                call(xs[rnd])
    assert col.order == list(range(len(plan))) * 2
    rows = col.results()
    assert [(r["name"], r["kind"], r["n"], r["channels"]) for r in rows] == plan and [r["index"] for r in rows] == list(range(len(plan)))
    for r, xs in zip(rows, fed):
        n, C = r["n"], r["channels"]
        A_ref, V_ref = notebook(torch.cat(xs).reshape(4, n, n, C).permute(0, 3, 1, 2).numpy())
        assert r["maps"] == 4 * C and len(r["curve"]) == n // 2 == len(r["delta"]) and r["delta"][0] == 0.0
        assert np.abs(np.array(r["curve"]) - A_ref.mean((0, 1))).max() <= 1e-12, r["name"]
        assert np.abs(np.array(r["delta"]) - (A_ref.mean((0, 1)) - A_ref.mean((0, 1))[0])).max() <= 1e-12
        assert abs(r["variance"] / V_ref.mean() - 1) <= 1e-12
    assert not any(m._forward_hooks for m in model.modules())
    assert not any("_tap" in vars(m) for m in model.modules() if isinstance(m, LeWinTransformerBlock))
    assert all(m._tap is None for m in model.modules() if isinstance(m, LeWinTransformerBlock))
    with pytest.raises(RuntimeError, match="boom"):          # an exception inside the context still removes everything
        with analysis.taps(model):
            raise RuntimeError("boom")
    assert not any(m._forward_hooks for m in model.modules()) and all(m._tap is None for m in model.modules() if isinstance(m, LeWinTransformerBlock))


def test_csv_round_trip(tmp_path):
    from dehaze_hip import analysis
    rows = [dict(index=0, name="input_proj", kind="proj", n=8, channels=32, maps=64, curve=[1.0, 0.5, 0.25, -3.0],
                 delta=[0.0, -0.5, -0.75, -4.0], variance=0.1234567890123456),
            dict(index=3, name="dowsample_0", kind="pool", n=4, channels=64, maps=128, curve=[2.0, 1.0 / 3.0], delta=[0.0, 1.0 / 3.0 - 2.0],
                 variance=1e-17)]
    prefix = str(tmp_path / "sub" / "run")
    fpath, vpath = analysis.write_csv(prefix, rows)
    assert fpath == prefix + "_fourier.csv" and vpath == prefix + "_variance.csv" and os.path.exists(fpath) and os.path.exists(vpath)
    lines = open(fpath).read().splitlines()
    assert len(lines) == 2 and len(lines[0].split(",")) == 6 + 4 and len(lines[1].split(",")) == 6 + 2           # ragged
    back = analysis.read_csv(prefix)
    for r, b in zip(rows, back):
        assert {k: r[k] for k in b} == b                                                                         # bit-exact floats


def test_script_refuses_what_it_does_not_take():
    import My_fourier_analysis as S
    for argv in ([], ["--synthetic", "2", "--input_dir", "x"], ["--synthetic", "2", "--batch_size", "0"], ["--attention", "sparse"]):
        with pytest.raises(SystemExit):
            S.main(argv)
    p = lambda **kw: type("O", (), {"win_size": 8, "train_ps": 128, **kw})()          # noqa: E731
    assert S.side_multiple(p()) == 128 and S.side_multiple(p(train_ps=64)) == 64 and S.side_multiple(p(win_size=4)) == 64


def _opt(input_dir, batch_size=2, **kw):
    return type("O", (), {"win_size": 8, "train_ps": 128, "synthetic": 0, "input_dir": str(input_dir), "batch_size": batch_size, "seed": 0, **kw})()


def _png(path, h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    Image.fromarray(img).save(path)
    return img


def test_input_dir_route_reads_the_folders_the_other_scripts_read(tmp_path):
    """--input_dir <dir with hazy/>: PNG files (what dataset.py and generate_patches_SIDD.py hold) are listed, in sorted order, batched,
    scaled to [0, 1] as [B, 3, H, W]; other files are ignored; a folder without images, a non-square image, a side the model does not
    take and a change of size are refused with a message"""
    import My_fourier_analysis as S
    dev = torch.device("cpu")
    hazy = tmp_path / "ok" / "hazy"
    hazy.mkdir(parents=True)
    imgs = [_png(hazy / name, 128, 128, i) for i, name in enumerate(("b.png", "a.PNG", "c.png"))]
    _png(hazy / "d.jpg", 128, 128, 7)
    (hazy / "notes.txt").write_text("not an image")
    got = list(S.batches(_opt(tmp_path / "ok"), dev))
    assert [tuple(b.shape) for b in got] == [(2, 3, 128, 128), (2, 3, 128, 128)] and got[0].dtype == torch.float32
    for t, src in zip(torch.cat(got)[:3], (imgs[1], imgs[0], imgs[2])):                      # a.PNG, b.png, c.png (sorted), then d.jpg
        assert torch.equal(t, torch.from_numpy(src.astype(np.float32) / 255.).permute(2, 0, 1))
    assert [b.shape[0] for b in S.batches(_opt(tmp_path / "ok", batch_size=3), dev)] == [3, 1]
    assert [b.shape[0] for b in S.batches(_opt(tmp_path / "ok", train_ps=64), dev)] == [2, 2]            # 128 is a multiple of 64 too

    def refused(name, files, what, **kw):
        d = tmp_path / name / "hazy"
        d.mkdir(parents=True)
        for i, (fname, h, w) in enumerate(files):
            _png(d / fname, h, w, i)
        with pytest.raises(SystemExit, match=what):
            list(S.batches(_opt(tmp_path / name, **kw), dev))

    refused("empty", [], "no images")
    refused("rect", [("a.png", 128, 256)], "square")
    refused("odd", [("a.png", 96, 96)], "multiple of 128")
    refused("odd64", [("a.png", 96, 96)], "multiple of 64", train_ps=64)
    refused("mixed", [("a.png", 128, 128), ("b.png", 128, 128), ("c.png", 256, 256)], "one run averages maps of one size")
    with pytest.raises(SystemExit, match="no hazy/"):
        list(S.batches(_opt(tmp_path / "nowhere"), dev))
    (tmp_path / "txt" / "hazy").mkdir(parents=True)
    (tmp_path / "txt" / "hazy" / "a.txt").write_text("x")
    with pytest.raises(SystemExit, match="no images"):
        list(S.batches(_opt(tmp_path / "txt"), dev))


def test_default_paths_do_not_import_the_new_module():
    code = ("import sys; sys.path[:0] = [%r, %r]; import My_train, FFA_main, My_model_1, My_model, losses, metrics, loss_landscape; "
            "import dehaze_hip.train, dehaze_hip.model; import importlib.util; "
            "spec = importlib.util.spec_from_file_location('bench', %r); bench = importlib.util.module_from_spec(spec); "
            "spec.loader.exec_module(bench); assert hasattr(bench, 'main') or hasattr(bench, 'ROOT'); "
            "assert 'dehaze_hip.analysis' not in sys.modules; "
            "import My_fourier_analysis; assert 'dehaze_hip.analysis' in sys.modules" % (PKG, ROOT, os.path.join(ROOT, "bench.py")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "analysis" not in open(os.path.join(ROOT, "bench.py")).read()
