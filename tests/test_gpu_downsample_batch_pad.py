"""-m gpu: Downsample (Conv2d k4 s2 p1 on tokens) with gradients at a batch whose output pixels are no multiple of 32 - the 256 -> 512 layer
onto the 4 x 4 map of 64-pixel patches at batch 3 or 1.  The implicit-GEMM kernels run it on a batch padded with zero images (the weight
gradient takes output pixels in 32s) instead of the library convolution: forward and every gradient against float64 conv2d at the bounds of
tests/test_gpu_conv.py::test_downsample_module_matches_library_conv, no library call, and the same bits from run to run in the
deterministic mode."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _run(ds, x, gout):
    ds.zero_grad(set_to_none=True)
    xa = x.clone().requires_grad_()
    y = ds(xa)
    y.backward(gout)
    return y.detach().clone(), xa.grad.clone(), ds.conv[0].weight.grad.clone(), ds.conv[0].bias.grad.clone()


@pytest.mark.parametrize("B,s,Cin,Cout", [(3, 8, 256, 512), (1, 8, 256, 512), (5, 4, 64, 128), (3, 8, 32, 64)])
def test_downsample_odd_batch_on_the_kernels(monkeypatch, B, s, Cin, Cout):
    import My_model_1 as M1
    from dehaze_hip import ops
    from test_gpu_deterministic import deterministic
    dev = torch.device("cuda:0")
    torch.manual_seed(B + s + Cin)
    ds = M1.Downsample(Cin, Cout).to(dev)
    x = torch.randn(B, s * s, Cin, device=dev)
    gout = torch.randn(B, (s // 2) ** 2, Cout, device=dev)
    assert (B * (s // 2) ** 2) % 32 != 0 and not ops.conv4s2_supported(x, s, s, True)

    def refuse(*a, **k):
        raise AssertionError("the library convolution was reached")

    with monkeypatch.context() as m:
        m.setattr(ops, "warn_library_fallback", refuse)
        m.setattr(F, "conv2d", refuse)
        y, dx, dw, db = _run(ds, x, gout)
        with deterministic():
            first, second = _run(ds, x, gout), _run(ds, x, gout)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    conv = ds.conv[0]
    w64, b64 = conv.weight.detach().double().requires_grad_(), conv.bias.detach().double().requires_grad_()
    x64 = x.double().requires_grad_()
    y64 = F.conv2d(x64.view(B, s, s, Cin).permute(0, 3, 1, 2), w64, b64, stride=2, padding=1).permute(0, 2, 3, 1).reshape(B, -1, Cout)
    y64.backward(gout.double())
    for what, got, want, atol, rtol in (("y", y, y64.detach(), 2e-4, 1e-4), ("dx", dx, x64.grad, 2e-4, 1e-3), ("dw", dw, w64.grad, 2e-3, 1e-3),
                                        ("db", db, b64.grad, 2e-3, 1e-3)):
        assert got.shape == want.shape
        print(f"Downsample({Cin}, {Cout}) B={B} {s}x{s} {what}: worst error {(got.double() - want).abs().max().item():.3e}")
        assert torch.allclose(got.double(), want, atol=atol, rtol=rtol), (what, (got.double() - want).abs().max().item())
    for a, b in zip(first, (y, dx, dw, db)):            # the mode computes what the default path computes
        assert torch.allclose(a, b, atol=2e-3, rtol=1e-3)
