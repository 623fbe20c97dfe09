"""-m gpu: the host state between the HIP kernels and autograd - in-place parameter gradients (ops._grad_buf / _grad_pair / _ready), the
operands that Uformer.forward stages and the blocks consume, the deferred bias-table gradients (fused._PENDING_TABLES) - driven the ways a
plain forward + backward of all-leaf parameters never drives it: checkpointing, a backward pass that raises, a second pass over a retained
graph, one module twice in a graph, two forwards before a backward, frozen subsets, non-leaf parameters, partial backward.

Reference: oracle.uformer_oracle in float64 on the run's parameters, sample tables, DropPath vectors and selections (tests/_autograd_ref.py).
Every value check stands on two assertions made next to it (Reference.check): each window-head keeps a gap of more than 1e-4 max|M| between
the u-th and the (u+1)-th sparsity measure, and the kernel selected what float64 selects - no check is skipped for a near-tie.
Bounds, none measured here: blocks and layers - tests/test_gpu_fused.py::test_fused_equals_unfused_chain (y 2e-5 / 1e-4, dx 5e-5 / 1e-3,
parameter gradients 2e-4 + 2e-3 max|ref|); the model - tests/test_gpu_odd_batch.py::test_model_grads_64px_odd_batch_vs_oracle (loss 5e-5,
gradients, dx among them, 2e-4 + 2e-3 max|ref|; outputs 2e-4 / 1e-3).  Same kernels on the same operands in deterministic mode: torch.equal.

Partial backward (case 7), the decision of INTEGRATION.md: a leaf parameter's .grad is untouched or holds the FULL gradient, per route -
untouched where the node returns the gradient to autograd, which drops it (UNTOUCHED below); full where the node accumulates in place."""
import contextlib
import copy
import functools

import pytest
import torch

import _autograd_ref as R
from test_gpu_deterministic import deterministic

pytestmark = pytest.mark.gpu
MODES = ("default", "deterministic")
NAMES = tuple(R.BLOCKS)
# parameters whose gradient the route hands to autograd instead of accumulating in place: the kernel chain under autograd (4 x 4 windows)
UNTOUCHED = {"c64_w4": ("norm1.weight", "norm1.bias", "attn.relative_position_bias_table")}
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def mode(m):
    with (deterministic() if m == "deterministic" else contextlib.nullcontext()):
        yield


@functools.lru_cache(None)
def _case(name):
    return R.block_case(name)


def _block(name, dev):
    blk, x, gout, feeds = _case(name)
    return copy.deepcopy(blk).to(dev).train(), x.to(dev), gout.to(dev), feeds


def _forward(blk, x, feeds, calls=1, call=None):
    """blk applied `calls` times under the staging hooks; call(x): another way to run it once (functional_call)"""
    with R.Stage({blk: feeds}, direct=True) as st:
        y = x
        for _ in range(calls):
            y = blk(y) if call is None else call(y)
    assert len(st.seen) == calls
    return y


_REFS = {}


def _reference(name, calls, y):
    """the float64 reference of the block case under the selections of the run behind y (computed once per module); the selections of
    THIS run are those of float64 too"""
    tops = R.run_selections(y)
    assert len(tops) == calls
    if (name, calls) not in _REFS:
        blk, x, gout, feeds = _case(name)
        _REFS[name, calls] = R.block_reference(name, dict(blk.named_parameters()), x, gout, feeds, tops, calls)
    r = _REFS[name, calls]
    r["ref"].check()
    for t, own in zip(tops, r["ref"].own):
        assert torch.equal(t.sort(-1)[0], own.sort(-1)[0]), "selection differs from the float64 top-u"
    return r


def _grads(blk):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in blk.named_parameters()}


def _check_grads(got, ref, factor=1.0, none=(), what=""):
    """got {name: tensor or None} against factor * the float64 gradients; names in `none`, and parameters float64 gives no gradient
    (the dead attn.qkv / attn.proj), hold None"""
    for n, g in ref.items():
        if g is None or n in none:
            assert got[n] is None, (what, n, "expected no gradient")
        else:
            assert got[n] is not None, (what, n, "no gradient")
            ex = R.grad_excess(got[n], factor * g)
            print(f"{what} {n}: error / bound {ex:.3f}")
            assert ex <= 1.0, (what, n, ex)


def _check_y_dx(r, y=None, dx=None, factor=1.0):
    if y is not None:
        assert R.close_block_y(y, r["y"]), (y.detach().cpu().to(F64) - r["y"]).abs().max()
    if dx is not None:
        assert R.close_block_dx(dx, factor * r["dx"]), (dx.detach().cpu().to(F64) - factor * r["dx"]).abs().max()


# ----------------------------------------------------------------------------------------------------------------- 3. repeated backward
@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_second_backward_over_a_retained_graph_doubles_every_gradient(dev, name, m):
    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        x.requires_grad_()
        y = _forward(blk, x, feeds)
        r = _reference(name, 1, y)
        loss = (y * gout).sum()
        loss.backward(retain_graph=True)
        g1, dx1 = _grads(blk), x.grad.clone()
        loss.backward(retain_graph=True)
        g2, dx2 = _grads(blk), x.grad.clone()
        _check_y_dx(r, y, dx1)
        _check_grads(g1, r["grads"], what="first pass")
        _check_y_dx(r, None, dx2, 2.0)
        _check_grads(g2, r["grads"], 2.0, what="second pass")
        da, = torch.autograd.grad(loss, x, retain_graph=True)
        db, = torch.autograd.grad(loss, x, retain_graph=True)
        _check_y_dx(r, None, da)
        _check_y_dx(r, None, db)
        if m == "deterministic":
            assert torch.equal(dx2, 2 * dx1) and torch.equal(da, dx1) and torch.equal(db, dx1)
            for n in g1:
                assert (g1[n] is None and g2[n] is None) or torch.equal(g2[n], 2 * g1[n]), n


# ----------------------------------------------------------------------------------------------------------------- 4. two forwards, one graph
@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_one_block_applied_twice(dev, name, m):
    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        x.requires_grad_()
        y = _forward(blk, x, feeds, calls=2)
        r = _reference(name, 2, y)
        (y * gout).sum().backward()
        _check_y_dx(r, y, x.grad)
        _check_grads(_grads(blk), r["grads"], what="blk(blk(x))")


# ----------------------------------------------------------------------------------------------------------------- 5. frozen subsets
FROZEN = {
    "norms": lambda n: n.startswith(("norm1.", "norm2.")),
    "query weight": lambda n: n == "attn.ProbSpare.query_projection.weight",
    "biases": lambda n: n.endswith(".bias"),
    "table": lambda n: n.endswith("relative_position_bias_table"),
    "all": lambda n: True,
}


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("subset", tuple(FROZEN))
@pytest.mark.parametrize("name", NAMES)
def test_frozen_subset(dev, name, subset, m):
    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        frozen = [n for n, p in blk.named_parameters() if FROZEN[subset](n)]
        assert frozen
        for n, p in blk.named_parameters():
            p.requires_grad_(n not in frozen)
        x.requires_grad_()
        y = _forward(blk, x, feeds)
        r = _reference(name, 1, y)
        (y * gout).sum().backward()
        _check_y_dx(r, y, x.grad)
        _check_grads(_grads(blk), r["grads"], none=frozen, what=subset)         # frozen: .grad stays None, never zeros


# ----------------------------------------------------------------------------------------------------------------- 6. non-leaf parameters
def _masters(mod):
    masters = {n: p.detach().clone().requires_grad_() for n, p in mod.named_parameters()}
    return masters, {n: v * 1.0 for n, v in masters.items()}


def _check_non_leaf(mod, masters, loss, ref_grads, x=None, ref_dx=None):
    names = list(masters)
    got = torch.autograd.grad(loss, [masters[n] for n in names] + ([x] if x is not None else []), retain_graph=True, allow_unused=True)
    assert all(p.grad is None for p in mod.parameters()) and all(v.grad is None for v in masters.values())
    _check_grads(dict(zip(names, got)), ref_grads, what="autograd.grad")
    loss.backward()
    assert all(p.grad is None for p in mod.parameters())
    _check_grads({n: v.grad for n, v in masters.items()}, ref_grads, what="backward")
    if x is not None:
        assert R.close_block_dx(got[-1], ref_dx) and R.close_block_dx(x.grad, ref_dx)


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_non_leaf_parameters_block(dev, name, m):
    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        masters, params = _masters(blk)
        x.requires_grad_()
        y = _forward(blk, x, feeds, call=lambda t: torch.func.functional_call(blk, params, (t,)))
        r = _reference(name, 1, y)
        _check_y_dx(r, y)
        _check_non_leaf(blk, masters, (y * gout).sum(), r["grads"], x, r["dx"])


def _layer(kind, dev):
    """(module, input, float64 function of (P, x)) at 16 x 16, batch 2"""
    import My_model_1 as M1
    from oracle import uformer_oracle as O
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(32)
    if kind == "downsample":
        mod, x = M1.Downsample(32, 64), torch.randn(2, 256, 32, generator=g)
        f = lambda P, t: O.downsample(t, {"d." + k: v for k, v in P.items()}, "d")
    elif kind == "input_proj":
        mod, x = M1.InputProj(in_channel=3, out_channel=32, kernel_size=3, stride=1, act_layer=torch.nn.LeakyReLU), torch.rand(2, 3, 16, 16, generator=g)
        f = lambda P, t: O.input_proj(t, {"input_proj." + k: v for k, v in P.items()})
    else:
        mod, x = M1.OutputProj(in_channel=64, out_channel=3, kernel_size=3, stride=1), torch.randn(2, 256, 64, generator=g)
        f = lambda P, t: O.output_proj(t, {"output_proj." + k: v for k, v in P.items()})
    return mod.to(dev), x, f


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("kind", ["downsample", "input_proj", "output_proj"])
def test_non_leaf_parameters_layer(dev, kind, m):
    with mode(m):
        mod, x, f = _layer(kind, dev)
        P = R.f64(dict(mod.named_parameters()))
        x64 = x.to(F64).requires_grad_(kind != "input_proj")
        y64 = f(P, x64)
        gout = torch.randn(y64.shape, generator=torch.Generator().manual_seed(33))
        (y64 * gout.to(F64)).sum().backward()
        masters, params = _masters(mod)
        xd = x.to(dev).requires_grad_(kind != "input_proj")          # (an image that requires a gradient takes the library convolution)
        y = torch.func.functional_call(mod, params, (xd,))
        assert R.close_block_y(y, y64.detach()), (y.detach().cpu().to(F64) - y64.detach()).abs().max()
        _check_non_leaf(mod, masters, (y * gout.to(dev)).sum(), {n: v.grad for n, v in P.items()},
                        xd if xd.requires_grad else None, x64.grad)


# ----------------------------------------------------------------------------------------------------------------- 7. partial backward
@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_partial_backward_on_leaf_parameters(dev, name, m):
    """dx is the float64 dx; a leaf parameter's .grad is untouched where its node returns the gradient (UNTOUCHED) and holds the full
    gradient where the node accumulates in place - never a part, never zeros"""
    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        x.requires_grad_()
        y = _forward(blk, x, feeds)
        r = _reference(name, 1, y)
        loss = (y * gout).sum()
        dx, = torch.autograd.grad(loss, x, retain_graph=True)
        _check_y_dx(r, y, dx)
        assert x.grad is None
        _check_grads(_grads(blk), r["grads"], none=UNTOUCHED.get(name, ()), what="autograd.grad(loss, x)")
        for p in blk.parameters():
            p.grad = None
        loss.backward(inputs=[x])
        _check_y_dx(r, None, x.grad)
        _check_grads(_grads(blk), r["grads"], none=UNTOUCHED.get(name, ()), what="backward(inputs=[x])")


# ----------------------------------------------------------------------------------------------------------------- 2. interrupted backward
def _direct(kind, blk, x, feed, dev):
    """fused.block / fused.attn_branch called the way LeWinTransformerBlock.forward calls them"""
    from dehaze_hip import fused
    res, shift = blk.input_resolution[0], blk.shift_size
    idx = feed[0].to(torch.uint8).to(dev).contiguous()
    s1, s2 = (v.to(dev) for v in feed[1])
    mask = blk._shift_mask(res, res, dev) if shift > 0 else None
    table = blk.attn.relative_position_bias_table
    if kind == "block":
        return fused.block(x, blk.norm1, blk.attn.ProbSpare, table, idx, mask, s1, res, res, shift, blk.num_heads, blk.norm2, blk.mlp, s2)
    return fused.attn_branch(x, blk.norm1, blk.attn.ProbSpare, table, idx, mask, s1, res, res, shift, blk.num_heads)


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("kind,name", [("block", "c32_s0"), ("block", "c32_s4"), ("attn_branch", "c64_s4")])
def test_backward_after_an_interrupted_backward(dev, kind, name, m):
    """a tensor hook raises (a Python exception, no device fault) after the node has queued its table gradient; the next pass reduces
    its own tiles, and only them"""
    from dehaze_hip import fused

    class Interrupt(RuntimeError):
        pass

    def stop(g):
        raise Interrupt("stop")

    with mode(m):
        blk, x, gout, feeds = _block(name, dev)
        x1 = x.clone().requires_grad_()
        x1.register_hook(stop)
        y1 = _direct(kind, blk, x1, feeds[0], dev)
        with pytest.raises(Interrupt):
            (y1 * (3.0 * gout)).sum().backward()            # (another gradient than the second pass's: its tiles would show)
        for p in blk.parameters():
            p.grad = None
        x2 = x.clone().requires_grad_()
        y2 = _direct(kind, blk, x2, feeds[0], dev)
        tops = R.run_selections(y2)
        case = _case(name)
        if kind == "block":
            r = _reference(name, 1, y2)
        else:
            r = R.attn_reference(name, dict(case[0].named_parameters()), case[1], case[2], feeds[0], tops)
            r["ref"].check()
        (y2 * gout).sum().backward()
        torch.cuda.synchronize()
        assert not fused._PENDING_TABLES
        _check_y_dx(r, y2, x2.grad)
        _check_grads(_grads(blk), r["grads"], what="pass after the interrupted one")


# ----------------------------------------------------------------------------------------------------------------- the model: 1. and 4.
class _Models:
    def __init__(self, dev):
        import My_model_1 as M1
        kw = dict(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff')
        torch.manual_seed(R.MODEL_SEED)
        self.plain = M1.Uformer(**kw)
        self.ckpt = M1.Uformer(use_checkpoint=True, **kw)
        self.ckpt.load_state_dict(self.plain.state_dict())
        self.P = {k: v.clone() for k, v in self.plain.state_dict().items()}
        self.plain.to(dev).train()
        self.ckpt.to(dev).train()
        self.dev = dev
        self.refs = {}

    @staticmethod
    def blocks(model):
        return [b for st in model.stages() for b in st.blocks]

    def run(self, model, k, seed=5, x_grad=True):
        """forward k of `model` under the staging hooks: (loss, x, the Stage, output)"""
        from losses import CharbonnierLoss
        hazy, gt = R.model_inputs(k)
        blocks = self.blocks(model)
        feeds = R.model_feeds(blocks, k)
        x = hazy.to(self.dev).requires_grad_(x_grad)
        torch.manual_seed(seed)
        torch.cuda.manual_seed(seed)
        st = R.Stage({b: {k: f} for b, f in zip(blocks, feeds)}, direct=False)
        st.slot = k
        out = model(x)
        loss, _ = CharbonnierLoss().forward_clamped(out, gt.to(self.dev))
        return loss, x, st, out

    def reference(self, k, loss):
        """float64 once per module, under the selections of the plain run behind `loss`"""
        if k not in self.refs:
            hazy, gt = R.model_inputs(k)
            self.refs[k] = R.model_reference(self.P, hazy, gt, R.model_feeds(self.blocks(self.plain), k), R.run_selections(loss))
        self.refs[k]["ref"].check()
        return self.refs[k]

    def zero(self):
        for mdl in (self.plain, self.ckpt):
            for p in mdl.parameters():
                p.grad = None


@pytest.fixture(scope="module")
def models(dev):
    return _Models(dev)


def _check_model(model, loss, x, refs, what):
    """loss of the last forward against refs[-1]; gradients against the SUM of refs"""
    assert abs(loss.item() - refs[-1]["loss"].item()) < 5e-5, (what, loss.item(), refs[-1]["loss"].item())
    live = {n for n, _ in model.live_parameters()}
    got = {n: p.grad for n, p in model.named_parameters()}
    ref = {n: None if refs[0]["grads"][n] is None else sum(r["grads"][n] for r in refs) for n in got}
    assert {n for n, g in ref.items() if g is not None} == live
    _check_grads(got, ref, what=what)


@pytest.mark.parametrize("m", MODES)
def test_checkpointed_model_is_the_plain_model(models, m):
    """use_checkpoint=True differentiates the function its forward computed: the recomputation of every block runs on the sample table
    and the DropPath vectors the forward consumed, and neither generator moves differently"""
    with mode(m):
        models.zero()
        res = {}
        for tag, model in (("plain", models.plain), ("ckpt", models.ckpt)):
            loss, x, st, out = models.run(model, 0)
            if tag == "plain":
                ref = models.reference(0, loss)
            loss.backward()
            st.close()
            torch.cuda.synchronize()
            res[tag] = dict(loss=loss.detach(), dx=x.grad, out=out.detach(), seen=st.seen, cpu=torch.get_rng_state(), gpu=torch.cuda.get_rng_state(),
                            grads={n: p.grad for n, p in model.named_parameters()})
            assert R.grad_excess(x.grad, ref["dx"]) <= 1.0, (tag, R.grad_excess(x.grad, ref["dx"]))
            _check_model(model, loss, x, [ref], tag)
        p, c = res["plain"], res["ckpt"]
        # what each block consumed: 18 forward calls, and in the checkpointed build 18 recomputations on the same operands
        assert len(p["seen"]) == 18 and len(c["seen"]) == 36
        first = {id(b): (t, v) for b, t, v in c["seen"][:18]}
        for b, t, v in c["seen"][18:]:
            t0, v0 = first[id(b)]
            assert t is not None and torch.equal(t, t0), "a recomputation without the forward's sample table"
            assert (v is None) == (v0 is None) and (v is None or all(torch.equal(a, b_) for a, b_ in zip(v, v0))), "other DropPath vectors"
        assert torch.equal(p["cpu"], c["cpu"]) and torch.equal(p["gpu"], c["gpu"])
        if m == "deterministic":
            assert torch.equal(p["loss"], c["loss"]) and torch.equal(p["out"], c["out"]) and torch.equal(p["dx"], c["dx"])
            differ = [n for n, g in p["grads"].items() if not ((g is None and c["grads"][n] is None) or torch.equal(g, c["grads"][n]))]
            print("parameters whose gradients differ between the builds, image with a gradient:", differ)
            # an image that requires a gradient sends InputProj to the library convolution (InputProj.forward), whose weight gradient
            # no mode of this package makes reproducible from run to run; everything else is bit-equal here, and ...
            assert set(differ) <= {"input_proj.proj.0.weight", "input_proj.proj.0.bias"}, differ
            # ... on the route a training step takes (the image is data: InputProj on its HIP kernels) every gradient is
            got = {}
            for tag, model in (("plain", models.plain), ("ckpt", models.ckpt)):
                models.zero()
                loss, _, st, out = models.run(model, 0, x_grad=False)
                loss.backward()
                st.close()
                got[tag] = (loss.detach(), out.detach(), {n: q.grad for n, q in model.named_parameters()})
                _check_model(model, loss, None, [ref], tag + ", image without a gradient")
            assert torch.equal(got["plain"][0], got["ckpt"][0]) and torch.equal(got["plain"][1], got["ckpt"][1])
            for n, g in got["plain"][2].items():
                assert (g is None and got["ckpt"][2][n] is None) or torch.equal(g, got["ckpt"][2][n]), n
        # one more forward after the step
        outs = []
        for model in (models.plain, models.ckpt):
            with torch.no_grad():
                _, _, st, out = models.run(model, 0)
            st.close()
            outs.append(out)
        assert torch.allclose(outs[1], outs[0], atol=2e-4, rtol=1e-3)
        assert torch.allclose(outs[0].cpu().to(F64), ref["out"], atol=2e-4, rtol=1e-3)
        if m == "deterministic":
            assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("order", ["sum", "second then first"])
@pytest.mark.parametrize("m", MODES)
def test_two_forwards_before_the_backward(models, m, order):
    with mode(m):
        models.zero()
        model = models.plain
        l0, x0, st0, _ = models.run(model, 0)
        st0.close()
        l1, x1, st1, _ = models.run(model, 1)
        st1.close()
        refs = [models.reference(0, l0), models.reference(1, l1)]
        if order == "sum":
            (l0 + l1).backward()
        else:
            l1.backward()
            l0.backward()
        assert R.grad_excess(x0.grad, refs[0]["dx"]) <= 1.0 and R.grad_excess(x1.grad, refs[1]["dx"]) <= 1.0
        assert abs(l0.item() - refs[0]["loss"].item()) < 5e-5
        _check_model(model, l1, x1, refs, order)
