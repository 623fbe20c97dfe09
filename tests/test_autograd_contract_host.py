"""No device: the host state of tests/test_gpu_autograd_contract.py where it can be driven without one.
1. the deferred bias-table gradients (fused._PENDING_TABLES) on the recorder of tests/_window_log.py: a pass that raises leaves nothing the
   next pass takes for its own queued callback, a pass inside a pass keeps the outer one's entries;
2. BasicUformerLayer(use_checkpoint=True) hands the recomputation of a block what the forward consumed, on stand-in blocks that consume
   their staged operands the way LeWinTransformerBlock does;
3. the seeds of the GPU tests leave every window-head the selection gap those tests assert (float64, the search of tests/_autograd_ref.py)."""
import pytest
import torch
import torch.nn as nn
from torch.autograd import Function

import _autograd_ref as R
import _window_log

H = 2


class _TableNode(Function):
    """a node whose backward hands one table gradient to fused._table_backward, and whose forward starts like the nodes of fused.py"""

    @staticmethod
    def forward(ctx, x, table):
        from dehaze_hip import fused
        if fused._PENDING_TABLES:
            fused._drop_stale_tables()
        ctx.table = table
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        from dehaze_hip import fused
        assert fused._table_backward(torch.empty((3 * H, 64, 64)), 3 * H, ctx.table, H) is None
        return g, None


class _InnerPass(Function):
    """a node whose backward runs a backward pass of its own (what re-entrant checkpointing does)"""

    @staticmethod
    def forward(ctx, x, table):
        ctx.table = table
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        with torch.enable_grad():
            z = torch.zeros(3, requires_grad=True)
            _TableNode.apply(z, ctx.table).sum().backward()
        return g, None


def _table():
    return torch.empty((225, H), requires_grad=True)


FLUSH_ONE = "bias_table_grad_multi(1)"


def test_tables_of_one_pass_are_reduced_in_one_launch_at_its_end():
    from dehaze_hip import fused
    x = torch.zeros(3, requires_grad=True)
    with _window_log.recorder() as log:
        _TableNode.apply(_TableNode.apply(x, _table()), _table()).sum().backward()
    assert log == ["bias_table_grad_multi(2)"], log
    assert not fused._PENDING_TABLES


def test_pass_after_an_interrupted_pass_reduces_its_own_tables():
    from dehaze_hip import fused

    def stop(g):
        raise RuntimeError("stop")

    x = torch.zeros(3, requires_grad=True)
    x.register_hook(stop)
    t1, t2 = _table(), _table()
    with _window_log.recorder() as log:
        y = _TableNode.apply(_TableNode.apply(x, t1), t1)
        with pytest.raises(RuntimeError, match="stop"):
            y.sum().backward()
        assert log == [], log                                           # the engine ran no callback of the pass that raised
        assert sum(len(v) for v in fused._PENDING_TABLES.values()) == 2
        x2 = torch.zeros(3, requires_grad=True)
        _TableNode.apply(x2, t2).sum().backward()
    assert log == [FLUSH_ONE], log                                      # its own tile, not the two stale ones with it
    assert not fused._PENDING_TABLES


def test_interrupted_pass_then_a_pass_over_a_graph_built_before_it():
    """no forward between the two passes drops the stale entries: the second pass still queues its own callback"""
    from dehaze_hip import fused

    def stop(g):
        raise RuntimeError("stop")

    t1, t2 = _table(), _table()
    with _window_log.recorder() as log:
        y2 = _TableNode.apply(torch.zeros(3, requires_grad=True), t2)
        x = torch.zeros(3, requires_grad=True)
        x.register_hook(stop)
        y1 = _TableNode.apply(x, t1)
        with pytest.raises(RuntimeError, match="stop"):
            y1.sum().backward()
        y2.sum().backward()
        assert log == [FLUSH_ONE], log
        fused._drop_stale_tables()
    assert not fused._PENDING_TABLES


def test_pass_inside_a_pass_keeps_the_outer_entries():
    from dehaze_hip import fused
    x = torch.zeros(3, requires_grad=True)
    with _window_log.recorder() as log:
        # backward order: the outer table node queues, then the inner pass runs and ends, then the outer pass ends
        _TableNode.apply(_InnerPass.apply(x, _table()), _table()).sum().backward()
    assert log == [FLUSH_ONE, FLUSH_ONE], log
    assert not fused._PENDING_TABLES


def test_table_gradient_outside_a_pass_is_reduced_at_once():
    from dehaze_hip import fused
    with _window_log.recorder() as log:
        assert fused._table_backward(torch.empty((3 * H, 64, 64)), 3 * H, _table(), H) is None
    assert len(log) == 1 and log[0].startswith("bias_table_grad_w("), log
    assert not fused._PENDING_TABLES


# ----------------------------------------------------------------------------------------------------------------- checkpoint replay
class _Block(nn.Module):
    """consumes staged operands like LeWinTransformerBlock: the table and the padding words on entry, a DropPath vector per residual;
    draws for itself what it does not find"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(1.5))
        self._staged_idx = self._staged_pad = self._staged_scales = None
        self.took = []

    def forward(self, x, mask=None):
        idx, self._staged_idx = self._staged_idx, None
        pad, self._staged_pad = self._staged_pad, None
        s = [self._staged_scales.pop(0) if self._staged_scales else torch.bernoulli(torch.full((x.shape[0],), 0.5)) for _ in range(2)]
        self.took.append((idx, pad, s[0], s[1]))
        if idx is None:
            idx = torch.randint(64, (4,))
        return x * (self.w * idx.float().mean()) * s[0].view(-1, 1, 1) + torch.sin(x) * self.w * s[1].view(-1, 1, 1)


def _layer(use_checkpoint):
    from dehaze_hip.model import BasicUformerLayer
    layer = BasicUformerLayer(dim=32, output_dim=32, input_resolution=(16, 16), depth=2, num_heads=1, win_size=8, token_mlp='leff',
                              use_checkpoint=use_checkpoint)
    layer.blocks = nn.ModuleList([_Block(), _Block()])
    return layer


def _stage(layer, staged):
    g = torch.Generator().manual_seed(3)
    for b in layer.blocks:
        if staged:
            b._staged_idx = torch.randint(64, (4,), generator=g)
            b._staged_pad = torch.zeros(2, dtype=torch.int64)
            b._staged_scales = [torch.bernoulli(torch.full((2,), 0.6), generator=g) + 0.25 for _ in range(2)]


@pytest.mark.parametrize("staged", [True, False])
def test_checkpoint_recomputes_on_what_the_forward_consumed(staged):
    x0 = torch.randn(2, 5, 3, generator=torch.Generator().manual_seed(1))
    res = {}
    for ck in (False, True):
        layer = _layer(ck)
        _stage(layer, staged)
        torch.manual_seed(9)
        x = x0.clone().requires_grad_()
        y = layer(x)
        y.sum().backward()
        res[ck] = (y.detach(), x.grad, [b.w.grad for b in layer.blocks], torch.get_rng_state(), layer)
    (y0, dx0, g0, rng0, _), (y1, dx1, g1, rng1, layer) = res[False], res[True]
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert torch.equal(rng0, rng1)
    for b in layer.blocks:
        assert len(b.took) == 2                                      # the forward and its recomputation
        (i0, p0, a0, b0), (i1, p1, a1, b1) = b.took
        if staged:
            assert i1 is i0 and p1 is p0 and a1 is a0 and b1 is b0 and i0 is not None and p0 is not None
        else:
            assert i1 is None and torch.equal(a0, a1) and torch.equal(b0, b1)      # drawn inside, under the restored generator state
        assert b._staged_idx is None and b._staged_pad is None and not b._staged_scales


# ----------------------------------------------------------------------------------------------------------------- the seeds
@pytest.mark.parametrize("name", tuple(R.BLOCKS))
def test_block_seed_leaves_the_selection_gap(name):
    blk, x, gout, feeds = R.block_case(name)
    r = R.block_reference(name, dict(blk.named_parameters()), x, gout, feeds, calls=2)
    assert len(r["ref"].gaps) == 2 and min(r["ref"].gaps) > R.GAP, r["ref"].gaps
    assert R.search_block_seed(name) == R.BLOCK_SEEDS[name]            # the first seed that does


@pytest.mark.parametrize("k", [0, 1])
def test_model_table_seeds_leave_the_selection_gap(k):
    import My_model_1 as M1
    torch.manual_seed(R.MODEL_SEED)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff')
    blocks = [b for st in model.stages() for b in st.blocks]
    hazy, gt = R.model_inputs(k)
    feeds = R.model_feeds(blocks, k)
    with torch.no_grad(), R.Reference(None, [s for _, sc in feeds if sc for s in sc]) as ref:
        from oracle import uformer_oracle as O
        O.uformer_forward({n: v.double() if v.dtype.is_floating_point else v for n, v in model.state_dict().items()}, hazy.double(),
                          img_size=64, win=8, drop_path_rate=R.DROP, training=True, idx_seq=[f[0] for f in feeds])
    assert len(ref.gaps) == 18 and min(ref.gaps) > R.GAP, ref.gaps
