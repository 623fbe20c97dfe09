"""Shared by tests/test_gpu_autograd_contract.py and tests/test_autograd_contract_host.py: the float64 reference of a run and the
read-back of what the run consumed.  Nothing here needs a device.

Reference  oracle.uformer_oracle in float64, with two of its functions replaced for the length of a `with`: `_drop_path` multiplies by the
           DropPath vectors of the run instead of drawing, `prob_attention` takes the selection of the run (the kernel's own ranks) instead
           of its own top-u and records, per window and head, the gap between the u-th and (u+1)-th sparsity measure relative to max |M|.
Stage      forward pre-hooks on LeWin blocks.  The sample tables and DropPath vectors of these tests are the TEST's (functions of seeds,
           drawn on the CPU, so that the seeds can be searched there): a block called on its own gets them staged; inside a model the hook
           replaces what Uformer.forward staged and leaves alone what it did not - a block that finds nothing staged draws for itself,
           which is what a checkpoint recomputation did before BasicUformerLayer replayed the forward's operands.  Every call is recorded.
Seeds      chosen by `python tests/_autograd_ref.py` (CPU): for a block configuration the first seed, for the model the first table seed
           per block in execution order, at which every window-head of every call keeps a gap above GAP.  The tests assert the gap."""
import math
import os
import sys

import torch

if __name__ == "__main__":                   # (under pytest, tests/conftest.py has put the repository and the package on the path)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_ROOT, "research-and-implementation-of-image-dehazing-algorithm-based-on-vision-transformer_amd"), _ROOT]

from oracle import uformer_oracle as O

GAP = 1e-4                       # (M_(u) - M_(u+1)) / max |M| that every window-head of a test keeps, in float64
F64 = torch.float64

# (C, heads, map side, window, shift) and the route the block takes on the GPU
BLOCKS = {
    "c32_s0": (32, 1, 16, 8, 0),          # fused forward, fused backward (the kernel chain backward in deterministic mode)
    "c32_s4": (32, 1, 16, 8, 4),
    "c64_s4": (64, 2, 16, 8, 4),          # fused forward, chain backward, dhz_linear_bwd_pair
    "c64_w4": (64, 2, 8, 4, 2),           # 4 x 4 windows: the kernel chain under autograd
}
BATCH = 2
DROP = 0.1
BLOCK_SEEDS = {"c32_s0": 0, "c32_s4": 0, "c64_s4": 0, "c64_w4": 0}
# Uformer(embed_dim=32) at 64 x 64, batch 2: table seed per block in execution order, for the two inputs of the two-forward cases
MODEL_SEED = 1234
MODEL_TABLE_SEEDS = ([5, 10, 0, 1, 0, 3, 0, 0, 0, 1, 0, 1, 0, 0, 5, 5, 2, 12],
                     [0, 6, 1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 1, 3, 2, 5, 16])


# ----------------------------------------------------------------------------------------------------------------- what the tests feed
def sample_table(seed, N):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(N, (N, O.n_top(N)), generator=g)


def drop_vectors(seed, B, drop, p_keep=0.6):
    """two DropPath vectors as the model stages them - 0 or 1 / keep per image - drawn with MORE drops than drop = 0.1 gives two images"""
    if drop == 0.:
        return None
    g = torch.Generator().manual_seed(int(seed))
    return [torch.bernoulli(torch.full((B,), p_keep), generator=g) / (1.0 - drop) for _ in range(2)]


def block_case(name, seed=None):
    """everything a block test runs on, as CPU tensors: parameters (fp32, by state_dict key), x, gout, and per call of the block (two: the
    block applied to its own output) the sample table and the DropPath vectors"""
    import My_model_1 as M1
    C, heads, res, win, shift = BLOCKS[name]
    seed = BLOCK_SEEDS[name] if seed is None else seed
    torch.manual_seed(1000 + seed)
    blk = M1.LeWinTransformerBlock(dim=C, input_resolution=(res, res), num_heads=heads, win_size=win, shift_size=shift, token_mlp='leff',
                                   drop_path=DROP)
    g = torch.Generator().manual_seed(2000 + seed)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.ndim == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("relative_position_bias_table"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    x = torch.randn(BATCH, res * res, C, generator=g)
    gout = torch.randn(BATCH, res * res, C, generator=g)
    feeds = [(sample_table(3000 + 10 * seed + k, win * win), drop_vectors(4000 + 10 * seed + k, BATCH, DROP)) for k in range(2)]
    return blk, x, gout, feeds


def model_inputs(k):
    """input k (0, 1) of the model tests: hazy, gt [2, 3, 64, 64]"""
    g = torch.Generator().manual_seed(70 + k)
    gt = torch.rand(BATCH, 3, 64, 64, generator=g)
    hazy = (0.6 * gt + 0.4 * torch.rand(BATCH, 1, 1, 1, generator=g)).clamp(0, 1)
    return hazy, gt


def model_feeds(blocks, k, table_seeds=None):
    """per block of the model, in execution order, the sample table and DropPath vectors of forward k"""
    seeds = MODEL_TABLE_SEEDS[k] if table_seeds is None else table_seeds
    out = []
    for j, b in enumerate(blocks):
        drop = b.drop_path.drop_prob if hasattr(b.drop_path, "drop_prob") else 0.
        out.append((sample_table(5000 + 1000 * k + 50 * j + seeds[j], b.win_size * b.win_size), drop_vectors(6000 + 100 * k + j, BATCH, drop)))
    return out


# ----------------------------------------------------------------------------------------------------------------- the reference
class GapTooSmall(Exception):
    pass


class Reference:
    """tops: per attention call of the forward, in order, the selection [B_, H, u] the run made (None: the float64 top-u);
    scales: per DropPath application with drop > 0, in order, the [B] vector of the run.  stop_below: raise GapTooSmall at the first call
    whose gap is not above it (the seed search)."""

    def __init__(self, tops=None, scales=(), stop_below=None):
        self.tops = None if tops is None else list(tops)
        self.scales = list(scales)
        self.stop_below = stop_below
        self.gaps = []                      # per attention call: the smallest relative gap of its window-heads
        self.agree = []                     # per attention call: the run's selection IS the float64 top-u
        self.own = []                       # per attention call: the float64 top-u

    def _drop_path(self, x, p, training):
        if p == 0.0 or not training:
            return x
        r = self.scales.pop(0)
        assert r.shape == (x.shape[0],)
        return x * r.to(x.dtype).view((-1,) + (1,) * (x.ndim - 1))

    def _prob_attention(self, q, k, v, idx, bias=None, mask=None, return_aux=False):
        """O.prob_attention, line by line, with the selection given"""
        assert not return_aux
        B_, H, N, d = q.shape
        u = idx.shape[1]
        ks = k[:, :, idx, :]
        S = torch.matmul(q.unsqueeze(-2), ks.transpose(-2, -1)).squeeze(-2)
        Mq = (S.max(-1)[0] - S.sum(-1) / N).detach()
        srt = Mq.sort(-1, descending=True)[0]
        gap = ((srt[..., u - 1] - srt[..., u]) / Mq.abs().amax(-1)).min().item() if u < N else math.inf
        self.gaps.append(gap)
        if self.stop_below is not None and not gap > self.stop_below:
            raise GapTooSmall(len(self.gaps) - 1)
        top = Mq.topk(u, sorted=False)[1]
        self.own.append(top)
        if self.tops is not None:
            mine, top = top, self.tops.pop(0).to(top.device)
            assert top.shape == mine.shape, (top.shape, mine.shape)
            self.agree.append(torch.equal(top.sort(-1)[0], mine.sort(-1)[0]))
        bi = torch.arange(B_)[:, None, None]
        hi = torch.arange(H)[None, :, None]
        scores = torch.matmul(q[bi, hi, top], k.transpose(-2, -1)) * (1.0 / math.sqrt(d))
        ctx = v.mean(dim=-2, keepdim=True).expand(B_, H, N, d).clone()
        a = torch.softmax(scores, dim=-1)
        if bias is not None:
            a = a + bias[hi, top]
        if mask is not None:
            wi = (torch.arange(B_) % mask.shape[0])[:, None, None]
            a = a + mask[wi, top]
        a = torch.softmax(a, dim=-1)
        ctx[bi, hi, top] = torch.matmul(a, v)
        return ctx

    def __enter__(self):
        self._saved = (O.prob_attention, O._drop_path)
        O.prob_attention, O._drop_path = self._prob_attention, self._drop_path
        return self

    def __exit__(self, et, ev, tb):
        O.prob_attention, O._drop_path = self._saved
        if et is None:
            assert not self.scales and not self.tops, "the reference consumed fewer vectors / selections than the run recorded"
        return False

    def check(self):
        """the properties every value check rests on: no near-tie anywhere, and the run selected what float64 selects"""
        assert min(self.gaps) > GAP, f"a window-head with a selection gap of {min(self.gaps):.2e} max|M|: choose another seed"
        assert all(self.agree), f"the run's selection differs from the float64 top-u in attention calls {[i for i, a in enumerate(self.agree) if not a]}"


def f64(P):
    """fresh float64 leaves of a {name: tensor} mapping"""
    return {k: v.detach().cpu().to(F64).requires_grad_(True) if v.dtype.is_floating_point else v.detach().cpu() for k, v in P.items()}


def block_reference(name, P, x, gout, feeds, tops=None, calls=1, stop_below=None):
    """the block of BLOCKS[name] applied `calls` times to x in float64: dict(y, dx, grads {name: tensor or None}, ref=the Reference)"""
    C, heads, res, win, shift = BLOCKS[name]
    P = f64(P)
    x = x.detach().cpu().to(F64).requires_grad_(True)
    scales = [s for _, sc in feeds[:calls] if sc for s in sc]
    with Reference(tops, scales, stop_below) as ref:
        y = x
        for k in range(calls):
            y = O.lewin_block(y, P, "", heads, win, shift, "probsparse", feeds[k][0], DROP, True, input_resolution=res)
    (y * gout.detach().cpu().to(F64)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, grads={k: v.grad for k, v in P.items() if v.dtype.is_floating_point}, ref=ref)


def attn_reference(name, P, x, gout, feed, tops=None):
    """the attention branch alone (M1:839-872: x + drop_path(attention(LN(x)))), what fused.attn_branch computes: dict(y, dx, grads, ref)"""
    import torch.nn.functional as F
    C, heads, res, win, shift = BLOCKS[name]
    P = f64(P)
    x = x.detach().cpu().to(F64).requires_grad_(True)
    B, L, _ = x.shape
    mask = O.shift_attn_mask(res, res, win, shift, F64) if shift > 0 else None
    with Reference(tops, feed[1][:1]) as ref:
        y = F.layer_norm(x, (C,), P["norm1.weight"], P["norm1.bias"], 1e-5).view(B, res, res, C)
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else y
        aw = O.window_attention(O.window_partition(y, win), P, "attn.", heads, win, "probsparse", feed[0], mask)
        y = O.window_reverse(aw, win, res, res)
        y = torch.roll(y, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else y
        y = x + O._drop_path(y.reshape(B, L, C), DROP, True)
    (y * gout.detach().cpu().to(F64)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, grads={k: v.grad for k, v in P.items() if v.dtype.is_floating_point}, ref=ref)


def model_reference(P, hazy, gt, feeds, tops=None, stop_below=None):
    """Uformer(embed_dim=32) at 64 x 64 with the clamped Charbonnier loss in float64: dict(out, loss, dx, grads, ref)"""
    P = f64(P)
    x = hazy.detach().cpu().to(F64).requires_grad_(True)
    scales = [s for _, sc in feeds if sc for s in sc]
    with Reference(tops, scales, stop_below) as ref:
        out = O.uformer_forward(P, x, img_size=64, win=8, drop_path_rate=DROP, training=True, idx_seq=[f[0] for f in feeds])
    loss = O.charbonnier(torch.clamp(out, 0, 1), gt.detach().cpu().to(F64))
    loss.backward()
    return dict(out=out.detach(), loss=loss.detach(), dx=x.grad, grads={k: v.grad for k, v in P.items() if v.dtype.is_floating_point}, ref=ref)


# ----------------------------------------------------------------------------------------------------------------- read-back of a run
class Stage:
    """feeds: {block: [(table, vectors or None) per slot]}.  direct: the blocks are called on their own - slot = how often the block has
    been called, and the operands are staged; else (blocks inside a model) slot = self.slot, set by the test per model forward, and only
    what the model staged is replaced.  self.seen: per call (block, table or None, vectors or None) as the block is about to consume them."""

    def __init__(self, feeds, direct):
        self.feeds, self.direct, self.slot = feeds, direct, 0
        self.ncall = {b: 0 for b in feeds}
        self.seen = []
        self._handles = [b.register_forward_pre_hook(self._hook) for b in feeds]

    def _hook(self, blk, args):
        dev = args[0].device
        slot = self.ncall[blk] if self.direct else self.slot
        self.ncall[blk] += 1
        table, vec = self.feeds[blk][slot]
        if self.direct or blk._staged_idx is not None:
            blk._staged_idx = table.to(torch.uint8).to(dev).contiguous()
        if vec is not None and (self.direct or blk._staged_scales):
            blk._staged_scales = [v.to(dev) for v in vec]
        self.seen.append((blk, None if blk._staged_idx is None else blk._staged_idx.cpu().long(),
                          [v.cpu().clone() for v in blk._staged_scales] if blk._staged_scales else None))

    def close(self):
        for h in self._handles:
            h.remove()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


_RANK_AT = {"attn_fused_bwd": 3, "attn_chain_bwd": 6}


def run_selections(out):
    """the selections [B_, H, u] (int64, CPU) of every ProbSparse attention in the graph of `out`, in forward order, from the ranks that
    the nodes saved for their backward (rank < u: selected)"""
    nodes, seen, stack = [], set(), [out.grad_fn]
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        if type(n).__name__ in ("_BlockNodeBackward", "_AttnNodeBackward", "_PSWindowAttentionBackward"):
            nodes.append(n)
        stack.extend(f for f, _ in n.next_functions)
    tops = []
    for n in sorted(nodes, key=lambda n: n._sequence_nr()):
        kind = type(n).__name__
        if kind == "_PSWindowAttentionBackward":
            B_, H, d, N, _ = n.dims
            rank = n.saved_tensors[3]
        else:
            rec = n.recs[0] if kind == "_BlockNodeBackward" else n.rec
            rank, H, N = n.saved_tensors[_RANK_AT[rec.kind]], rec.geom[5], 64
        u = O.n_top(N)
        sel = (rank.view(-1, H, N).cpu() < u)
        assert (sel.sum(-1) == u).all()
        tops.append(sel.to(torch.int8).sort(dim=-1, descending=True, stable=True)[1][..., :u])
    return tops


# ----------------------------------------------------------------------------------------------------------------- bounds (not measured)
def close_block_y(got, ref):
    """outputs: tests/test_gpu_fused.py::test_fused_equals_unfused_chain"""
    return torch.allclose(got.detach().cpu().to(F64), ref, atol=2e-5, rtol=1e-4)


def close_block_dx(got, ref):
    return torch.allclose(got.detach().cpu().to(F64), ref, atol=5e-5, rtol=1e-3)


def grad_excess(got, ref):
    """parameter gradients, block and model level alike: |got - ref| <= 2e-4 + 2e-3 max |ref|; returns error / bound"""
    err = (got.detach().cpu().to(F64) - ref).abs().max().item()
    return err / (2e-4 + 2e-3 * ref.abs().max().item())


# ----------------------------------------------------------------------------------------------------------------- the seed search
def search_block_seed(name, tries=200):
    for seed in range(tries):
        blk, x, gout, feeds = block_case(name, seed)
        try:
            block_reference(name, dict(blk.named_parameters()), x, gout, feeds, calls=2, stop_below=GAP)
            return seed
        except GapTooSmall:
            continue
    raise RuntimeError(name)


def search_model_table_seeds(k, tries=400):
    import My_model_1 as M1
    torch.manual_seed(MODEL_SEED)
    model = M1.Uformer(img_size=64, embed_dim=32, win_size=8, token_projection='linear', token_mlp='leff')
    blocks = [b for st in model.stages() for b in st.blocks]
    hazy, gt = model_inputs(k)
    P = {n: v.to(F64) if v.dtype.is_floating_point else v for n, v in model.state_dict().items()}
    seeds = [0] * len(blocks)
    memo, state, block_fn = {}, {}, O.lewin_block

    def block(x, P_, pre, heads, win, shift, variant, idx, drop, *a, **kw):
        """a block whose own and upstream tables did not change since it last passed: its output of then"""
        j = state["n"]
        state["n"] += 1
        key = (j, tuple(seeds[:j + 1]))
        if key in memo:
            ref = state["ref"]
            ref.gaps.append(math.inf)
            del ref.scales[:2 if drop > 0 else 0]
            return memo[key]
        memo[key] = block_fn(x, P_, pre, heads, win, shift, variant, idx, drop, *a, **kw)
        return memo[key]

    O.lewin_block = block
    try:
        with torch.no_grad():
            for _ in range(tries * len(blocks)):
                feeds = model_feeds(blocks, k, seeds)
                state["n"] = 0
                try:
                    with Reference(None, [s for _, sc in feeds if sc for s in sc], GAP) as ref:
                        state["ref"] = ref
                        O.uformer_forward(P, hazy.to(F64), img_size=64, win=8, drop_path_rate=DROP, training=True, idx_seq=[f[0] for f in feeds])
                    return seeds
                except GapTooSmall as e:
                    seeds[e.args[0]] += 1
                    print(seeds, flush=True)
                    assert seeds[e.args[0]] < tries, (e.args[0], seeds)
    finally:
        O.lewin_block = block_fn
    raise RuntimeError(seeds)


if __name__ == "__main__":
    if sys.argv[1:] == ["blocks"]:
        print("BLOCK_SEEDS =", {n: search_block_seed(n) for n in BLOCKS})
    else:
        k = int(sys.argv[1])
        print(f"MODEL_TABLE_SEEDS[{k}] =", search_model_table_seeds(k), flush=True)
