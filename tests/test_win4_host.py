"""CPU tests of the host side of 4 x 4 windows: the sample tables of a model with mixed windows consume the global generator like the
reference's per-block draws, and the library exports the window-parametrised entries."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W_ENTRIES = ("dhz_ps_attn_fwd_w", "dhz_ps_attn_bwd_w", "dhz_ps_attn_bwd_parts_w", "dhz_dense_attn_fwd_w", "dhz_dense_attn_bwd_w",
             "dhz_ln_partition_fwd_w", "dhz_ln_partition_bwd_w", "dhz_reverse_residual_fwd_w", "dhz_reverse_residual_bwd_w",
             "dhz_shift_mask_w", "dhz_bias_gather_w", "dhz_bias_table_grad_w")


def test_sample_tables_per_run_match_per_block_draws():
    """a 64-pixel model: seventeen blocks with L = 64 around one... the reference draws torch.randint(L, (L, u)) per block in block order"""
    import My_model_1 as M1
    from dehaze_hip.model import draw_sample_index, n_top, sample_runs
    model = M1.Uformer(img_size=64, embed_dim=16, win_size=8, token_projection='linear', token_mlp='leff')
    blocks = [b for st in model.stages() for b in st.blocks]
    Ls = [b.win_size ** 2 for b in blocks]
    assert Ls == [64] * 8 + [16] * 2 + [64] * 8
    runs = sample_runs(Ls)
    assert [(r.L, list(r)) for r in runs] == [(64, list(range(8))), (16, [8, 9]), (64, list(range(10, 18)))]
    assert (n_top(64), n_top(16)) == (25, 15)
    torch.manual_seed(321)
    ref = [torch.randint(L, (L, n_top(L))) for L in Ls]                # the reference: one draw per block, its own L
    state_ref = torch.get_rng_state()
    torch.manual_seed(321)
    model._stage_sample_indices(torch.device("cpu"))
    assert torch.equal(torch.get_rng_state(), state_ref), "the staged draws leave the global generator in another state"
    for b, r in zip(blocks, ref):
        assert b._staged_idx.dtype == torch.uint8 and torch.equal(b._staged_idx.long(), r)
    # seventeen blocks of L = 64 around one of L = 16, drawn run by run
    Ls = [64] * 9 + [16] + [64] * 8
    torch.manual_seed(5)
    ref = [torch.randint(L, (L, n_top(L))) for L in Ls]
    state_ref = torch.get_rng_state()
    torch.manual_seed(5)
    got = [None] * len(Ls)
    for run in sample_runs(Ls):
        idx = draw_sample_index(len(run), run.L)
        for i, j in enumerate(run):
            got[j] = idx[i]
    assert torch.equal(torch.get_rng_state(), state_ref)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # all windows 8 x 8: ONE draw, as before
    assert len(sample_runs([64] * 18)) == 1


def test_window_entries_declared_and_exported():
    from dehaze_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "dehaze_hip.h")).read()
    declared = set(re.findall(r"\b(dhz_[a-z0-9_]+)\s*\(", hdr))
    for name in W_ENTRIES:
        assert name in declared, f"{name} is not declared in include/dehaze_hip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES, f"{name} is not exported / bound"
    # argument checks run without a GPU: windows other than 4 and 8 are refused with a message
    assert lib.dhz_shift_mask_w(None, 32, 32, 2, 16, None) == -22 and b"4 or 8" in lib.dhz_last_error()
    assert lib.dhz_bias_gather_w(None, None, 1, 5, None) == -22 and lib.dhz_last_error()
    assert lib.dhz_ps_attn_bwd_parts_w(8, 2, 32, 16) == 0
    assert lib.dhz_ps_attn_bwd_parts_w(8192, 1, 32, 8) == lib.dhz_ps_attn_bwd_parts_d(8192, 1, 32)
    assert lib.dhz_ps_attn_bwd_parts_w(8192, 1, 32, 4) == 2048 and lib.dhz_ps_attn_bwd_parts_w(3, 16, 64, 4) == 48


def test_unsupported_window_message_names_4_and_8():
    import pytest
    from dehaze_hip import model, ops
    for win in (2, 16, 5):
        with pytest.raises(NotImplementedError) as e:
            model.check_window(win)
        assert "4x4" in str(e.value) and "8x8" in str(e.value)
    with pytest.raises(NotImplementedError):
        ops.shift_mask(32, 32, 8, torch.device("cpu"), win=16)
