"""CPU-side (-m "not gpu"): what the two stores of dataset.py ask the library to do, held line for line against the commit BEFORE
PatchStoreHBM.batch became one path and the three callers got one table builder.  `batch` is driven on CPU tensors under
tests/_launch_log.recorder (nothing is computed; gather_pair asserts device tensors and stays with the GPU tests).  numpy, `random` and
torch are seeded per case; a line holds the entry name with every non-pointer argument, the six floats behind `norm`, the contents of
store._table (and _draws for the image store), and a digest of each of the three generator states after the call - so a draw more, a draw
less, draws in another order, another entry, a permuted argument or another table cell changes a line.

tests/golden/feed_call_log_parent.txt was written by this file's `grid()` with the parent commit's dataset.py in front on sys.path
(python -c "import sys; sys.path.insert(0, <dir with the parent's dataset.py>); import test_feed_calls_host as t;
open('tests/golden/feed_call_log_parent.txt', 'w').write('\\n'.join(t.grid()) + '\\n')", run under tests/conftest.py's paths)."""
import hashlib
import os
import random

import numpy as np
import torch

import _launch_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(obj):
    return hashlib.sha1(repr(obj).encode()).hexdigest()[:12]


def _states():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return f"numpy {_digest((kind, keys.tolist(), pos, has_gauss, cached))} random {_digest(random.getstate())} " \
           f"torch {_digest(torch.get_rng_state().tolist())}"


def _run(out, seed, tag, store, *args, **kwargs):
    """one store.batch(...) -> one line"""
    from dehaze_hip import _lib
    np.random.seed(seed); random.seed(seed); torch.manual_seed(seed)
    store._table = store._draws = None
    norms = []
    with _launch_log.recorder() as log:
        record = _lib.call

        def call(name, *a):
            norm = a[5] if "ragged" in name else None           # the one pointer whose target the host reads
            norms.append("none" if norm is None else ",".join(f"{v:.9g}" for v in norm))
            record(name, *a)
        _lib.call = call                                        # (the recorder puts the library's own back)
        try:
            store.batch(*args, **kwargs)
        except Exception as e:                                  # noqa: BLE001 - a refusal is logged with its type and its words
            log.append(f"raises {type(e).__name__}: {e}")
    tab = store._table
    out.append(f"{tag} | {'; '.join(log)} | norm {'; '.join(norms)} | table {None if tab is None else (str(tab.dtype), tab.tolist())} | "
               f"draws {None if store._draws is None else store._draws.tolist()} | {_states()}")


def grid():
    """["case | call | norm | table | draws | generator states"] in a fixed order"""
    import dataset
    import utils
    g = torch.Generator().manual_seed(8)

    def u8(*shape):
        return torch.randint(0, 256, shape + (3,), generator=g, dtype=torch.uint8)

    out, seed = [], 100
    mixes = (("plain", None), ("mixup", utils.MixUp_AUG()))
    patches = dataset.PatchStoreHBM(u8(5, 12, 15), u8(5, 12, 15), "cpu")
    square = dataset.PatchStoreHBM(u8(5, 12, 12), u8(5, 12, 12), "cpu")
    idx = [4, 0, 2, 2, 1, 3, 7]
    for store, name, ps in ((patches, "12x15", 8), (patches, "12x15", (6, 9)), (patches, "12x15", (7, 7)), (patches, "12x15", None),
                            (square, "12x12", 12)):
        for mname, mix in mixes:
            seed += 1
            _run(out, seed, f"PatchStoreHBM {name} ps={ps} {mname}", store, idx, ps, mixup=mix)
    # hazy 10 x 13, 12 x 12 and twice 16 x 11; the last two share ONE clear frame, which is larger (18 x 14: centre-crop origin (1, 2))
    shared = u8(18, 14)
    images = dataset.ImageStoreHBM([(u8(10, 13), u8(10, 13)), (u8(12, 12), u8(12, 12)), (shared, u8(16, 11)), (shared, u8(16, 11))], "cpu")
    assert images.origin[2:] == [(1, 2), (1, 2)] and images.clear_of == [0, 1, 2, 2]
    for ps, idx in ((6, [3, 0, 1, 2, 2, 4]), ((5, 8), [1, 3, 0, 2, 3]), (None, [2, 3, 3, 2])):
        for nname, norm in (("raw", None), ("reside", (dataset.RESIDE_MEAN, dataset.RESIDE_STD))):
            for mname, mix in mixes:
                seed += 1
                _run(out, seed, f"ImageStoreHBM ps={ps} {nname} {mname}", images, idx, ps, normalize=norm, mixup=mix)
    # refusals: nothing is drawn, nothing is called
    for mname, mix in mixes:
        seed += 1
        _run(out, seed, f"PatchStoreHBM 12x15 ps=(13, 15) {mname}", patches, [0, 1], (13, 15), mixup=mix)
        _run(out, seed, f"PatchStoreHBM 12x15 ps=(12, 16) {mname}", patches, [0, 1], (12, 16), mixup=mix)
        _run(out, seed, f"ImageStoreHBM ps=11 {mname}", images, [1, 0], 11, mixup=mix)
        _run(out, seed, f"ImageStoreHBM ps=(5, 14) {mname}", images, [2, 0], (5, 14), mixup=mix)
        _run(out, seed, f"ImageStoreHBM ps=None two sizes {mname}", images, [2, 0], None, mixup=mix)
    _run(out, seed, "PatchStoreHBM 12x15 ps=13 mixup", patches, [0, 1], 13, mixup=mixes[1][1])
    return out


def test_the_stores_make_the_parent_commits_calls_tables_and_draws():
    with open(os.path.join(ROOT, "tests", "golden", "feed_call_log_parent.txt")) as f:
        parent = f.read().splitlines()
    got = grid()
    assert len(parent) == len(got) == 33
    # the log tells the cases apart: every entry is reached, the square entry by an int crop without MixUp only
    entries = [line.split(" | ")[1].split("(")[0] for line in parent[:22]]
    assert entries[:10] == ["crop_augment_pair", "crop_augment_mix_pair_rect"] + ["crop_augment_pair_rect", "crop_augment_mix_pair_rect"] * 3 \
        + ["crop_augment_pair", "crop_augment_mix_pair_rect"]
    assert entries[10:] == ["crop_augment_pair_ragged", "crop_augment_mix_pair_ragged"] * 6
    assert "PatchStoreHBM 12x15 ps=(6, 9) plain | crop_augment_pair_rect(7,12,15,6,9) | norm none | table ('torch.int32', [[4, " in parent[2]
    assert " | norm 0.639999986,0.600000024,0.579999983,0.140000001,0.150000006,0.151999995 | table ('torch.int64', [[" in parent[12] and " | norm none | " in parent[10]
    assert all(" | raises ValueError: " in line and " | table None | draws None | " in line for line in parent[22:])
    assert sum("does not fit" in line for line in parent[22:]) == 9 and sum("different sizes" in line for line in parent[22:]) == 2
    np.random.seed(123); random.seed(123); torch.manual_seed(123)
    assert {line.split(" | ")[-1] for line in parent[22:27]} == {_states()}          # a refusal draws nothing: the states are the seeded ones
    assert len({line.split(" | ")[-1] for line in parent[:22]}) == 22
    diff = [(p, g) for p, g in zip(parent, got) if p != g]
    assert not diff, f"{len(diff)} of {len(parent)} lines differ (parent, now), first: {diff[:2]}"
