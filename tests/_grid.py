"""Reserved-grid harness of tests/test_gpu_persistent.py (a plain helper module, not a conftest).

Every persistent grid of the library is "resident workgroups per CU x dhz_num_cus()" and dhz_set_reserved_cus(k) takes k compute units
away from all of them at once (csrc/api.hip).  reserved_grid(ncu) runs a block of calls on grids sized for ncu CUs, so that a small
problem already makes many trips of every grid-stride loop.  The setting is process-global and the whole suite shares one process:
it is always given back (0) on the way out.

dhz_num_cus() never goes below 8.  The levels the tests use:
  None  the whole device (no reservation), with shapes big enough to exceed its grids;
  8     grids of 8, 16, 24 or 64 workgroups: the GEMMs' XCD remap is on wherever the tile count is a multiple of 8;
  9     grids of 9, 18 or 27 workgroups: the remap is off.
"""
import contextlib

LEVELS = (None, 8, 9)
MAX_WG_PER_CU = 8          # 256-thread workgroups: 32 waves per CU at most


def _lib():
    from dehaze_hip import _lib as L
    return L


def physical_cus():
    """the device's CU count, whatever is reserved at the moment (as dehaze_hip/vgg.py sizes its non-persistent grid)"""
    lib = _lib().load()
    return lib.dhz_grid_cus() + lib.dhz_get_reserved_cus()


@contextlib.contextmanager
def reserved_grid(ncu):
    """persistent grids sized for ncu CUs inside the block (None: the whole device); yields the CU count the grids are sized for"""
    L = _lib()
    lib = L.load()
    if ncu is None:
        assert lib.dhz_get_reserved_cus() == 0
        yield lib.dhz_grid_cus()
        return
    phys = physical_cus()
    assert 8 <= ncu < phys
    try:
        L.call("dhz_set_reserved_cus", phys - ncu)
        assert lib.dhz_grid_cus() == ncu
        yield ncu
    finally:
        L.call("dhz_set_reserved_cus", 0)


def assert_trips(what, items, grid, unit=None):
    """a grid-stride loop of `grid` workgroups over `items` work items makes at least three trips and a ragged last one.  unit: when
    only a bound of the grid is known (grid = unit x an occupancy the runtime picks), items % unit != 0 makes the last trip ragged
    for every such grid."""
    assert grid >= 1
    assert items >= 3 * grid, f"{what}: {items} items on {grid} workgroups: fewer than three trips"
    assert items % (unit or grid) != 0, f"{what}: {items} items on {grid} workgroups: no ragged last trip"
