"""CPU: the C ABI of occupancy-grid rendering (cn_occupancy_build,
cn_sparse_mark, cn_sparse_gather, cn_sparse_scatter): exported, bound, additive
to ABI 4, and every host check refuses with -1 and a message naming the entry
before anything is launched (the pointers below are never dereferenced); the
optimize.py flags and the Optimizer's argument checks."""
import ctypes
import os

import pytest

ENTRIES = ("cn_occupancy_build", "cn_sparse_mark", "cn_sparse_gather", "cn_sparse_scatter")
NAN, INF = float("nan"), float("inf")


def _lib():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load_library()


def test_the_four_symbols_are_exported_and_bound():
    L, lib = _lib()
    nargs = dict(zip(ENTRIES, (6, 16, 11, 9)))
    for name in ENTRIES:
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L._SIGS[name][1]) == nargs[name]
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert L._SIGS["cn_occupancy_build"][1] == [P, I, F, I, P, P]
    assert L._SIGS["cn_sparse_mark"][1] == [P, P, P, I, I, I, P, I, F, F, F, F, I, P, P, P]
    assert L.ABI_VERSION == 4 and lib.cn_abi_version() == 4


D = ctypes.c_void_p(256)


def _build(lib, sigma=D, G=32, tau=0.5, dilate=1, bits=D):
    return lib.cn_occupancy_build(sigma, G, tau, dilate, bits, None)


def _mark(lib, ro=D, z_stride=0, R=8, N=64, bits=D, G=32, lo=(-0.5, -0.5, -0.5), inv_cell=32.0, keep=D, count=D):
    return lib.cn_sparse_mark(ro, D, D, z_stride, R, N, bits, G, lo[0], lo[1], lo[2], inv_cell, 1, keep, count, None)


def _gather(lib, ro=D, z_stride=0, R=8, N=64, keep=D, offset=D, xyz=D):
    return lib.cn_sparse_gather(ro, D, D, z_stride, R, N, keep, offset, xyz, D, None)


def _scatter(lib, keep=D, R=8, N=64, sigma_k=D, rgb=D):
    return lib.cn_sparse_scatter(keep, D, R, N, sigma_k, D, D, rgb, None)


CALLS = dict(zip(ENTRIES, (_build, _mark, _gather, _scatter)))


def _refused(lib, entry, what, **kw):
    assert CALLS[entry](lib, **kw) == -1, (entry, kw)
    err = lib.cn_last_error()
    assert entry.encode() + b":" in err and what in err, err


def test_occupancy_build_refusals():
    _, lib = _lib()
    e = "cn_occupancy_build"
    _refused(lib, e, b"NULL argument", sigma=None)
    _refused(lib, e, b"NULL argument", bits=None)
    for G in (0, 16, 48, 288, 257, -32):
        _refused(lib, e, b"G must be a multiple of 32 in [32, 256]", G=G)
    for d in (-1, 5):
        _refused(lib, e, b"dilate must be in [0, 4]", dilate=d)
    _refused(lib, e, b"tau is NaN", tau=NAN)


def test_sparse_mark_refusals():
    _, lib = _lib()
    e = "cn_sparse_mark"
    for k in ("ro", "bits", "keep", "count"):
        _refused(lib, e, b"NULL argument", **{k: None})
    _refused(lib, e, b"R must be at least 1", R=0)
    for N in (0, 257):
        _refused(lib, e, b"N must be in [1, 256]", N=N)
    _refused(lib, e, b"CN_MAX_SAMPLES", R=(1 << 28) // 256 + 1, N=256)
    _refused(lib, e, b"z_stride must be 0 or N", z_stride=7)
    for G in (16, 48, 288):
        _refused(lib, e, b"G must be a multiple of 32 in [32, 256]", G=G)
    for ic in (0.0, -1.0, NAN, INF):
        _refused(lib, e, b"inv_cell must be finite and positive", inv_cell=ic)
    for lo in ((NAN, 0, 0), (0, INF, 0), (0, 0, -INF)):
        _refused(lib, e, b"lo must be finite", lo=lo)


def test_sparse_gather_and_scatter_refusals():
    _, lib = _lib()
    e = "cn_sparse_gather"
    for k in ("ro", "keep", "offset", "xyz"):
        _refused(lib, e, b"NULL argument", **{k: None})
    _refused(lib, e, b"R must be at least 1", R=0)
    for N in (0, 257):
        _refused(lib, e, b"N must be in [1, 256]", N=N)
    _refused(lib, e, b"CN_MAX_SAMPLES", R=(1 << 28) // 256 + 1, N=256)
    _refused(lib, e, b"z_stride must be 0 or N", z_stride=63)
    e = "cn_sparse_scatter"
    for k in ("keep", "sigma_k", "rgb"):
        _refused(lib, e, b"NULL argument", **{k: None})
    _refused(lib, e, b"R must be at least 1", R=-1)
    for N in (0, 257):
        _refused(lib, e, b"N must be in [1, 256]", N=N)
    _refused(lib, e, b"CN_MAX_SAMPLES", R=(1 << 28) // 256 + 1, N=256)


def test_optimize_flags_parse_and_default_off():
    import optimize
    a = optimize.build_parser().parse_args([])
    assert a.sparse_eval is False
    assert a.occ_grid is None and a.occ_tau is None and a.occ_dilate is None and a.occ_bound is None
    a = optimize.build_parser().parse_args(["--sparse_eval", "True", "--occ_grid", "64", "--occ_tau", "0.1",
                                            "--occ_dilate", "2", "--occ_bound", "0.6"])
    assert a.sparse_eval is True and a.occ_grid == 64 and a.occ_dilate == 2
    assert a.occ_tau == 0.1 and a.occ_bound == 0.6
    for bad in (["--occ_grid", "big"], ["--occ_tau", "x"], ["--occ_dilate", "1.5"]):
        with pytest.raises(SystemExit):
            optimize.build_parser().parse_args(bad)
    for flag in ("--sparse_eval", "--occ_grid", "--occ_tau", "--occ_dilate", "--occ_bound"):
        assert flag in optimize.__doc__


@pytest.mark.parametrize("kw", [dict(occ_tau=-1.0), dict(occ_tau=NAN), dict(occ_dilate=-1), dict(occ_dilate=5),
                                dict(occ_grid=48), dict(occ_bound=0.0)])
def test_optimizer_rejects_bad_grid_arguments(kw):
    """Refused before the device, the model or the data is touched."""
    from codenerf_amd.optimizer import Optimizer
    with pytest.raises(ValueError, match="occ_"):
        Optimizer("nowhere", hpams={"N_importance": 0}, sparse_eval=True, **kw)


def test_occupancy_grid_geometry_needs_no_device():
    import numpy as np
    import torch
    from codenerf_amd.occupancy import OccupancyGrid
    bits = torch.zeros(32 ** 3 // 32, dtype=torch.int32)
    bits[5] = 0x0F
    g = OccupancyGrid(bits, 32, (0.1, 0.0, -0.05), 0.5)
    assert g.lo == tuple(float(np.float32(c) - np.float32(0.5)) for c in (0.1, 0.0, -0.05))
    assert g.inv_cell == 32.0 and g.fraction() == 4 / 32 ** 3
    c = OccupancyGrid.cell_centers(32, (0, 0, 0), 0.5)
    assert tuple(c.shape) == (32 ** 3, 3)
    assert torch.equal(c[1], torch.tensor([-0.5 + 0.5 / 32, -0.5 + 0.5 / 32, -0.5 + 1.5 / 32]))
    for bad in (dict(G=48), dict(bound=0.0)):
        with pytest.raises(ValueError):
            OccupancyGrid(bits, **{**dict(G=32, bound=0.5), **bad})
