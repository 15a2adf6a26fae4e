"""CPU: the C ABI of mesh extraction (cn_mesh_count, cn_mesh_emit): exported,
bound, additive to ABI 4, and every host check refuses with -1 and a message
naming the entry before anything is launched (the pointers below are never
dereferenced); the generated triangle table; the PLY round trip; the
optimize.py flags and the Optimizer's argument checks."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cn_mesh_count", "cn_mesh_emit")
NAN, INF = float("nan"), float("inf")


def _lib():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load_library()


def test_the_two_symbols_are_exported_and_bound():
    L, lib = _lib()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {"cn_mesh_count": [P, I, I, I, F, P, P, P, P],
            "cn_mesh_emit": [P, I, I, I, F, F, F, F, F, F, F, P, P, P, P, P, P]}
    for name in ENTRIES:
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L._SIGS[name][1] == want[name]
    assert L.ABI_VERSION == 4 and lib.cn_abi_version() == 4
    from codenerf_amd import engine
    assert callable(engine.mesh_count) and callable(engine.mesh_emit)


D = ctypes.c_void_p(256)


def _count(lib, field=D, dims=(4, 5, 6), iso=0.5, vflags=D, vcount=D, tcount=D):
    return lib.cn_mesh_count(field, *dims, iso, vflags, vcount, tcount, None)


def _emit(lib, field=D, dims=(4, 5, 6), iso=0.5, lo=(-0.5, -0.5, -0.5), s=(0.1, 0.2, 0.3), vflags=D, voff=D, toff=D,
          vert=D, tri=D):
    return lib.cn_mesh_emit(field, *dims, iso, *lo, *s, vflags, voff, toff, vert, tri, None)


CALLS = dict(zip(ENTRIES, (_count, _emit)))
BAD_DIMS = [(1, 5, 6), (4, 0, 6), (4, 5, -3), (1025, 5, 6), (4, 1025, 6), (4, 5, 1025)]


def _refused(lib, entry, what, **kw):
    assert CALLS[entry](lib, **kw) == -1, (entry, kw)
    err = lib.cn_last_error()
    assert entry.encode() + b":" in err and what in err, err


def test_mesh_count_refusals():
    _, lib = _lib()
    e = "cn_mesh_count"
    for k in ("field", "vflags", "vcount", "tcount"):
        _refused(lib, e, b"NULL argument", **{k: None})
    for dims in BAD_DIMS:
        _refused(lib, e, b"every dimension must be in [2, 1024]", dims=dims)
    _refused(lib, e, b"exceeds 2^27 lattice points", dims=(1024, 1024, 129))
    _refused(lib, e, b"exceeds 2^27 lattice points", dims=(513, 512, 512))
    _refused(lib, e, b"iso is NaN", iso=NAN)


def test_mesh_emit_refusals():
    _, lib = _lib()
    e = "cn_mesh_emit"
    for k in ("field", "vflags", "voff", "toff", "vert", "tri"):
        _refused(lib, e, b"NULL argument", **{k: None})
    for dims in BAD_DIMS:
        _refused(lib, e, b"every dimension must be in [2, 1024]", dims=dims)
    _refused(lib, e, b"exceeds 2^27 lattice points", dims=(1024, 1024, 129))
    _refused(lib, e, b"iso is NaN", iso=NAN)
    for bad in (0.0, -0.1, NAN, INF):
        for a in range(3):
            s = [0.1, 0.2, 0.3]
            s[a] = bad
            _refused(lib, e, b"spacing must be finite and positive", s=tuple(s))
    for lo in ((NAN, 0, 0), (0, INF, 0), (0, 0, -INF)):
        _refused(lib, e, b"lo must be finite", lo=lo)


def test_generated_table_is_the_committed_header_and_the_rule():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_mesh_tables as G
    import mesh_util as U
    assert open(G.HEADER).read() == G.render()
    # the header's entries decode to the table the restatement derives from the rule with coordinates
    table, rule = G.build_table(), U.rule_table()
    assert len(table) == 96
    for t in range(6):
        for mask in range(16):
            word, tris = table[t * 16 + mask], rule[t][mask]
            assert word & 3 == len(tris) == (0, 1, 2, 1, 0)[bin(mask).count("1")]
            corners = [(o, k) for tri in tris for o, k in tri]
            for j, (o, k) in enumerate(corners):
                ck = (word >> (2 + 6 * j)) & 63
                assert (ck & 7, ck >> 3) == (k, int(o[0]) * 4 + int(o[1]) * 2 + int(o[2]))
            assert word >> (2 + 6 * len(corners)) == 0


def test_ply_round_trip_is_exact(tmp_path):
    from codenerf_amd.mesh import colors_to_uint8, read_ply, write_ply
    rng = np.random.default_rng(1)
    v = rng.standard_normal((11, 3)).astype(np.float32)
    v[0] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]
    t = rng.integers(0, 11, (7, 3)).astype(np.int32)
    n = rng.standard_normal((11, 3)).astype(np.float32)
    c = rng.random((11, 3)).astype(np.float32)
    c[1] = [-0.5, 1.5, 0.5]
    for normals, colors in ((None, None), (n, None), (None, c), (n, c)):
        p = str(tmp_path / "m.ply")
        write_ply(p, v, t, normals, colors)
        rv, rt, rn, rc = read_ply(p)
        assert rv.dtype == np.float32 and rt.dtype == np.int32
        assert rv.tobytes() == v.tobytes() and np.array_equal(rt, t)
        assert (rn is None) == (normals is None) and (rc is None) == (colors is None)
        if normals is not None:
            assert rn.tobytes() == n.tobytes()
        if colors is not None:
            assert rc.dtype == np.uint8 and np.array_equal(rc, colors_to_uint8(c))
            assert rc[1].tolist() == [0, 255, 128]
    head = open(p, "rb").read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 11\n")
    # an empty mesh and torch tensors
    import torch
    write_ply(p, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3))
    rv, rt, rn, rc = read_ply(p)
    assert rv.shape == (0, 3) and rt.shape == (0, 3) and rn.shape == (0, 3) and rc.shape == (0, 3)


def test_optimize_flags_parse_and_default_off():
    import optimize
    a = optimize.build_parser().parse_args([])
    assert a.save_mesh is False and a.mesh_grid is None and a.mesh_iso is None and a.mesh_bound is None
    a = optimize.build_parser().parse_args(["--save_mesh", "True", "--mesh_grid", "64", "--mesh_iso", "12.5",
                                            "--mesh_bound", "0.6"])
    assert a.save_mesh is True and a.mesh_grid == 64 and a.mesh_iso == 12.5 and a.mesh_bound == 0.6
    for bad in (["--mesh_grid", "big"], ["--mesh_iso", "x"], ["--mesh_grid", "1.5"]):
        with pytest.raises(SystemExit):
            optimize.build_parser().parse_args(bad)
    for flag in ("--save_mesh", "--mesh_grid", "--mesh_iso", "--mesh_bound"):
        assert flag in optimize.__doc__


@pytest.mark.parametrize("kw", [dict(), dict(mesh_iso=NAN), dict(mesh_iso=INF), dict(mesh_iso=1.0, mesh_grid=1),
                                dict(mesh_iso=1.0, mesh_grid=513), dict(mesh_iso=1.0, mesh_bound=0.0),
                                dict(mesh_iso=1.0, mesh_bound=-1.0)])
def test_optimizer_rejects_bad_mesh_arguments(kw):
    """Refused before the device, the model or the data is touched."""
    from codenerf_amd.optimizer import Optimizer
    with pytest.raises(ValueError, match="mesh_"):
        Optimizer("nowhere", hpams={"N_importance": 0}, save_mesh=True, **kw)
