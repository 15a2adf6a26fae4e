"""CPU: the numpy restatement of the iso-surface definition (tests/mesh_util.py,
DESIGN.md 8.5) on analytic fields, so that the definition the kernels are held
to is itself checked: the surface is closed and consistently oriented, has the
genus of the shape, encloses a positive volume, and has the vertex and triangle
counts a prototype of the rule measured.

Fields: float32 of float64 linspace(-1, 1, n) per axis, iso = 0; the sphere
0.49 - |x|^2, the torus 0.0625 - ((sqrt(x^2 + y^2) - 0.6)^2 + z^2)."""
import numpy as np
import pytest

import mesh_util as U

CASES = [("sphere", (5, 5, 5), 74, 144, 2), ("sphere", (9, 9, 9), 386, 768, 2), ("sphere", (7, 9, 12), 466, 928, 2),
         ("sphere", (17, 17, 17), 1730, 3456, 2), ("torus", (17, 17, 9), 1116, 2232, 0)]


@pytest.mark.parametrize("name,dims,nv,nt,chi", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in CASES])
def test_analytic_surface(name, dims, nv, nt, chi):
    field = getattr(U, name)(dims)
    lo, s = U.lattice_geometry(dims)
    m = U.marching_tets(field, 0.0, lo, s)
    verts, tris = m["verts"], m["tris"]
    vol = U.signed_volume(verts, tris)
    print(f"{name} {dims}: {len(verts)} vertices, {len(tris)} triangles, volume {vol:.4f}")
    assert (len(verts), len(tris)) == (nv, nt)
    assert int(m["vcount"].sum()) == nv and int(m["tcount"].sum()) == nt and m["tcount"].max() <= 12
    assert np.array_equal(m["vcount"], U.POP[m["vflags"]])
    assert sorted(np.unique(tris).tolist()) == list(range(nv))          # every vertex is used
    assert U.is_closed_oriented(tris)
    assert U.euler(nv, tris) == chi
    assert vol > 0
    assert np.isfinite(verts).all() and (np.abs(verts) <= 1).all()


def test_vertices_lie_on_their_edges():
    """A crossing's vertex is between its edge's ends, at the linear zero of the field."""
    dims = (7, 9, 12)
    lo, s = U.lattice_geometry(dims)
    m = U.marching_tets(U.sphere(dims), 0.0, lo, s)
    r = np.linalg.norm(m["verts"].astype(np.float64), axis=1)
    # linear interpolation of a concave field along an edge lands inside the sphere, within one cell of it
    assert (r <= 0.7 + 1e-6).all() and (r > 0.7 - max(s) * np.sqrt(3)).all()


def test_values_equal_to_iso_keep_the_surface_closed():
    f = U.rounded_random()
    assert (f == 0).sum() > 20
    m = U.marching_tets(f, 0.0)
    assert (len(m["verts"]), len(m["tris"])) == (338, 676)
    assert U.is_closed_oriented(m["tris"])
    assert np.isfinite(m["verts"]).all()


def test_nan_and_inf_are_inside_and_give_finite_vertices():
    f = np.full((4, 4, 4), -1.0, dtype=np.float32)
    f[1, 1, 1], f[2, 2, 2], f[1, 2, 1] = np.nan, np.inf, 0.0
    m = U.marching_tets(f, 0.0)
    assert U.is_closed_oriented(m["tris"]) and len(m["tris"]) > 0
    assert np.isfinite(m["verts"]).all()


def test_empty_and_full_fields_have_no_surface():
    for v in (-1.0, 1.0):
        m = U.marching_tets(np.full((3, 4, 5), v, dtype=np.float32), 0.0)
        assert len(m["verts"]) == 0 and len(m["tris"]) == 0 and not m["vflags"].any()
