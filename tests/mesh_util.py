"""Numpy restatement of the iso-surface definition (include/codenerf.h,
DESIGN.md 8.5): marching tetrahedra on the Kuhn triangulation (test
infrastructure).  It is written from the rule, with coordinates instead of the
offset codes of csrc/mesh_tables.h, and is the definition the kernels are held
to bit for bit.  Everything is float32 with one rounding per operation."""
import itertools

import numpy as np

F = np.float32
POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)
# edge k of a lattice point: m = k + 1, offset ((m >> 2) & 1, (m >> 1) & 1, m & 1)
EDGE = np.array([(((k + 1) >> 2) & 1, ((k + 1) >> 1) & 1, (k + 1) & 1) for k in range(7)], dtype=np.int64)
_EDGE_K = {tuple(e): k for k, e in enumerate(EDGE.tolist())}


def tets():
    """Local vertices (4, 3) of the 6 tetrahedra of the unit cube, one per axis
    permutation in lexicographic order."""
    out = []
    for perm in itertools.permutations(range(3)):
        v = np.zeros((4, 3), dtype=np.int64)
        v[1, perm[0]] = 1
        v[2] = v[1]
        v[2, perm[1]] = 1
        v[3] = 1
        out.append(v)
    return out


def tet_triangles(v, mask):
    """Triangles of one tetrahedron (vertices v) under an inside mask: lists of
    three (owner corner (3,), edge k), oriented from inside to outside."""
    ins = [i for i in range(4) if (mask >> i) & 1]
    out = [i for i in range(4) if not (mask >> i) & 1]
    e = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tris = [[e(ins[0], o) for o in out]]
    elif len(ins) == 3:
        tris = [[e(i, out[0]) for i in ins]]
    else:
        (a, b), (c, d) = ins, out
        tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    vf = v.astype(np.float64)
    g = vf[out].mean(0) - vf[ins].mean(0)
    res = []
    for tri in tris:
        q = [(vf[i] + vf[j]) / 2 for i, j in tri]
        dot = float(np.dot(np.cross(q[1] - q[0], q[2] - q[0]), g))
        assert abs(dot) > 1e-9
        if dot < 0:
            tri = [tri[0], tri[2], tri[1]]
        res.append([(v[i], _EDGE_K[tuple((v[j] - v[i]).tolist())]) for i, j in tri])
    return res


def rule_table():
    """[6][16] -> list of triangles of (owner offset (3,), k): the table the rule gives."""
    return [[tet_triangles(v, mask) for mask in range(16)] for v in tets()]


def _lookup():
    """Dense arrays of rule_table(): count [6,16], owner offsets [6,16,2,3,3], k [6,16,2,3]."""
    n = np.zeros((6, 16), dtype=np.int64)
    off = np.zeros((6, 16, 2, 3, 3), dtype=np.int64)
    kk = np.zeros((6, 16, 2, 3), dtype=np.int64)
    for t, row in enumerate(rule_table()):
        for mask, tris in enumerate(row):
            n[t, mask] = len(tris)
            for j, tri in enumerate(tris):
                for i, (o, k) in enumerate(tri):
                    off[t, mask, j, i] = o
                    kk[t, mask, j, i] = k
    return n, off, kk


_N, _OFF, _K = _lookup()
_TETS = np.stack(tets())                    # [6, 4, 3]


def axis_positions(n, lo, s):
    """p = lo + float(i) s, separately rounded."""
    return (F(lo) + (np.arange(n).astype(F) * F(s)).astype(F)).astype(F)


def marching_tets(field, iso, lo=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """field (nx, ny, nz) float32 -> dict(vflags uint8 [P], vcount int32 [P],
    tcount int32 [P], verts float32 [Nv, 3], tris int32 [Nt, 3])."""
    field = np.ascontiguousarray(field, dtype=F)
    nx, ny, nz = dims = field.shape
    iso = F(iso)
    with np.errstate(invalid="ignore"):
        inside = ~(field < iso)
    P = field.size
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    idx = np.stack([ix, iy, iz], -1).reshape(P, 3)
    lin = lambda p: (p[..., 0] * ny + p[..., 1]) * nz + p[..., 2]
    fin, ffl = inside.reshape(-1), field.reshape(-1)
    in_lattice = lambda p: (p < np.array(dims)).all(-1)

    vflags = np.zeros(P, dtype=np.uint8)
    for k in range(7):
        q = idx + EDGE[k]
        ok = in_lattice(q)
        cross = np.zeros(P, dtype=bool)
        cross[ok] = fin[ok] != fin[lin(q[ok])]
        vflags |= (cross.astype(np.uint8) << k).astype(np.uint8)
    vcount = POP[vflags]
    voff = np.cumsum(vcount) - vcount

    pos = [axis_positions(n, l, s) for n, l, s in zip(dims, lo, spacing)]
    verts = np.zeros((int(vcount.sum()), 3), dtype=F)
    for k in range(7):
        own = np.nonzero((vflags >> k) & 1)[0]
        a, b = idx[own], idx[own] + EDGE[k]
        sa, sb = ffl[own], ffl[lin(b)]
        with np.errstate(all="ignore"):
            t = ((iso - sa).astype(F) / (sb - sa).astype(F)).astype(F)
        t = np.where(np.isnan(t), F(0.5), np.where(t < 0, F(0), np.where(t > 1, F(1), t))).astype(F)
        row = voff[own] + POP[vflags[own] & ((1 << k) - 1)]
        for ax in range(3):
            pa, pb = pos[ax][a[:, ax]], pos[ax][b[:, ax]]
            verts[row, ax] = (pa + (t * (pb - pa).astype(F)).astype(F)).astype(F)

    cube = (idx < np.array(dims) - 1).all(-1)
    cubes = np.nonzero(cube)[0]
    base = idx[cubes]                                                     # [C, 3]
    corner_in = fin[lin(base[:, None, None, :] + _TETS[None])]            # [C, 6, 4]
    mask = (corner_in.astype(np.int64) << np.arange(4)).sum(-1)           # [C, 6]
    t6 = np.arange(6)[None, :]
    ntri = _N[t6, mask]                                                   # [C, 6]
    tcount = np.zeros(P, dtype=np.int32)
    tcount[cubes] = ntri.sum(1)
    owner = lin(base[:, None, None, None, :] + _OFF[t6, mask])            # [C, 6, 2, 3]
    k = _K[t6, mask]
    vid = voff[owner] + POP[vflags[owner] & ((1 << k) - 1)]
    valid = np.arange(2)[None, None, :] < ntri[..., None]                 # [C, 6, 2]
    tris = vid[valid].astype(np.int32).reshape(-1, 3)                     # cube, tetrahedron, table order
    assert tris.shape[0] == int(tcount.sum())
    return dict(vflags=vflags, vcount=vcount.astype(np.int32), tcount=tcount, verts=verts, tris=tris)


# ------------------------------------------------------------------ properties
def directed_edges(tris):
    t = np.asarray(tris, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented(tris):
    """Every directed edge occurs once and its reverse once."""
    e = directed_edges(tris)
    if len(e) == 0:
        return True
    n = int(e.max()) + 1
    key, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    u, c = np.unique(key, return_counts=True)
    return bool((c == 1).all()) and np.array_equal(u, np.unique(rev))


def euler(nv, tris):
    e = directed_edges(tris)
    und = np.unique(np.sort(e, axis=1), axis=0)
    return nv - len(und) + len(tris)


def signed_volume(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


# ------------------------------------------------------------------ fields
def axes(dims):
    return [np.linspace(-1.0, 1.0, n).astype(F) for n in dims]


def lattice_geometry(dims):
    """lo, spacing of the [-1, 1] lattice the analytic fields are sampled on."""
    return (-1.0,) * 3, tuple(float(F(2.0 / (n - 1))) for n in dims)


def sphere(dims, r2=0.49):
    x, y, z = np.meshgrid(*[a.astype(np.float64) for a in axes(dims)], indexing="ij")
    return (r2 - (x * x + y * y + z * z)).astype(F)


def torus(dims):
    x, y, z = np.meshgrid(*[a.astype(np.float64) for a in axes(dims)], indexing="ij")
    return (0.0625 - ((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z)).astype(F)


def rounded_random(dims=(6, 7, 5), seed=0):
    """Integers, so that many values equal iso = 0; the boundary layer outside."""
    f = np.rint(np.random.default_rng(seed).standard_normal(dims)).astype(F)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (F(-1),) * 6
    return f
