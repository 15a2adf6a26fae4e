"""Coloured triangle mesh of one object's density field (no reference
counterpart).

``marching_tets`` is the iso-surface of a lattice of densities: marching
tetrahedra on the Kuhn triangulation (cn_mesh_count -> the caller's prefix
sums -> cn_mesh_emit; include/codenerf.h has the definition).  ``extract_mesh``
evaluates the model's own plan on an n^3 lattice, takes the surface at ``iso``,
and gives every vertex the normal -grad(sigma) / |grad(sigma)| (the input
gradient kernels) and the colour the texture code gives a camera looking
straight at the surface.  ``write_ply`` / ``read_ply`` store it as binary
little-endian PLY.
"""
import collections

import numpy as np
import torch

from . import engine as _eng
from .occupancy import CHUNK, eval_density

Mesh = collections.namedtuple("Mesh", "verts tris normals colors")


def marching_tets(field, dims, iso, lo, spacing):
    """Iso-surface of ``field`` (any float32 device tensor of nx ny nz values
    in lattice order) at ``iso``; lattice point i sits at lo + i spacing per
    axis.  -> (verts (Nv, 3) float32, tris (Nt, 3) int32).  One read-back (the
    two totals); an empty surface launches no emit."""
    if field.dtype != torch.float32:
        raise ValueError("marching_tets: field must be float32")
    field = field.contiguous().reshape(-1)
    vflags, vcount, tcount = _eng.mesh_count(field, dims, iso)
    vsum = torch.cumsum(vcount, 0, dtype=torch.int32)
    tsum = torch.cumsum(tcount, 0, dtype=torch.int32)
    Nv, Nt = (int(x) for x in torch.stack([vsum[-1], tsum[-1]]).cpu())
    if Nt == 0:
        return (torch.empty(0, 3, dtype=torch.float32, device=field.device),
                torch.empty(0, 3, dtype=torch.int32, device=field.device))
    return _eng.mesh_emit(field, dims, iso, lo, spacing, vflags, vsum - vcount, tsum - tcount, Nv, Nt)


def lattice_geometry(n, bound, center=(0.0, 0.0, 0.0)):
    """lo (3 floats) and the spacing of the n^3 lattice over [center - bound,
    center + bound]^3: lo = center - bound in float32, s = float32(2 bound / (n - 1))."""
    lo = tuple(float(np.float32(c) - np.float32(bound)) for c in center)
    return lo, float(np.float32(2.0 * bound / (n - 1)))


def lattice_points(n, lo, s, a=0, b=None, device=None):
    """Points [a, b) of the lattice in lattice order, float32 (b - a, 3):
    lo + float(i) s per axis, separately rounded -- the kernel's formula."""
    b = n ** 3 if b is None else b
    c = torch.arange(a, b, dtype=torch.int64, device=device)
    idx = torch.stack([c // (n * n), (c // n) % n, c % n], dim=1).to(torch.float32)
    return torch.tensor(lo, dtype=torch.float32, device=device) + idx * s


def unit_normals(dxyz):
    """-dxyz / |dxyz| per row; (0, 0, 0) where the gradient is zero (or NaN)."""
    x, y, z = dxyz[:, 0], dxyz[:, 1], dxyz[:, 2]
    nrm = (x * x + y * y + z * z).sqrt()
    return torch.where((nrm > 0)[:, None], -dxyz / nrm[:, None], torch.zeros_like(dxyz))


def vertex_normals(eng, blob, verts):
    """Unit normals at explicit points: the codes forward, the pose backward
    with dsigma = 1 and drgb = 0, the input gradient (= grad sigma), in
    chunks whose workspace fits engine.ACT_BUDGET."""
    dev = eng.device
    Nv = verts.shape[0]
    out = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    step = min(eng.max_act_samples(), CHUNK)
    for a in range(0, Nv, step):
        M = min(step, Nv - a)
        Mp = eng.pad(M)
        x = verts[a:a + M].contiguous()
        vd = torch.zeros(M, 3, dtype=torch.float32, device=dev)
        vd[:, 2] = 1.0
        act = eng.new_act(M)
        eng.mlp_fwd(blob, M, xyz=x, viewdir=vd, act=act, codes=True)
        eng.mlp_bwd(blob, M, torch.ones(Mp, dtype=torch.float32, device=dev),
                    torch.zeros(Mp, 3, dtype=torch.float32, device=dev), act, pose=True)
        dxyz, _, _, _ = eng.mlp_input_grad(act, M, xyz=x, viewdir=vd)
        out[a:a + M] = unit_normals(dxyz[:M])
    return out


def vertex_colors(eng, blob, verts, normals=None):
    """rgb at explicit points seen along -normal ((0, 0, 1) where the normal is
    zero or there are none)."""
    dev = eng.device
    Nv = verts.shape[0]
    vd = torch.zeros(Nv, 3, dtype=torch.float32, device=dev)
    vd[:, 2] = 1.0
    if normals is not None:
        vd = torch.where((normals != 0).any(1, keepdim=True), -normals, vd)
    out = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    for a in range(0, Nv, CHUNK):
        M = min(CHUNK, Nv - a)
        _, rgb = eng.mlp_fwd(blob, M, xyz=verts[a:a + M].contiguous(), viewdir=vd[a:a + M].contiguous())
        out[a:a + M] = rgb[:M]
    return out


def extract_mesh(model, shape_code, texture_code, n=128, bound=0.5, center=(0.0, 0.0, 0.0), *, iso, normals=True,
                 colors=True):
    """The surface sigma = ``iso`` of ``model`` under the two codes, on the n^3
    lattice over [center - bound, center + bound]^3 -> Mesh(verts, tris,
    normals or None, colors or None), device tensors.  ``iso`` has no default:
    no value has been measured on a real model."""
    n = int(n)
    if not 2 <= n <= 512:
        raise ValueError(f"n must be in [2, 512], got {n}")
    if not bound > 0:
        raise ValueError(f"bound must be positive, got {bound}")
    iso = float(iso)
    if iso != iso:
        raise ValueError("iso is NaN")
    eng = model.engine()
    params = model.param_list()
    dev = eng.device
    with torch.no_grad():
        eng.ensure_packed(params, bwd=bool(normals))
        code = lambda c: c.detach().reshape(-1).to(dev, torch.float32).contiguous()
        blob, _ = eng.latent_fwd(params, code(shape_code), code(texture_code))
        lo, s = lattice_geometry(n, bound, center)
        field = eval_density(eng, blob, n ** 3, lambda a, b: lattice_points(n, lo, s, a, b, dev))
        verts, tris = marching_tets(field, (n, n, n), iso, lo, (s, s, s))
        nrm = col = None
        if verts.shape[0]:
            if normals:
                nrm = vertex_normals(eng, blob, verts)
            if colors:
                col = vertex_colors(eng, blob, verts, nrm)
        else:
            empty = torch.empty(0, 3, dtype=torch.float32, device=dev)
            nrm, col = (empty if normals else None), (empty if colors else None)
    return Mesh(verts, tris, nrm, col)


# ---------------------------------------------------------------- PLY
def colors_to_uint8(colors):
    c = np.asarray(colors)
    if c.dtype == np.uint8:
        return c
    return np.floor(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _vertex_dtype(normals, colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)


_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_PLY_TYPES = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}


def write_ply(path, verts, tris, normals=None, colors=None):
    """Binary little-endian PLY: float32 positions (and normals), uint8 colours
    (floats are clipped to [0, 1] and rounded to the nearest of 255 steps),
    faces as uchar-counted int32 lists."""
    verts, tris = _host(verts).astype("<f4").reshape(-1, 3), _host(tris).astype("<i4").reshape(-1, 3)
    vt = _vertex_dtype(normals is not None, colors is not None)
    v = np.empty(len(verts), dtype=vt)
    v["x"], v["y"], v["z"] = verts.T
    if normals is not None:
        v["nx"], v["ny"], v["nz"] = _host(normals).astype("<f4").reshape(-1, 3).T
    if colors is not None:
        v["red"], v["green"], v["blue"] = colors_to_uint8(_host(colors)).reshape(-1, 3).T
    f = np.empty(len(tris), dtype=_FACE)
    f["n"], f["v"] = 3, tris
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {_PLY_TYPES[vt[name].str]} {name}" for name in vt.names]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())


def read_ply(path):
    """What write_ply wrote -> (verts (Nv, 3) float32, tris (Nt, 3) int32,
    normals (Nv, 3) float32 or None, colors (Nv, 3) uint8 or None)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    names = [ln.split()[2] for ln in lines if ln.startswith("property") and "list" not in ln]
    vt = _vertex_dtype("nx" in names, "red" in names)
    if list(vt.names) != names:
        raise ValueError(f"{path}: unexpected vertex properties {names}")
    v = np.frombuffer(data, dtype=vt, count=nv, offset=end)
    f = np.frombuffer(data, dtype=_FACE, count=nf, offset=end + nv * vt.itemsize)
    if nf and not (f["n"] == 3).all():
        raise ValueError(f"{path}: faces must be triangles")
    col = lambda *k: np.stack([v[x] for x in k], axis=1)
    return (col("x", "y", "z"), f["v"].astype(np.int32).reshape(-1, 3),
            col("nx", "ny", "nz") if "nx" in names else None,
            col("red", "green", "blue") if "red" in names else None)
