"""Numpy restatement of the occupancy-grid entries (include/codenerf.h, DESIGN.md
8.4) and the test scene they share (test infrastructure).  Everything is
float32 with one rounding per operation, in the order the definition gives."""
import numpy as np
import torch

from oracle import ref_cpu
from oracle.params import look_at_pose

F = np.float32
NEAR, FAR = 0.8, 1.8


def rays(H, W=None):
    """The scene's camera: look_at_pose(1.3, 35, 20), focal 131.25 at 128 px."""
    W = H if W is None else W
    ro, vd = ref_cpu.get_rays(H, W, 131.25 * 16 / 128, look_at_pose(1.3, 35, 20))
    return ro.contiguous().numpy().astype(F), vd.contiguous().numpy().astype(F)


def midpoints(N):
    """Stratified midpoints of [NEAR, FAR] (ref_cpu.stratified_z without jitter)."""
    half = (FAR - NEAR) / (2 * N)
    return torch.linspace(NEAR + half, FAR - half, N).numpy().astype(F)


def grid_geometry(G, center, bound):
    lo = np.array([F(c) - F(bound) for c in center], dtype=F)
    return lo, F(G / (2.0 * bound))


def ball_bits(G=32, bound=0.5, center=(0.1, 0.0, -0.05), radius=0.35):
    """Cells of the box [-bound, bound]^3 whose centre lies within `radius` of `center` -> words."""
    c = (np.arange(G) + 0.5) * (2.0 * bound / G) - bound
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    occ = (x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2 <= radius ** 2
    return pack_cells(occ)


def pack_cells(occ):
    """bool (G, G, G) -> uint32 words: cell c = (ix G + iy) G + iz is bit c & 31 of word c >> 5."""
    b = occ.reshape(-1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def unpack_cells(words, G):
    w = np.asarray(words).view(np.uint32).reshape(-1, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(G, G, G)


def build_bits(sigma, G, tau, dilate):
    """cn_occupancy_build: sigma >= tau (NaN occupied), OR over the Chebyshev ball, clamped."""
    occ = ~(sigma.reshape(G, G, G).astype(F) < F(tau))
    out = np.zeros_like(occ)
    d = int(dilate)
    pad = np.zeros((G + 2 * d,) * 3, dtype=bool)
    pad[d:d + G, d:d + G, d:d + G] = occ
    for dx in range(2 * d + 1):
        for dy in range(2 * d + 1):
            for dz in range(2 * d + 1):
                out |= pad[dx:dx + G, dy:dy + G, dz:dz + G]
    return pack_cells(out)


def points(ro, rd, z):
    """x = o + d z, one rounding per operation -> (R, N, 3) float32."""
    z = np.asarray(z, dtype=F)
    zz = (z[None, :] if z.ndim == 1 else z)[:, :, None]
    return (ro[:, None, :] + (rd[:, None, :] * zz).astype(F)).astype(F)


def keep_mask(ro, rd, z, words, G, lo, inv_cell, keep_last):
    """The keep rule -> bool (R, N)."""
    x = points(ro, rd, z)
    with np.errstate(invalid="ignore"):
        t = ((x - lo.astype(F)).astype(F) * F(inv_cell)).astype(F)
        inside = ((t >= 0) & (t < F(G))).all(-1)
    i = np.floor(np.where(inside[..., None], t, 0)).astype(np.int64)
    c = (i[..., 0] * G + i[..., 1]) * G + i[..., 2]
    w = np.asarray(words).view(np.uint32)
    keep = inside & (((w[c >> 5] >> (c & 31).astype(np.uint32)) & 1) == 1)
    if keep_last:
        keep[:, -1] = True
    return keep


def pack_keep(keep):
    """bool (R, N) -> (keep words (R, 8) uint32, counts (R,) int32)."""
    R, N = keep.shape
    full = np.zeros((R, 256), dtype=np.uint64)
    full[:, :N] = keep
    words = (full.reshape(R, 8, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return words, keep.sum(1).astype(np.int32)
