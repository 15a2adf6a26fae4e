"""Occupancy grid of one object's density field (no reference counterpart;
DESIGN.md 8.4).

With the codes fixed -- every evaluation and novel-view render -- the density
is a fixed function of space, so one grid per object tells every later view
which samples lie in empty space.  ``ImageStep.render[_fine](occupancy=grid)``
evaluates the MLP at the samples in set cells only (and at the last coarse
sample of every ray); the density and colour of every other sample are 0.

The grid is G^3 cells over the box [center - bound, center + bound)^3, one bit
per cell in the order of include/codenerf.h: cell (ix, iy, iz) is bit c & 31
of word c >> 5, c = (ix G + iy) G + iz.
"""
import numpy as np
import torch

from . import engine as _eng

CHUNK = 1 << 20          # points per MLP launch of build()


def eval_density(eng, blob, total, points):
    """Density (total,) of the engine's plan at the points ``points(a, b)`` ->
    float32 (b - a, 3) of rows [a, b): explicit points, at most CHUNK per
    launch, view direction (0, 0, 1) (it does not enter the density).  Shared
    by OccupancyGrid.build and mesh.extract_mesh."""
    dev = eng.device
    sigma = torch.empty(total, dtype=torch.float32, device=dev)
    n = min(CHUNK, total)
    vd = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    vd[:, 2] = 1.0
    for a in range(0, total, CHUNK):
        b = min(a + CHUNK, total)
        sg, _ = eng.mlp_fwd(blob, b - a, xyz=points(a, b), viewdir=vd)
        sigma[a:b] = sg[:b - a]
    return sigma


class OccupancyGrid:
    def __init__(self, bits, G, center=(0.0, 0.0, 0.0), bound=0.5):
        G = int(G)
        if G % 32 or not 32 <= G <= 256:
            raise ValueError(f"G must be a multiple of 32 in [32, 256], got {G}")
        if not bound > 0:
            raise ValueError(f"bound must be positive, got {bound}")
        if bits.dtype != torch.int32 or bits.numel() != G ** 3 // 32 or not bits.is_contiguous():
            raise ValueError(f"bits must be {G ** 3 // 32} contiguous int32 words")
        self.bits = bits
        self.G = G
        self.center = tuple(float(c) for c in center)
        self.bound = float(bound)
        self.lo = tuple(float(np.float32(c) - np.float32(bound)) for c in self.center)
        self.inv_cell = float(np.float32(G / (2.0 * self.bound)))

    def fraction(self):
        """Share of set cells."""
        words = self.bits.cpu().numpy().view(np.uint8)
        return float(np.unpackbits(words).sum()) / self.G ** 3

    @staticmethod
    def cell_centers(G, center, bound, a=0, b=None, device=None):
        """Centres of cells [a, b) of a G^3 grid in cell order, float32 (n, 3):
        lo + (i + 0.5) * cell per axis, cell = float32(2 bound / G)."""
        b = G ** 3 if b is None else b
        c = torch.arange(a, b, dtype=torch.int64, device=device)
        idx = torch.stack([c // (G * G), (c // G) % G, c % G], dim=1).to(torch.float32)
        lo = torch.tensor([np.float32(x) - np.float32(bound) for x in center], dtype=torch.float32, device=device)
        cell = float(np.float32(2.0 * bound / G))
        return lo + (idx + 0.5) * cell

    @classmethod
    def full(cls, G=32, bound=0.5, center=(0.0, 0.0, 0.0), device=None):
        """Every cell set: the box [center - bound, center + bound)^3 alone."""
        return cls(torch.full((int(G) ** 3 // 32,), -1, dtype=torch.int32, device=device), G, center, bound)

    @classmethod
    def build(cls, model, shape_code, G=128, bound=0.5, center=(0.0, 0.0, 0.0), tau=1e-1, dilate=2, supersample=1):
        """The grid of ``model`` under ``shape_code``: the model's own plan is
        evaluated at the centres of a (G supersample)^3 lattice (explicit
        points, at most 2^20 per launch), the max over each supersample^3 block
        is the cell's density, and cn_occupancy_build thresholds (sigma >= tau)
        and dilates it.  The texture code does not enter the density: zeros."""
        s = int(supersample)
        if s < 1:
            raise ValueError("supersample must be at least 1")
        if tau < 0:
            raise ValueError("tau must not be negative")
        Gs = int(G) * s
        eng = model.engine()
        params = model.param_list()
        dev = eng.device
        eng.ensure_packed(params, bwd=False)
        code = shape_code.detach().reshape(-1).to(dev, torch.float32).contiguous()
        blob, _ = eng.latent_fwd(params, code, torch.zeros_like(code))
        sigma = eval_density(eng, blob, Gs ** 3, lambda a, b: cls.cell_centers(Gs, center, bound, a, b, dev))
        if s > 1:
            sigma = sigma.reshape(G, s, G, s, G, s).amax(dim=(1, 3, 5)).contiguous().reshape(-1)
        return cls(_eng.occupancy_build(sigma, int(G), tau, dilate), G, center, bound)
