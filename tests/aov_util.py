"""Helpers of the geometry-buffer tests (test infrastructure): the inputs of
the cn_composite_aov tests and a float64 numpy restatement of its five
outputs, built from oracle.ref_cpu.merge_samples and composite_weights.

Definitions (include/codenerf.h, cn_composite_aov), over a ray's merged
samples with the compositing weights w:
  rgb = sum w c (+ 1 - sum w on a white background), depth = sum w z,
  acc = sum w, depth_med = z_m of the first m with C_m = sum_{j <= m} w_j >= 0.5
  (z_{N-1} when there is none), normal = sum w u, u = -g / |g| and 0 unless
  |g| > 0.
"""
import numpy as np
import torch

from oracle import ref_cpu

R_MAX = 257
# A ray is left out of the depth_med comparison when a C_k of the float64
# restatement lies this close to 0.5: the kernel's fp32 weights differ from the
# float64 ones by ~1e-6, so the first index at or above 0.5 is then undecided.
MED_GUARD = 1e-5


def inputs(Nc, Nf, per_ray_z):
    """257 rays in the construction of test_gpu_fine_opt._composite_inputs
    (Nf 0: coarse only), plus gradients -> dict of float32 tensors zc, zf, sc,
    sf, rc, rf, gc, gf (the fine ones (R, 0[, 3]) when Nf is 0).
    Ray 0: coarse / fine ties; ray 1: zero density (the depth_med fall-back, a
    zero-length normal); ray 2: an opaque wall; ray 3: a zero gradient at its
    heaviest sample.  Gradients: randn times a per-sample scale 10^U(-6, 6);
    colours: randn clipped to [-1, 1]."""
    g = torch.Generator().manual_seed(Nc * 13 + Nf + int(per_ray_z))
    R = R_MAX
    if per_ray_z:
        zc = torch.sort(0.8 + torch.rand(R, Nc, generator=g), -1).values
    else:
        zc = torch.linspace(0.8, 1.8, Nc)
    zf = torch.sort(0.8 + torch.rand(R, Nf, generator=g), -1).values
    if Nf:
        zf[0, :4] = zc[0, 3] if per_ray_z else zc[3]
        zf[0] = torch.sort(zf[0]).values             # the tied samples stay; z_f stays ascending
    sc = torch.rand(R, Nc, generator=g) * 6
    sf = torch.rand(R, Nf, generator=g) * 6
    sc[1], sf[1] = 0.0, 0.0
    sc[2, Nc // 2] = 1e4
    rc = torch.randn(R, Nc, 3, generator=g).clamp(-1, 1)
    rf = torch.randn(R, Nf, 3, generator=g).clamp(-1, 1)
    scale = lambda n: 10.0 ** (torch.rand(R, n, 1, generator=g) * 12 - 6)
    gc = torch.randn(R, Nc, 3, generator=g) * scale(Nc)
    gf = torch.randn(R, Nf, 3, generator=g) * scale(Nf)
    # ray 3: the heaviest merged sample gets a zero gradient
    d = dict(zc=zc, zf=zf, sc=sc, sf=sf, rc=rc, rf=rf, gc=gc, gf=gf)
    z_m, s_m, src = merged(d, ("sc", "sf"), "index")
    k = int(src[3, int(ref_cpu.composite_weights(s_m.double(), z_m.double())[3].argmax())])
    if k < Nc:
        gc[3, k] = 0.0
    else:
        gf[3, k - Nc] = 0.0
    return d


def merged(d, *pairs):
    """merge_samples of the inputs: z and, per pair of keys, the merged values;
    the pair "index" gives every merged sample's source (coarse i: i, fine j:
    Nc + j)."""
    R, Nc, Nf = R_MAX, d["sc"].shape[1], d["sf"].shape[1]
    vals = []
    for p in pairs:
        if p == "index":
            idx = torch.arange(Nc + Nf).expand(R, -1)
            vals.append((idx[:, :Nc], idx[:, Nc:]))
        else:
            vals.append((d[p[0]], d[p[1]]))
    return ref_cpu.merge_samples(d["zc"], d["zf"], *vals)


def restate(z, sigma, rgb, grad, white_bg=False):
    """float64 numpy restatement over already merged samples: z, sigma (R, N),
    rgb, grad (R, N, 3), any float tensors / arrays -> dict of float64 arrays
    rgb, depth, acc, depth_med, normal, C (R, N) and the weights w."""
    z, sigma, rgb, grad = (torch.as_tensor(np.asarray(a, dtype=np.float64)) for a in (z, sigma, rgb, grad))
    w = ref_cpu.composite_weights(sigma, z).numpy()
    z, rgb, g = z.numpy(), rgb.numpy(), grad.numpy()
    acc = w.sum(-1)
    col = (w[..., None] * rgb).sum(-2)
    if white_bg:
        col = col + 1 - acc[:, None]
    C = np.cumsum(w, -1)
    hit = C >= 0.5
    m = np.where(hit.any(-1), hit.argmax(-1), z.shape[-1] - 1)
    n = np.sqrt((g * g).sum(-1, keepdims=True))
    u = np.divide(-g, n, out=np.zeros_like(g), where=n > 0)
    return dict(rgb=col, depth=(w * z).sum(-1), acc=acc, depth_med=np.take_along_axis(z, m[:, None], -1)[:, 0],
                normal=(w[..., None] * u).sum(-2), C=C, w=w)


def restate_inputs(d, white_bg=False):
    """restate over the merged samples of ``inputs``."""
    z_m, s_m, r_m, g_m = merged(d, ("sc", "sf"), ("rc", "rf"), ("gc", "gf"))
    return restate(z_m, s_m, r_m, g_m, white_bg)


def undecided(C):
    """Rays whose running weight sum comes within MED_GUARD of 0.5 (R,) bool."""
    return (np.abs(C - 0.5) < MED_GUARD).any(-1)


def unit_normals_f32(g):
    """u = -g / |g| as the kernel forms it, in float32: |g| = sqrt((x x + y y)
    + z z) with every operation rounded separately, (0, 0, 0) unless |g| > 0."""
    g = np.asarray(g, dtype=np.float32)
    x, y, z = g[..., 0], g[..., 1], g[..., 2]
    n = np.sqrt((x * x + y * y) + z * z)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, -g / n, np.float32(0)).astype(np.float32)
