"""Helpers of the scene tests (test infrastructure): numpy restatements of the
three scene entries (include/codenerf.h) and the inputs of their
kernel tests.

cn_scene_rays and cn_scene_combine are restated in float32 with one rounding
per operation in the order the header gives, so the device must match them bit
for bit.  cn_scene_composite is restated in float64 over the merged samples,
built on oracle.ref_cpu.merge_samples and composite_weights as aov_util.restate
is.
"""
import numpy as np
import torch

import aov_util
from oracle import ref_cpu

F = np.float32
R_MAX = aov_util.R_MAX
INV_S = (1.0, 0.5, 2.0, 1.25, 0.75, 1.5, 1.0, 3.0)
SHAPES = [(2, 0), (5, 0), (64, 0), (65, 0), (256, 0), (5, 3), (64, 64), (96, 160)]
KS = (1, 2, 3, 8)
# A ray's label is undecided when, in float64, its opacity lies this close to
# acc_min or its two largest shares this close to each other: the kernel's
# float32 weights differ from the float64 ones by ~1e-6.
GUARD = 1e-5
MAX_UNDECIDED = 0.02


# ------------------------------------------------------------ transforms
def transform_row(rot, t, scale):
    """The 13 float32 values cn_scene_rays takes: R row-major, t, 1 / s."""
    return np.concatenate([np.asarray(rot, dtype=np.float64).reshape(-1), np.asarray(t, dtype=np.float64),
                           [1.0 / float(scale)]]).astype(F)


def random_rotation(rng):
    """A proper rotation from a random unit quaternion -> (3, 3) float64."""
    w, x, y, z = (q := rng.standard_normal(4)) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_rays(ro, rd, rows):
    """cn_scene_rays: ro, rd (R, 3) float32, rows (K, 13) float32 ->
    (origins (K, R, 3), directions (K, R, 3)) float32."""
    ro, rd = np.asarray(ro, dtype=F), np.asarray(rd, dtype=F)
    out_o, out_d = [], []
    for row in np.asarray(rows, dtype=F).reshape(-1, 13):
        rot, t, inv_s = row[:9].reshape(3, 3), row[9:12], row[12]
        q = ro - t
        o = np.stack([((rot[0, a] * q[:, 0] + rot[1, a] * q[:, 1]) + rot[2, a] * q[:, 2]) * inv_s for a in range(3)], 1)
        d = np.stack([(rot[0, a] * rd[:, 0] + rot[1, a] * rd[:, 1]) + rot[2, a] * rd[:, 2] for a in range(3)], 1)
        assert o.dtype == F and d.dtype == F
        out_o.append(o)
        out_d.append(d)
    return np.stack(out_o), np.stack(out_d)


# ------------------------------------------------------------ combine
def shares(sig_k, inv_s, sigma):
    """f_k = (sigma_k * (1 / s_k)) / sigma in float32, 0 unless sigma > 0:
    sig_k (K, ...), sigma (...) -> (K, ...) float32."""
    sig_k, sigma = np.asarray(sig_k, dtype=F), np.asarray(sigma, dtype=F)
    pos = sigma > 0
    out = np.zeros(sig_k.shape, dtype=F)
    with np.errstate(all="ignore"):
        for k in range(sig_k.shape[0]):
            a = sig_k[k] * F(inv_s[k])
            out[k] = np.where(pos, a / np.where(pos, sigma, F(1)), F(0))
    return out


def combine(sig_k, rgb_k, inv_s):
    """cn_scene_combine: sig_k (K, M), rgb_k (K, M, 3) float32 -> (sigma (M,),
    rgb (M, 3)) float32; both sums left to right from the first term."""
    sig_k, rgb_k = np.asarray(sig_k, dtype=F), np.asarray(rgb_k, dtype=F)
    K = sig_k.shape[0]
    with np.errstate(all="ignore"):
        sigma = sig_k[0] * F(inv_s[0])
        for k in range(1, K):
            sigma = sigma + sig_k[k] * F(inv_s[k])
        f = shares(sig_k, inv_s, sigma)
        rgb = f[0][:, None] * rgb_k[0]
        for k in range(1, K):
            rgb = rgb + f[k][:, None] * rgb_k[k]
    rgb = np.where((sigma > 0)[:, None], rgb, F(0))
    assert sigma.dtype == F and rgb.dtype == F
    return sigma, rgb


def same_bits(a, b):
    """Equal bit for bit, any NaN standing for any NaN."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------ composite
def inputs(Nc, Nf, per_ray_z, K):
    """The kernel-test inputs: aov_util.inputs' 257 rays and z (ray 0 the
    coarse / fine ties, ray 1 zero density, ray 2 a wall) with K object planes
    rand * 6 / K, each (object, ray) pair zeroed with probability 1/2, every
    object zeroed on ray 1, a 1e4 wall in object K - 1 at ray 2's coarse sample
    Nc // 2, ray 3 + k object k alone and dense enough to own it (so that every
    label occurs whatever the draw), colours in [0, 1), 1 / s the first K of
    INV_S; the combined planes are ``combine`` of these.  -> dict of float32 arrays zc ((Nc,) or (R, Nc)),
    zf (R, Nf), oc (K, R, Nc), of (K, R, Nf), sc, sf, rc, rf and inv_s."""
    base = aov_util.inputs(Nc, Nf, per_ray_z)
    R = R_MAX
    g = torch.Generator().manual_seed(7919 * K + Nc * 13 + Nf + int(per_ray_z))
    oc = torch.rand(K, R, Nc, generator=g) * 6 / K
    of = torch.rand(K, R, Nf, generator=g) * 6 / K
    live = torch.rand(K, R, generator=g) >= 0.5
    live[:, 1] = False
    for k in range(K):                           # ray 3 + k: object k alone, at a density of rand * 6 after its scale
        live[:, 3 + k] = False
        live[k, 3 + k] = True
        oc[k, 3 + k] *= K / INV_S[k]
        of[k, 3 + k] *= K / INV_S[k]
    oc, of = oc * live[..., None], of * live[..., None]
    oc[K - 1, 2, Nc // 2] = 1e4
    ck = torch.rand(K, R, Nc, 3, generator=g)
    fk = torch.rand(K, R, Nf, 3, generator=g)
    inv_s = [float(v) for v in INV_S[:K]]
    oc, of, ck, fk = (t.numpy().astype(F) for t in (oc, of, ck, fk))
    sc, rc = combine(oc.reshape(K, -1), ck.reshape(K, -1, 3), inv_s)
    if Nf:
        sf, rf = combine(of.reshape(K, -1), fk.reshape(K, -1, 3), inv_s)
    else:
        sf, rf = np.zeros(0, dtype=F), np.zeros((0, 3), dtype=F)
    return dict(zc=base["zc"].numpy().astype(F), zf=base["zf"].numpy().astype(F), oc=oc, of=of,
                sc=sc.reshape(R, Nc), sf=sf.reshape(R, Nf), rc=rc.reshape(R, Nc, 3), rf=rf.reshape(R, Nf, 3),
                inv_s=inv_s)


def labels(obj_acc, acc, acc_min=0.5):
    """instance and the undecided rays from float64 obj_acc (R, K), acc (R,)."""
    inst = np.where(acc >= acc_min, obj_acc.argmax(-1), -1).astype(np.int32)
    und = np.abs(acc - acc_min) < GUARD
    if obj_acc.shape[1] > 1:
        top = np.sort(obj_acc, -1)
        und |= (acc >= acc_min) & (top[:, -1] - top[:, -2] < GUARD)
    return inst, und


def restate_composite(zc, sc, rc, oc, inv_s, zf=None, sf=None, rf=None, of=None, white_bg=False, acc_min=0.5):
    """float64 restatement of cn_scene_composite: zc (Nc,) or (R, Nc), sc (R, Nc),
    rc (R, Nc, 3) the combined planes, oc (K, R, Nc) the object densities; the
    fine ones alike (None or Nf 0: coarse only) -> dict of float64 arrays rgb,
    depth, acc, obj_acc (R, K), w (R, N) and instance int32, undecided bool."""
    t64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    K, R = oc.shape[0], sc.shape[0]
    z, sig, rgb = t64(zc), t64(sc), t64(rc)
    if z.dim() == 1:
        z = z.expand(R, -1)
    obj = [t64(oc[k]) for k in range(K)]
    if zf is not None and np.asarray(zf).shape[-1] > 0:
        pairs = [(sig, t64(sf)), (rgb, t64(rf))] + [(obj[k], t64(of[k])) for k in range(K)]
        z, sig, rgb, *obj = ref_cpu.merge_samples(z, t64(zf), *pairs)
    w = ref_cpu.composite_weights(sig, z).numpy()
    z, sig, rgb = z.numpy(), sig.numpy(), rgb.numpy()
    acc = w.sum(-1)
    col = (w[..., None] * rgb).sum(-2)
    if white_bg:
        col = col + 1 - acc[:, None]
    pos = sig > 0
    with np.errstate(all="ignore"):
        f = [np.where(pos, obj[k].numpy() * float(inv_s[k]) / np.where(pos, sig, 1.0), 0.0) for k in range(K)]
    obj_acc = np.stack([(w * f[k]).sum(-1) for k in range(K)], -1)
    inst, und = labels(obj_acc, acc, acc_min)
    return dict(rgb=col, depth=(w * z).sum(-1), acc=acc, obj_acc=obj_acc, w=w, instance=inst, undecided=und)


def restate_inputs(d, white_bg=False, acc_min=0.5):
    return restate_composite(d["zc"], d["sc"], d["rc"], d["oc"], d["inv_s"], d["zf"], d["sf"], d["rf"], d["of"],
                             white_bg, acc_min)


def obj_acc_from_weights(w, sigma, obj, inv_s):
    """Coarse obj_acc from the device's own float32 weights w (R, N): float32
    shares, float32 products, float64 sums -> (R, K) float64."""
    f = shares(obj, inv_s, sigma)
    w = np.asarray(w, dtype=F)
    return np.stack([(w * f[k]).astype(np.float64).sum(-1) for k in range(obj.shape[0])], -1)
