"""GPU: the ray entries' outputs, bit for bit, against recorded SHA-256 hashes.

The compositing kernels share one ray (csrc/cn_ray.h: ray_forward, ray_reduce,
ray_backward, merge_ray) and one loss body (render.hip ray_loss).  The fine
loss is compared with the oracle only to a tolerance (test_gpu_fine.py), so
this is what pins every entry's bits across a change of that shared code: each
entry runs on fixed finite inputs and the SHA-256 of every output buffer is
compared with tests/golden/ray_kernel_bits.json.

Entries: cn_composite_fwd (with the weights), cn_composite_bwd, cn_render_loss,
cn_render_loss_masked (weights and a silhouette term), cn_sample_pdf,
cn_render_loss_fine and cn_render_loss_fine_masked (each from fixed non-zero
dsig_c / drgb_c), cn_composite_fine_fwd (with the opacity), cn_composite_aov
(every output) and cn_scene_composite (K = 3, labels); the last two also
without fine samples.

Shapes: R = 9 rays (two full blocks of 4 and one block with a single ray),
chunk = 4 (a ragged last chunk), (Nc, Nf) = (5, 3), (64, 64), (96, 160) (the
smallest, the workload's, the 256-sample limit), shared and per-ray coarse z;
the shared-z cases on the white background, the per-ray ones on black.  Inputs
come from numpy's frozen RandomState streams; densities include exact zeros
and values above 20, and in every ray a few fine z are set exactly equal to a
coarse z (the merge's tie rule: the coarse sample first).  No NaN, no
infinity.

The hashes belong to one build of the device code: to this ROCm's expf and
division sequences as much as to the kernels.  They say "the same as the
commit they were recorded from", not "right".  Whenever the toolchain moves,
or a change is meant to alter an output, re-record from the commit BEFORE the
change under test: build that commit's library in a scratch checkout, then on
the GPU

    CODENERF_LIB=<that checkout>/code-nerf_amd/libcodenerf_hip.so CODENERF_MEASURE=1 \\
        python tests/test_gpu_ray_bits.py > tests/golden/ray_kernel_bits.json

(the engine.* wrappers of this tree drive that library through the same C ABI).
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(REPO, "tests", "golden", "ray_kernel_bits.json")

R, CHUNK, K = 9, 4, 3
NEAR, FAR = 0.8, 1.8
SIL = 0.1
INV_S = [1.0, 0.5, 2.0]
CASES = [(Nc, Nf, per_ray) for (Nc, Nf) in ((5, 3), (64, 64), (96, 160)) for per_ray in (0, 1)]


def case_name(Nc, Nf, per_ray):
    return f"Nc{Nc}_Nf{Nf}_{'rayz' if per_ray else 'sharedz'}"


def _sigma(rs, n):
    """Densities in [0, 30): about a fifth exactly 0, about a tenth above 20."""
    s = (rs.uniform(0, 1, n) ** 3 * 20).astype(np.float32)
    pick = rs.uniform(0, 1, n)
    s[pick < 0.2] = 0.0
    hi = pick > 0.9
    s[hi] = (20 + 10 * rs.uniform(0, 1, n)).astype(np.float32)[hi]
    return s


def make_inputs(Nc, Nf, per_ray):
    """Every input of one case as float32 numpy arrays (built on the CPU)."""
    rs = np.random.RandomState(1000 * Nc + 10 * Nf + per_ray)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    zc = np.sort(f32(rs.uniform(NEAR, FAR, (R if per_ray else 1, Nc))), axis=-1)
    zf = f32(rs.uniform(NEAR, FAR, (R, Nf)))
    for r in range(R):                       # ties: a few fine z equal a coarse z exactly
        row = zc[r if per_ray else 0]
        for j, i in zip(rs.choice(Nf, min(3, Nf), replace=False), rs.choice(Nc, min(3, Nc), replace=False)):
            zf[r, j] = row[i]
    zf = np.sort(zf, axis=-1)
    d = dict(zc=zc if per_ray else zc[0], zf=zf,
             sig_c=_sigma(rs, R * Nc), sig_f=_sigma(rs, R * Nf),
             rgb_c=f32(rs.uniform(0, 1, (R * Nc, 3))), rgb_f=f32(rs.uniform(0, 1, (R * Nf, 3))),
             gt=f32(rs.uniform(0, 1, (R, 3))), g_rgb=f32(rs.normal(0, 1, (R, 3))), g_depth=f32(rs.normal(0, 1, R)),
             weight=f32(rs.uniform(0, 2, R)), acc_target=f32(rs.uniform(0, 1, R)),
             rand=f32(rs.uniform(0, 1, (R, Nf)) * 0.999),
             dsig_c0=f32(rs.normal(0, 1, R * Nc)), drgb_c0=f32(rs.normal(0, 1, (R * Nc, 3))),
             grad_c=f32(rs.normal(0, 1, (R * Nc, 3))), grad_f=f32(rs.normal(0, 1, (R * Nf, 3))))
    d["grad_c"][::7] = 0.0                   # no normal at these samples
    d["grad_f"][::5] = 0.0
    # the scene: the densities above are the combined ones, split at random
    # onto K objects of scale 1 / INV_S
    for tag, n in (("c", R * Nc), ("f", R * Nf)):
        share = f32(rs.dirichlet(np.ones(K), n).T)                       # (K, n)
        d["obj_" + tag] = f32(share * d["sig_" + tag][None] / f32(INV_S)[:, None])
    return d


def run_case(Nc, Nf, per_ray):
    """{entry.output: sha256 hex} of one case, through the engine wrappers."""
    from codenerf_amd import engine
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in make_inputs(Nc, Nf, per_ray).items()}
    wb = not per_ray
    out = {}

    def put(entry, **bufs):
        torch.cuda.synchronize()
        for name, b in bufs.items():
            assert b is not None, (entry, name)
            out[f"{entry}.{name}"] = hashlib.sha256(b.contiguous().cpu().numpy().tobytes()).hexdigest()

    w = torch.zeros(R * Nc, device=dev)
    rgb, depth = engine.composite_fwd(t["sig_c"], t["rgb_c"], t["zc"], R, Nc, white_bg=wb, weights=w)
    put("composite_fwd", rgb=rgb, depth=depth, w=w)
    dsig, drgb = engine.composite_bwd(t["sig_c"], t["rgb_c"], t["zc"], R, Nc, t["g_rgb"], t["g_depth"], white_bg=wb)
    put("composite_bwd", dsig=dsig, drgb=drgb)
    rgb, loss, dsig, drgb = engine.render_loss(t["sig_c"], t["rgb_c"], t["zc"], R, Nc, t["gt"], CHUNK, white_bg=wb)
    put("render_loss", rgb=rgb, loss=loss, dsig=dsig, drgb=drgb)
    rgb, loss, dsig, drgb, acc = engine.render_loss_masked(
        t["sig_c"], t["rgb_c"], t["zc"], R, Nc, t["gt"], CHUNK, white_bg=wb, ray_weight=t["weight"],
        acc_target=t["acc_target"], sil_coef=SIL)
    put("render_loss_masked", rgb=rgb, loss=loss, dsig=dsig, drgb=drgb, acc=acc)
    put("sample_pdf", zf=engine.sample_pdf(t["sig_c"], t["zc"], R, Nc, t["rand"]))

    planes = (t["sig_c"], t["rgb_c"], t["zc"], Nc, t["sig_f"], t["rgb_f"], t["zf"], Nf, R)
    for masked in (False, True):
        dsig_c, drgb_c = t["dsig_c0"].clone(), t["drgb_c0"].clone()
        dsig_f, drgb_f = torch.zeros(R * Nf, device=dev), torch.zeros(R * Nf, 3, device=dev)
        if masked:
            rgb, loss, acc = engine.render_loss_fine_masked(
                *planes, t["gt"], CHUNK, dsig_c, drgb_c, dsig_f, drgb_f, white_bg=wb, ray_weight=t["weight"],
                acc_target=t["acc_target"], sil_coef=SIL)
            put("render_loss_fine_masked", acc=acc)
        else:
            rgb, loss = engine.render_loss_fine(*planes, t["gt"], CHUNK, dsig_c, drgb_c, dsig_f, drgb_f, white_bg=wb)
        put("render_loss_fine_masked" if masked else "render_loss_fine", rgb=rgb, loss=loss, dsig_c=dsig_c,
            drgb_c=drgb_c, dsig_f=dsig_f, drgb_f=drgb_f)
    rgb, depth, acc = engine.composite_fine_fwd(*planes, white_bg=wb, acc=True)
    put("composite_fine_fwd", rgb=rgb, depth=depth, acc=acc)

    o = engine.composite_aov(t["sig_c"], t["rgb_c"], t["zc"], Nc, R, white_bg=wb, grad_c=t["grad_c"],
                             sigma_f=t["sig_f"], rgb_f=t["rgb_f"], z_f=t["zf"], Nf=Nf, grad_f=t["grad_f"])
    put("composite_aov", **o)
    o = engine.composite_aov(t["sig_c"], t["rgb_c"], t["zc"], Nc, R, white_bg=wb, grad_c=t["grad_c"])
    put("composite_aov_coarse", **o)
    o = engine.scene_composite(t["sig_c"], t["rgb_c"], t["zc"], Nc, R, INV_S, white_bg=wb, sigma_f=t["sig_f"],
                               rgb_f=t["rgb_f"], z_f=t["zf"], Nf=Nf, obj_c=t["obj_c"], obj_f=t["obj_f"])
    put("scene_composite", **o)
    o = engine.scene_composite(t["sig_c"], t["rgb_c"], t["zc"], Nc, R, INV_S, white_bg=wb, obj_c=t["obj_c"])
    put("scene_composite_coarse", **o)
    return out


def test_inputs_are_finite_with_ties_and_extreme_densities():
    """What the fixture's inputs are meant to contain (no device needed)."""
    for Nc, Nf, per_ray in CASES:
        d = make_inputs(Nc, Nf, per_ray)
        assert all(np.isfinite(v).all() for v in d.values())
        assert (np.diff(d["zc"], axis=-1) >= 0).all() and (np.diff(d["zf"], axis=-1) >= 0).all()
        for tag in ("c", "f"):
            assert (d["sig_" + tag] == 0).any() and (d["sig_" + tag] > 20).any()
        zc = d["zc"] if per_ray else np.broadcast_to(d["zc"], (R, Nc))
        assert all(np.isin(d["zf"][r], zc[r]).sum() >= 1 for r in range(R))


@pytest.mark.gpu
@pytest.mark.parametrize("Nc,Nf,per_ray", CASES, ids=[case_name(*c) for c in CASES])
def test_ray_entries_match_recorded_bits(Nc, Nf, per_ray):
    with open(FIXTURE) as f:
        want = json.load(f)[case_name(Nc, Nf, per_ray)]
    got = run_case(Nc, Nf, per_ray)
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f"outputs whose bits differ from the recorded ones: {differ}"


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    print(json.dumps({case_name(*c): run_case(*c) for c in CASES}, indent=1, sort_keys=True))
