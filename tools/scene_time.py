"""Time of a composed scene, in ms by device events (--warmup
calls, median of --reps, min and max beside it), on a random-weight srncar net
(oracle.params.make_params) at --precision, a --size^2 (default 128) image with
64 + 64 samples, every object's grid built by OccupancyGrid.build with the
Optimizer's defaults over the box of half side 0.5:

  * ImageStep.render_scene with one object (identity, s = 1) against
    render_fine(occupancy=) on the same grid;
  * render_scene with three objects (generic rotations, translations within
    0.3, scales 0.75, 1, 1.5) against three such render_fine calls;
  * the three new kernels alone at the scene's shapes (cn_scene_rays once,
    cn_scene_combine for the coarse and for the fine rows, cn_scene_composite
    with the labels) and their share of the three-object render;
  * the kept-sample shares (``ImageStep.last_sparse``) and the grid fraction.

The clock probe (bench.clock_probe) runs before and after.  Prints one JSON line.

  python tools/scene_time.py [--precision bf16x3f] [--size 128] [--reps 20] [--warmup 5]   (GPU)
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16x3f")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from codenerf_amd import _lib, engine as E
    _lib.lib()                                     # no device: HipUnavailable, nothing is timed
    from bench import clock_probe
    from codenerf_amd.edit import orbit_pose
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.occupancy import OccupancyGrid
    from codenerf_amd.render import ImageStep
    from codenerf_amd.scene import Scene, SceneObject, rotation_zyx
    from codenerf_amd.utils import get_rays
    from oracle.params import make_codes, make_params
    dev = torch.device("cuda", 0)

    def timed(fn):
        ev = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ev.append(s.elapsed_time(e))
        return {"event_ms": round(statistics.median(ev), 4), "event_min_max_ms": [round(min(ev), 4), round(max(ev), 4)]}

    Nc = Nf = 64
    out = {"tool": "scene_time", "device": torch.cuda.get_device_name(0), "precision": a.precision, "reps": a.reps,
           "warmup": a.warmup, "size": a.size, "Nc": Nc, "Nf": Nf, "clock_before": clock_probe(dev)}
    m = CodeNeRF(3, 1, precision=a.precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in make_params(3, sigma_bias_shift=2.0).items()})
    m = m.to(dev)
    shapes, textures = (torch.tensor(c, device=dev) for c in make_codes(3, 3))
    step = ImageStep(m)
    ro, vd = get_rays(a.size, a.size, 131.25 * a.size / 128, orbit_pose(1.3, 35.0, 20.0).to(dev))
    R = ro.shape[0]
    z = torch.linspace(0.8, 1.8, Nc, device=dev)
    grids = [OccupancyGrid.build(m, shapes[k], bound=0.5) for k in range(3)]
    out["grid_fraction"] = [round(g.fraction(), 4) for g in grids]
    share = lambda: round((step.last_sparse[0] + step.last_sparse[1]) / step.last_sparse[2], 4)

    one = Scene([SceneObject(shapes[0], textures[0], grids[0])])
    r = {"render_fine_occupancy": timed(lambda: step.render_fine(ro, vd, z, Nf, shapes[0], textures[0],
                                                                 occupancy=grids[0]))}
    r["kept_render_fine"] = share()
    r["render_scene"] = timed(lambda: step.render_scene(ro, vd, z, one, n_fine=Nf))
    r["kept_render_scene"] = share()
    r["render_scene_no_labels"] = timed(lambda: step.render_scene(ro, vd, z, one, n_fine=Nf, labels=False))
    out["one_object"] = r

    xf = [(rotation_zyx(30, 20, -15), (0.25, -0.1, 0.05), 0.75), (rotation_zyx(-70, 10, 40), (-0.3, 0.2, -0.1), 1.0),
          (rotation_zyx(115, -25, 5), (0.05, 0.3, 0.2), 1.5)]
    three = Scene([SceneObject(shapes[k], textures[k], grids[k], *xf[k]) for k in range(3)])
    r = {"three_render_fine_occupancy": timed(lambda: [step.render_fine(ro, vd, z, Nf, shapes[k], textures[k],
                                                                        occupancy=grids[k]) for k in range(3)])}
    r["render_scene"] = timed(lambda: step.render_scene(ro, vd, z, three, n_fine=Nf))
    r["kept_render_scene"] = share()
    out["three_objects"] = r

    # the new kernels alone, at the three-object scene's shapes
    K = 3
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g).to(dev)
    inv_s = three.inv_s()
    oc, of = rnd(K, R * Nc) * 2, rnd(K, R * Nf) * 2
    cc, cf = rnd(K, R * Nc, 3), rnd(K, R * Nf, 3)
    zf = torch.sort(0.8 + rnd(R, Nf), -1).values.contiguous()
    sc, rc = E.scene_combine(oc, cc, inv_s)
    sf, rf = E.scene_combine(of, cf, inv_s)
    k = {"K": K, "R": R,
         "scene_rays": timed(lambda: E.scene_rays(ro, vd, three.transforms())),
         "scene_combine_coarse": timed(lambda: E.scene_combine(oc, cc, inv_s)),
         "scene_combine_fine": timed(lambda: E.scene_combine(of, cf, inv_s)),
         "scene_composite": timed(lambda: E.scene_composite(sc, rc, z, Nc, R, inv_s, sigma_f=sf, rgb_f=rf, z_f=zf,
                                                            Nf=Nf, obj_c=oc, obj_f=of)),
         "scene_composite_no_labels": timed(lambda: E.scene_composite(sc, rc, z, Nc, R, inv_s, sigma_f=sf, rgb_f=rf,
                                                                      z_f=zf, Nf=Nf, labels=False)),
         "composite_fine_fwd": timed(lambda: E.composite_fine_fwd(sc, rc, z, Nc, sf, rf, zf, Nf, R, acc=True))}
    new = sum(k[n]["event_ms"] for n in ("scene_rays", "scene_combine_coarse", "scene_combine_fine", "scene_composite"))
    k["new_kernels_ms"] = round(new, 4)
    k["share_of_render_scene"] = round(new / out["three_objects"]["render_scene"]["event_ms"], 4)
    out["kernels"] = k
    out["clock_after"] = clock_probe(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
