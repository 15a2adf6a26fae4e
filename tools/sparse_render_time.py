"""Time of rendering a view dense and through an occupancy grid.

128^2 rays from a pose on the radius-1.3 sphere, 64 and 64 + 64 samples, the
bf16x3f and the bf16 plan, for two grids over [-0.5, 0.5]^3:

  * "ball": the geometric grid of a radius-0.35 ball at the origin (its kept
    share is reported; the net is then whatever --state or the committed
    weights give, only the sample count matters for the time);
  * "object": with --state (written by tools/sparse_render_eval.py) the grid
    OccupancyGrid.build makes from the trained object's optimised shape code
    at --grid / --tau / --dilate, rendered with that object's codes.

Dense and sparse calls alternate in one process after --warmup calls of each;
every call is timed by device events around it and by a host clock around the
call and a synchronise (the sparse path reads its kept count back, so its host
time is what a caller waits).  Reported, each as what it is, in ms: the dense
and the sparse time (medians of --reps), the sparse path's own overhead
(sparse_mark, the prefix sum and its read-back, sparse_gather and
sparse_scatter, timed as a pass without the MLP and compositing), the one-off
grid build, and the evaluation of 249 views both ways (249 x the per-view host
medians; the sparse one plus one build).  The clock probe (bench.clock_probe)
runs before and after.  Prints one JSON line.

  python tools/sparse_render_time.py [--state PATH] [--grid 128] [--tau 1e-1] [--dilate 2] [--reps 20] [--warmup 5]   (GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

H = W = 128
NC, NF = 64, 64
BOUND = 0.5


def ball_grid(G, dev, radius=0.35):
    from codenerf_amd.occupancy import OccupancyGrid
    c = (torch.arange(G, dtype=torch.float64) + 0.5) * (2 * BOUND / G) - BOUND
    occ = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= radius ** 2
    words = (occ.reshape(-1, 32).to(torch.int64) << torch.arange(32)).sum(1)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    return OccupancyGrid(words.to(dev), G, (0, 0, 0), BOUND)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", default=None)
    ap.add_argument("--grid", type=int, default=None)
    ap.add_argument("--tau", type=float, default=None)
    ap.add_argument("--dilate", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from codenerf_amd import _lib, engine as E
    _lib.lib()                                     # no device: HipUnavailable, nothing is timed
    from bench import clock_probe
    from codenerf_amd import optimizer as O
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.occupancy import OccupancyGrid
    from codenerf_amd.render import ImageStep
    from codenerf_amd.utils import get_rays
    from oracle.params import look_at_pose
    G = a.grid or O.OCC_GRID
    tau = O.OCC_TAU if a.tau is None else a.tau
    dilate = O.OCC_DILATE if a.dilate is None else a.dilate
    dev = torch.device("cuda", 0)
    if a.state:
        st = torch.load(a.state, map_location="cpu", weights_only=True)
        params, shape, tex = st["model"], st["shape"].to(dev), st["texture"].to(dev)
        c2w = st["poses"][1].reshape(4, 4).to(torch.float32)
    else:
        saved = torch.load(os.path.join(REPO, "weights", "c2_regime_400.pth"), map_location="cpu", weights_only=True)
        params = saved["model_params"]
        shape = saved["shape_code_params"]["weight"].mean(0).to(dev)
        tex = saved["texture_code_params"]["weight"].mean(0).to(dev)
        c2w = torch.tensor(look_at_pose(1.3, 35, 20), dtype=torch.float32)
    ro, vd = get_rays(H, W, 131.25, c2w.to(dev))
    torch.manual_seed(0)
    half = (1.8 - 0.8) / (2 * NC)
    z = (torch.linspace(0.8 + half, 1.8 - half, NC) + torch.rand(NC) * half).to(dev)

    def wall(fn):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, s.elapsed_time(e)

    med = lambda x: round(statistics.median(x), 4)
    out = {"tool": "sparse_render_time", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "Nc": NC, "Nf": NF,
           "reps": a.reps, "warmup": a.warmup, "state": bool(a.state), "grid": G, "tau": tau, "dilate": dilate,
           "clock_before": clock_probe(dev), "results": []}
    for plan in ("bf16x3f", "bf16"):
        m = CodeNeRF(3, 1, precision=plan)
        m.load_state_dict(params)
        m = m.to(dev)
        step = ImageStep(m)
        grids = {"ball": ball_grid(G, dev)}
        build_ms = None
        if a.state:
            mk = lambda: OccupancyGrid.build(m, shape, G=G, bound=BOUND, tau=tau, dilate=dilate)
            mk()
            build_ms = med([wall(mk)[0] for _ in range(5)])
            grids["object"] = mk()
        for gname, grid in grids.items():
            for nf in (0, NF):
                def render(g):
                    if nf:
                        return step.render_fine(ro, vd, z, nf, shape, tex, occupancy=g)
                    return step.render(ro, vd, z, shape, tex, occupancy=g)

                def overhead():
                    # the sparse path's own kernels and read-back over the coarse (and fine) samples,
                    # without the MLP and the compositing; fine z: the last sparse render's
                    passes = [(z, NC, True)] + ([(step.last_z_f, nf, False)] if nf else [])
                    for zz, N, last in passes:
                        keep, count = E.sparse_mark(ro, vd, zz, H * W, N, grid.bits, grid.G, grid.lo, grid.inv_cell,
                                                    last)
                        incl = torch.cumsum(count, 0, dtype=torch.int32)
                        Mk = int(incl[-1])
                        off = incl - count
                        if Mk:
                            xyz, v = E.sparse_gather(ro, vd, zz, H * W, N, keep, off, Mk)
                            E.sparse_scatter(keep, off, H * W, N, torch.empty(Mk, device=dev), xyz)

                paths = {"dense": lambda: render(None), "sparse": lambda: render(grid), "overhead": overhead}
                for _ in range(a.warmup):
                    for fn in paths.values():
                        fn()
                kept = step.last_sparse
                walls, evs = {k: [] for k in paths}, {k: [] for k in paths}
                for _ in range(a.reps):
                    for k, fn in paths.items():
                        w_, e_ = wall(fn)
                        walls[k].append(w_)
                        evs[k].append(e_)
                render(grid)
                kept = step.last_sparse
                r = {"plan": plan, "grid": gname, "samples": f"{NC}+{nf}" if nf else str(NC),
                     "grid_fraction": round(grid.fraction(), 5),
                     "kept_share": round((kept[0] + kept[1]) / kept[2], 5)}
                for k in paths:
                    r[f"{k}_host_ms"] = med(walls[k])
                    r[f"{k}_event_ms"] = med(evs[k])
                    r[f"{k}_host_min_max_ms"] = [round(min(walls[k]), 4), round(max(walls[k]), 4)]
                r["sparse_over_dense_host"] = round(r["sparse_host_ms"] / r["dense_host_ms"], 3)
                r["build_ms"] = build_ms if gname == "object" else None
                r["eval_249_views_dense_ms"] = round(249 * r["dense_host_ms"], 1)
                r["eval_249_views_sparse_ms"] = round(249 * r["sparse_host_ms"] + (r["build_ms"] or 0.0), 1)
                out["results"].append(r)
    out["clock_after"] = clock_probe(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
