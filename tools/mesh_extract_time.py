"""Time of mesh extraction, stage by stage.

The object: with --state (written by tools/sparse_render_eval.py) the trained
synthetic object's model and optimised codes; without it, a short run of the
same recipe in this process (--iters training steps, --num_opts code steps).
For every lattice of --grids (default 128 256) points per axis over
[-0.5, 0.5]^3 and the plan --precision, separately, in ms by device events
(--warmup calls, median of --reps, min and max beside it):

  * lattice: the density of the n^3 points through the MLP (2^20 per launch);
  * count:   cn_mesh_count;
  * scan:    the two prefix sums and the read-back of the two totals (host
             clock around a synchronise as well: the read-back is a wait);
  * emit:    cn_mesh_emit;
  * normals: codes forward, pose backward, input gradient at the vertices;
  * colors:  the forward at the vertices;
  * total:   mesh.extract_mesh, host clock around the call and a synchronise.

iso is the --quantile (default 0.9) of the lattice's densities, so the share of
crossing edges does not depend on the model's scale.  count and emit are set
against the bytes they must move at --hbm TB/s (DESIGN.md 3 uses 8): the field
is read once by each kernel (4 P), the flag and count arrays are written once
(9 P) and flags and offsets read once (9 P), the outputs written (12 Nv + 12
Nt).  The clock probe (bench.clock_probe) runs before and after.  Prints one
JSON line.

  python tools/mesh_extract_time.py [--state PATH] [--grids 128 256] [--precision bf16x3f] [--reps 20] [--warmup 5]   (GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

BOUND = 0.5


def min_bytes(P, Nv, Nt):
    """-> (count, emit) bytes the two kernels must move."""
    return 4 * P + 9 * P, 4 * P + 9 * P + 12 * Nv + 12 * Nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--state", default=None)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--precision", default="bf16x3f")
    ap.add_argument("--quantile", type=float, default=0.9)
    ap.add_argument("--hbm", type=float, default=8.0, help="TB/s the byte counts are set against")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--train_objs", type=int, default=4)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--n_fine", type=int, default=64)
    ap.add_argument("--num_opts", type=int, default=50)
    a = ap.parse_args()
    from codenerf_amd import _lib, engine as E
    _lib.lib()                                     # no device: HipUnavailable, nothing is timed
    from bench import clock_probe
    from codenerf_amd import mesh as M
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.occupancy import eval_density
    dev = torch.device("cuda", 0)
    if a.state:
        st = torch.load(a.state, map_location="cpu", weights_only=True)
        params, shape, tex = st["model"], st["shape"].to(dev), st["texture"].to(dev)
    else:
        import sparse_render_eval as S
        opt, _ = S.trained_object(a)
        params = {k: v.detach().cpu() for k, v in opt.model.state_dict().items()}
        shape, tex = opt.optimized_shapecodes[0].to(dev), opt.optimized_texturecodes[0].to(dev)
    m = CodeNeRF(3, 1, precision=a.precision)
    m.load_state_dict(params)
    m = m.to(dev)
    eng = m.engine()
    plist = m.param_list()
    eng.ensure_packed(plist, bwd=True)
    blob, _ = eng.latent_fwd(plist, shape.reshape(-1).contiguous(), tex.reshape(-1).contiguous())

    def timed(fn):
        """-> (event ms, host ms around the call and a synchronise) medians, and the event min / max."""
        ev, host = [], []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
                ev.append(s.elapsed_time(e))
        return {"event_ms": round(statistics.median(ev), 4), "host_ms": round(statistics.median(host), 4),
                "event_min_max_ms": [round(min(ev), 4), round(max(ev), 4)]}

    out = {"tool": "mesh_extract_time", "device": torch.cuda.get_device_name(0), "precision": a.precision,
           "state": bool(a.state), "reps": a.reps, "warmup": a.warmup, "quantile": a.quantile, "hbm_tbps": a.hbm,
           "clock_before": clock_probe(dev), "results": []}
    for n in a.grids:
        P, dims = n ** 3, (n, n, n)
        lo, s = M.lattice_geometry(n, BOUND)
        lattice = lambda: eval_density(eng, blob, P, lambda i, j: M.lattice_points(n, lo, s, i, j, dev))
        field = lattice()
        # the quantile of a sample: torch.quantile takes at most 2^24 values
        iso = float(torch.quantile(field[::max(1, P // (1 << 22))], a.quantile))
        vflags, vcount, tcount = E.mesh_count(field, dims, iso)

        def scan():
            vs, ts = torch.cumsum(vcount, 0, dtype=torch.int32), torch.cumsum(tcount, 0, dtype=torch.int32)
            nv, nt = (int(x) for x in torch.stack([vs[-1], ts[-1]]).cpu())
            return vs - vcount, ts - tcount, nv, nt

        voff, toff, Nv, Nt = scan()
        r = {"n": n, "points": P, "iso": iso, "vertices": Nv, "triangles": Nt}
        if Nt == 0:
            r["note"] = "no surface at this iso"
            out["results"].append(r)
            continue
        vert = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
        tri = torch.empty(Nt, 3, dtype=torch.int32, device=dev)
        emit = lambda: E.mesh_emit(field, dims, iso, lo, (s, s, s), vflags, voff, toff, Nv, Nt, vert=vert, tri=tri)
        emit()
        nrm = M.vertex_normals(eng, blob, vert)
        stages = {"lattice": lattice, "count": lambda: E.mesh_count(field, dims, iso), "scan": scan, "emit": emit,
                  "normals": lambda: M.vertex_normals(eng, blob, vert),
                  "colors": lambda: M.vertex_colors(eng, blob, vert, nrm),
                  "total": lambda: M.extract_mesh(m, shape, tex, n=n, bound=BOUND, iso=iso)}
        for name, fn in stages.items():
            r[name] = timed(fn)
        for name, nbytes in zip(("count", "emit"), min_bytes(P, Nv, Nt)):
            floor_ms = nbytes / (a.hbm * 1e12) * 1e3
            r[name].update(min_bytes=nbytes, floor_ms=round(floor_ms, 5),
                           achieved_tbps=round(nbytes / (r[name]["event_ms"] * 1e-3) / 1e12, 3),
                           fraction_of_hbm=round(floor_ms / r[name]["event_ms"], 4))
        out["results"].append(r)
    out["clock_after"] = clock_probe(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
