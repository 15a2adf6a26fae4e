"""Time of the geometry buffers, in ms by device events
(--warmup calls, median of --reps, min and max beside it), on a random-weight
srncar net (oracle.params.make_params) at --precision:

  * kernels, R = --rays (default 16,384), N = 64 and 64 + 64, random inputs:
    cn_composite_fwd / cn_composite_fine_fwd (with the opacity) against
    cn_composite_aov without and with the normal;
  * a --size^2 (default 128) image, 64 and 64 + 64 samples: ImageStep.render /
    render_fine against render_aov(normals=False) and render_aov(normals=True).

The clock probe (bench.clock_probe) runs before and after.  Prints one JSON line.

  python tools/aov_time.py [--precision bf16x3f] [--rays 16384] [--size 128] [--reps 20] [--warmup 5]   (GPU)
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
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from codenerf_amd import _lib, engine as E
    _lib.lib()                                     # no device: HipUnavailable, nothing is timed
    from bench import clock_probe
    from codenerf_amd.edit import orbit_pose
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.render import ImageStep
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

    out = {"tool": "aov_time", "device": torch.cuda.get_device_name(0), "precision": a.precision, "reps": a.reps,
           "warmup": a.warmup, "clock_before": clock_probe(dev), "kernels": [], "images": []}
    g = torch.Generator().manual_seed(0)
    R = a.rays
    rnd = lambda *s: torch.rand(*s, generator=g).to(dev)
    for Nc, Nf in ((64, 0), (64, 64)):
        zc = torch.linspace(0.8, 1.8, Nc, device=dev)
        sc, rc, gc = rnd(R * Nc) * 6, rnd(R * Nc, 3), rnd(R * Nc, 3) - 0.5
        r = {"R": R, "Nc": Nc, "Nf": Nf}
        fine = {}
        if Nf:
            zf = torch.sort(0.8 + rnd(R, Nf), -1).values.contiguous()
            fine = dict(sigma_f=rnd(R * Nf) * 6, rgb_f=rnd(R * Nf, 3), z_f=zf, Nf=Nf)
            r["composite_fine_fwd"] = timed(lambda: E.composite_fine_fwd(sc, rc, zc, Nc, fine["sigma_f"], fine["rgb_f"],
                                                                         zf, Nf, R, acc=True))
        else:
            r["composite_fwd"] = timed(lambda: E.composite_fwd(sc, rc, zc, R, Nc))
        r["composite_aov"] = timed(lambda: E.composite_aov(sc, rc, zc, Nc, R, **fine))
        grads = dict(fine, grad_c=gc, **(dict(grad_f=rnd(R * Nf, 3) - 0.5) if Nf else {}))
        r["composite_aov_normal"] = timed(lambda: E.composite_aov(sc, rc, zc, Nc, R, **grads))
        out["kernels"].append(r)

    m = CodeNeRF(3, 1, precision=a.precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in make_params(3, sigma_bias_shift=2.0).items()})
    m = m.to(dev)
    s, t = (torch.tensor(c[1], device=dev) for c in make_codes(3, 2))
    step = ImageStep(m)
    ro, vd = get_rays(a.size, a.size, 131.25 * a.size / 128, orbit_pose(1.3, 35.0, 20.0).to(dev))
    z = torch.linspace(0.8, 1.8, 64, device=dev)
    for Nf in (0, 64):
        r = {"size": a.size, "Nc": 64, "Nf": Nf}
        if Nf:
            r["render_fine"] = timed(lambda: step.render_fine(ro, vd, z, Nf, s, t))
        else:
            r["render"] = timed(lambda: step.render(ro, vd, z, s, t))
        r["render_aov"] = timed(lambda: step.render_aov(ro, vd, z, s, t, n_fine=Nf, normals=False))
        r["render_aov_normals"] = timed(lambda: step.render_aov(ro, vd, z, s, t, n_fine=Nf))
        out["images"].append(r)
    out["clock_after"] = clock_probe(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
