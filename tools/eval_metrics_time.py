"""Time of the evaluation metrics of one object: host loop against device kernel.

On seeded 128 x 128 white-background images and 249 views (one SRN test
object), both given the same device tensors:

  (a) host: what Optimizer.optimize_objs does per view with device_metrics
      off -- the chunk means read with float() (one host synchronisation per
      chunk), the two .cpu() copies and metrics.ssim_legacy;
  (b) device: metrics.image_metrics per view into one (views, 2) buffer and
      one read-back after the last view (device_metrics on);
  (c) the same kernel in one call over all views (what a caller holding all
      images at once would do; the Optimizer renders view by view).

Every path is warmed up, then timed `--reps` times, alternating, by a host
clock around work that ends in a device synchronise; (b) and (c) also by
device events around the enqueued work.  Prints one JSON line (times in ms
per object: medians, and every repetition) with the largest PSNR / SSIM
difference between the paths.  Needs a HIP device.

  python tools/eval_metrics_time.py [--views 249] [--size 128] [--chunk 2048] [--reps 5]
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


def make_views(V, H, W, dev):
    """Renders and targets with the SRN look: white background, a textured
    rectangle, the render a perturbed copy of the target."""
    g = torch.Generator().manual_seed(0)
    tgt = torch.ones(V, H, W, 3)
    tgt[:, H // 4:H - H // 4, W // 4:W - W // 4] = torch.rand(V, H - 2 * (H // 4), W - 2 * (W // 4), 3, generator=g)
    rgb = (tgt + 0.05 * torch.randn(tgt.shape, generator=g)).clamp(0, 1)
    return rgb.reshape(V, H * W, 3).to(dev), tgt.reshape(V, H * W, 3).to(dev)


def host_path(rgbs, tgts, H, W, B):
    from codenerf_amd.metrics import ssim_legacy
    res = []
    for rgb, tgt_img in zip(rgbs, tgts):
        se = ((rgb - tgt_img) ** 2).sum(-1)
        chunk_mse = [float(se[i:i + B].mean()) / 3 for i in range(0, H * W, B)]
        res.append((float(-10 * np.log(float(np.mean(chunk_mse))) / np.log(10)),
                    ssim_legacy(rgb.reshape(H, W, 3).cpu().numpy(), tgt_img.reshape(H, W, 3).cpu().numpy())))
    return np.array(res)


def device_path(rgbs, tgts, H, W, B, batched):
    """-> ((psnr, ssim) per view, device ms of the enqueued metrics work)."""
    from codenerf_amd.metrics import image_metrics, psnr
    V = rgbs.shape[0]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    met = torch.empty(V, 2, dtype=torch.float64, device=rgbs.device)
    s.record()
    if batched:
        image_metrics(rgbs, tgts, H, W, B, out=met)
    else:
        for k in range(V):
            image_metrics(rgbs[k], tgts[k], H, W, B, out=met[k:k + 1])
    e.record()
    host = met.cpu().numpy()                       # the one read-back (synchronises)
    return np.stack([psnr(host[:, 0]), host[:, 1]], 1), s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=249)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from codenerf_amd import _lib
    _lib.lib()                                     # no device: HipUnavailable, nothing is timed
    dev = torch.device("cuda", 0)
    H = W = a.size
    rgbs, tgts = make_views(a.views, H, W, dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    paths = {"host": lambda: (host_path(rgbs, tgts, H, W, a.chunk), None),
             "device": lambda: device_path(rgbs, tgts, H, W, a.chunk, False),
             "device_batched": lambda: device_path(rgbs, tgts, H, W, a.chunk, True)}
    results = {k: fn()[0] for k, fn in paths.items()}          # warm-up, and the numbers to compare
    torch.cuda.synchronize()
    walls, events = {k: [] for k in paths}, {k: [] for k in paths}
    for _ in range(a.reps):
        for k, fn in paths.items():
            (_, ev), ms = wall(fn)
            walls[k].append(ms)
            if ev is not None:
                events[k].append(ev)
    med = lambda x: round(statistics.median(x), 4)
    out = {"tool": "eval_metrics_time", "device": torch.cuda.get_device_name(0), "views": a.views, "H": H, "W": W,
           "chunk": a.chunk, "reps": a.reps,
           "host_wall_ms": med(walls["host"]), "device_wall_ms": med(walls["device"]),
           "device_event_ms": med(events["device"]),
           "device_batched_wall_ms": med(walls["device_batched"]),
           "device_batched_event_ms": med(events["device_batched"]),
           "host_ms_per_view": round(statistics.median(walls["host"]) / a.views, 5),
           "device_ms_per_view": round(statistics.median(walls["device"]) / a.views, 5),
           "speedup_wall": round(statistics.median(walls["host"]) / statistics.median(walls["device"]), 2),
           "max_psnr_diff_db": float(np.abs(results["host"][:, 0] - results["device"][:, 0]).max()),
           "max_ssim_diff": float(np.abs(results["host"][:, 1] - results["device"][:, 1]).max()),
           "batched_equals_per_view": bool(np.array_equal(results["device"], results["device_batched"])),
           "all_wall_ms": {k: [round(x, 3) for x in v] for k, v in walls.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
