"""Error of rendering through an occupancy grid, measured on a trained object.

Trains the srncar net on the synthetic SRN set (codenerf_amd.data.
make_synthetic_srn; Trainer = src/trainer.py's loop) at the C4-eval geometry
(128^2 views, focal 131.25, near / far 0.8 / 1.8, 64 coarse + 64 fine samples),
optimises the codes of one unseen object from one view (Optimizer, 200 steps),
and renders its evaluation views dense and, for every setting of the sweep

    tau in {1e-3, 1e-2, 1e-1, 1} x dilate in {0, 1, 2} x G in {64, 128}

through an OccupancyGrid built from the optimised shape code over the box
[-b, b]^3 for every b of --bounds (default (far - near) / 2, the Optimizer's
default).  Samples outside the box are culled whatever the grid holds, so the
rows of a bound whose grid is full (grid_fraction 1) show the error of the box
alone.  Per setting: the grid's set share, the
kept share of the samples, and against the DENSE RENDER OF THE SAME CODES the
worst and mean per-view |delta PSNR| (each view's PSNR against its ground
truth, sparse minus dense) and the largest |delta rgb| of any pixel.  Each view
uses one z jitter for all of its renders.  Prints one JSON line per setting and
a last line naming the setting with the smallest kept share whose worst
|delta PSNR| is at most --bar dB.  --state PATH also saves the
model, the codes and the test poses for tools/sparse_render_time.py.

  python tools/sparse_render_eval.py [--iters 3000] [--train_objs 8] [--views 250] [--precision bf16x3f]
                                     [--n_fine 64] [--num_opts 200] [--bar 0.005] [--bounds B ...] [--state PATH]
                                                                                                      (GPU)
"""
import argparse
import itertools
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TAUS, DILATES, GRIDS = (1e-3, 1e-2, 1e-1, 1.0), (0, 1, 2), (64, 128)


def hpams(root, precision, n_samples, n_fine, n_train_views, n_test_views):
    return {"net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "W": 256, "num_xyz_freq": 10,
                                "num_dir_freq": 4, "latent_dim": 256},
            "data": {"cat": "srn_cars", "splits": "cars_train", "data_dir": root, "n_train_views": n_train_views,
                     "n_test_views": n_test_views},
            "N_samples": n_samples, "N_importance": n_fine, "near": 0.8, "far": 1.8, "loss_reg_coef": 1e-4,
            "lr_schedule": [{"type": "step", "lr": 1e-4, "interval": 250000},
                            {"type": "step", "lr": 1e-3, "interval": 250000}],
            "check_points": 10 ** 9, "precision": precision}


def trained_object(a):
    """Train, optimise object 0 of the test split from its view 0 -> (Optimizer, hpams, eval views)."""
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.optimizer import Optimizer
    from codenerf_amd.trainer import Trainer
    tmp = tempfile.mkdtemp()
    root, exps = os.path.join(tmp, "data"), os.path.join(tmp, "exps")
    n_tv = 20
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=a.train_objs, n_views=n_tv, seed=5)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=a.views, seed=6)
    hp = hpams(root, a.precision, 64, a.n_fine, n_tv, a.views)
    torch.manual_seed(0)
    np.random.seed(0)
    tr = Trainer("t", 0, hpams=hp, batch_size=2048, check_iter=0, exp_root=exps)
    tr.training(0, a.iters, 1)
    ps = np.array(tr.psnr_log)
    print(json.dumps({"train_iters": a.iters, "train_psnr_first_epoch": round(float(ps[:a.train_objs].mean()), 2),
                      "train_psnr_last_epoch": round(float(ps[-a.train_objs:].mean()), 2)}), flush=True)
    opt = Optimizer("t", 0, [0], "test", hpams=hp, batch_size=2048, num_opts=a.num_opts, exp_root=exps,
                    device_metrics=True)
    opt.optimize_objs([0], lr=1e-2, lr_half_interval=50, save_img=False)
    print(json.dumps({"optimised_psnr_last_step": round(opt.psnr_opt[0][-1], 2),
                      "eval_psnr_mean_dense": round(float(np.mean(opt.psnr_eval[0])), 3)}), flush=True)
    return opt, hp


def psnr(img, gt):
    return -10.0 * torch.log10(((img.double() - gt.double()) ** 2).mean(dim=(1, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--train_objs", type=int, default=8)
    ap.add_argument("--views", type=int, default=250)
    ap.add_argument("--precision", default="bf16x3f")
    ap.add_argument("--n_fine", type=int, default=64)
    ap.add_argument("--num_opts", type=int, default=200)
    ap.add_argument("--bar", type=float, default=0.005)
    ap.add_argument("--bounds", type=float, nargs="+", default=None)
    ap.add_argument("--state", default=None)
    a = ap.parse_args()
    from codenerf_amd import _lib
    _lib.lib()                                     # no device: HipUnavailable
    from codenerf_amd.data import collate_one
    from codenerf_amd.occupancy import OccupancyGrid
    from codenerf_amd.utils import get_rays

    opt, hp = trained_object(a)
    dev, step, model = opt.device, opt.step_impl, opt.model
    shape = opt.optimized_shapecodes[0].to(dev)
    tex = opt.optimized_texturecodes[0].to(dev)
    focal, H, W, imgs, poses, _ = collate_one(opt.dataset[0])
    H, W = int(H), int(W)
    views = list(range(1, imgs.shape[1]))
    bounds = a.bounds or [(hp["far"] - hp["near"]) / 2]
    bound = bounds[0]
    if a.state:
        torch.save({"model": model.state_dict(), "shape": shape.cpu(), "texture": tex.cpu(), "poses": poses[0],
                    "focal": float(focal), "H": H, "W": W, "precision": a.precision, "bound": bound}, a.state)

    def render(rays, z, grid):
        if a.n_fine:
            return step.render_fine(rays[0], rays[1], z, a.n_fine, shape, tex, occupancy=grid)[0]
        return step.render(rays[0], rays[1], z, shape, tex, occupancy=grid)[0]

    with torch.no_grad():
        torch.manual_seed(1)
        rays = [get_rays(H, W, focal, poses[0, v]) for v in views]
        zs = [opt._z_vals() for _ in views]
        gts = torch.stack([imgs[0, v].reshape(-1, 3) for v in views]).to(dev)
        dense = torch.stack([render(r, z, None) for r, z in zip(rays, zs)])
        p_dense = psnr(dense, gts)
        rows = []
        for bound, G, tau, dilate in itertools.product(bounds, GRIDS, TAUS, DILATES):
            grid = OccupancyGrid.build(model, shape, G=G, bound=bound, tau=tau, dilate=dilate)
            kept, imgs_s = [], []
            for r, z in zip(rays, zs):
                imgs_s.append(render(r, z, grid))
                kc, kf, tot = step.last_sparse
                kept.append((kc + kf) / tot)
            sparse = torch.stack(imgs_s)
            dp = (psnr(sparse, gts) - p_dense).abs()
            row = {"bound": bound, "G": G, "tau": tau, "dilate": dilate, "grid_fraction": round(grid.fraction(), 5),
                   "kept_share": round(float(np.mean(kept)), 5),
                   "worst_abs_dpsnr_db": float(dp.max()), "mean_abs_dpsnr_db": float(dp.mean()),
                   "max_abs_drgb": float((sparse - dense).abs().max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    ok = [r for r in rows if r["worst_abs_dpsnr_db"] <= a.bar]
    best = min(ok, key=lambda r: r["kept_share"]) if ok else min(rows, key=lambda r: r["worst_abs_dpsnr_db"])
    print(json.dumps({"tool": "sparse_render_eval", "device": torch.cuda.get_device_name(0), "views": len(views),
                      "H": H, "W": W, "n_samples": 64, "n_fine": a.n_fine, "precision": a.precision, "bounds": bounds,
                      "bar_db": a.bar, "meets_bar": bool(ok), "dense_psnr_mean_db": float(p_dense.mean()),
                      "choice": best}))


if __name__ == "__main__":
    main()
