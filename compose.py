"""Compose several trained objects into one scene on MI355X: each object with
its own codes, position, heading and size, occluding the others correctly, with
the instance map, the opacity and the depth of every frame.

  python compose.py --saved_dir srncar [--jsonfile srncar.json] [--gpu 0] [--codes PATH]
         --scene FILE [--frames K] [--azimuth A0 [A1]] [--elevation E] [--radius r]
         [--size 128] [--focal 131.25] [--near N] [--far F] [--n_samples N]
         [--n_importance N] [--labels True] [--out DIR]

--saved_dir names the training run under exps/ whose models.pth holds the
network and the code tables; --jsonfile its hyper-parameters (N_samples,
N_importance, the network, the precision).  --codes PATH takes the codes from a
test-time run's codes.pth instead of the training tables, as render.py does.

--scene FILE is a JSON scene file (codenerf_amd/scene.py)::

    {"objects": [{"shape": 0, "texture": 0, "translation": [0.3, 0, 0],
                  "rotation_deg": [30, 0, 0], "scale": 1.0, "bound": 0.5}, ...]}

with 1 to 8 objects.  ``shape`` / ``texture``: a row of the tables, or
``[i, j, t]`` for a blend; ``rotation_deg``: yaw, pitch, roll; ``bound``: half
the side of the object's box, outside which it contributes nothing; optional
``occ_grid`` / ``occ_tau`` / ``occ_dilate`` of its occupancy grid.

The camera orbits the world origin: --frames K frames; --azimuth A0 [A1]
degrees: frame k looks from A0 + (A1 - A0) k / K (one value: a fixed camera);
--elevation degrees (default 20); --radius of the camera's sphere (default 1.3);
--size pixels per side and --focal of the pinhole camera (defaults 128 and
131.25).  --near / --far default to the scene's depth range at that radius
(``Scene.depth_range``); --n_samples and --n_importance default to the JSON's
``N_samples`` and ``N_importance``.  z is the fixed linspace(near, far,
n_samples) and the fine samples are the deterministic ones: frames are
reproducible.

--labels True (the default) also writes, next to ``rgb_%03d.png``:
``instance_%03d.png`` (uint8: object index + 1, 0 = background),
``alpha_%03d.png`` (accumulated opacity) and ``depth_%03d.png`` (expected depth
over [near, far]).

--out DIR (default exps/<saved_dir>/compose) receives the PNGs and a
``scene_frames.json`` with every frame's pose, the scene as read and each
object's grid fraction.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def build_parser():
    from codenerf_amd.utils import str2bool
    ap = argparse.ArgumentParser(description="CodeNeRF: compose several objects into one scene")
    ap.add_argument("--gpu", dest="gpu", type=int, default=0)
    ap.add_argument("--saved_dir", dest="saved_dir", default="srncar")
    ap.add_argument("--jsonfile", dest="jsonfile", default="srncar.json")
    ap.add_argument("--codes", dest="codes", default=None, help="a codes.pth to take the codes from")
    ap.add_argument("--scene", dest="scene", required=True, help="the JSON scene file")
    ap.add_argument("--frames", dest="frames", type=int, default=1)
    ap.add_argument("--azimuth", dest="azimuth", type=float, nargs="+", default=[0.0],
                    help="degrees: a fixed azimuth, or the start and the (excluded) end of a sweep")
    ap.add_argument("--elevation", dest="elevation", type=float, default=20.0)
    ap.add_argument("--radius", dest="radius", type=float, default=1.3)
    ap.add_argument("--size", dest="size", type=int, default=128)
    ap.add_argument("--focal", dest="focal", type=float, default=131.25)
    ap.add_argument("--near", dest="near", type=float, default=None, help="default: the scene's depth range")
    ap.add_argument("--far", dest="far", type=float, default=None, help="default: the scene's depth range")
    ap.add_argument("--n_samples", dest="n_samples", type=int, default=None,
                    help="coarse samples per ray (default: the JSON's N_samples)")
    ap.add_argument("--n_importance", dest="n_importance", type=int, default=None,
                    help="fine samples per ray (default: the JSON's N_importance; 0: coarse only)")
    ap.add_argument("--labels", dest="labels", type=str2bool, default=True,
                    help="also write the instance, opacity and depth maps")
    ap.add_argument("--out", dest="out", default=None, help="output directory (default exps/<saved_dir>/compose)")
    return ap


def render_scene_frames(model, scene, desc, out_dir, frames=1, azimuth=(0.0,), elevation=20.0, radius=1.3, size=128,
                        focal=131.25, near=None, far=None, n_samples=64, n_fine=0, labels=True):
    """Render the frames into out_dir and write scene_frames.json -> its content."""
    import numpy as np
    from PIL import Image
    from codenerf_amd.edit import aov_to_uint8, frame_plan, orbit_pose, rgb_to_uint8
    from codenerf_amd.render import ImageStep
    from codenerf_amd.utils import get_rays, stratified_z
    dev = next(model.parameters()).device
    step = ImageStep(model)
    H = W = int(size)
    lo, hi = scene.depth_range(radius)
    near, far = float(lo if near is None else near), float(hi if far is None else far)
    z = stratified_z(near, far, int(n_samples), z_fixed=True).to(dev)
    os.makedirs(out_dir, exist_ok=True)
    record, kept = [], []
    for k, (_, _, az) in enumerate(frame_plan(frames, (0,), (0,), azimuth)):
        pose = orbit_pose(radius, az, elevation)
        rays_o, viewdir = get_rays(H, W, float(focal), pose.to(dev))
        out = step.render_scene(rays_o, viewdir, z, scene, n_fine=int(n_fine), labels=bool(labels))
        img = lambda a: a.reshape(H, W, -1).squeeze(-1).cpu().numpy()
        save = lambda arr, stem: Image.fromarray(arr).save(os.path.join(out_dir, f"{stem}_{k:03d}.png"))
        save(rgb_to_uint8(img(out["rgb"])), "rgb")
        if labels:
            save((img(out["instance"]) + 1).astype(np.uint8), "instance")
            save(aov_to_uint8("acc", img(out["acc"])), "alpha")
            save(aov_to_uint8("depth", img(out["depth"]), near, far), "depth")
        kc, kf, total = step.last_sparse
        kept.append((kc + kf) / total)
        record.append(dict(frame=k, azimuth=az, elevation=float(elevation), radius=float(radius), pose=pose.tolist(),
                           kept=kept[-1]))
    meta = dict(size=H, focal=float(focal), near=near, far=far, n_samples=int(n_samples), n_importance=int(n_fine),
                labels=bool(labels), scene=desc, grid_fraction=[o.grid.fraction() for o in scene.objects],
                frames=record)
    with open(os.path.join(out_dir, "scene_frames.json"), "w") as f:
        json.dump(meta, f, indent=2)
    return meta


def main(argv=None, exp_root="exps"):
    args = build_parser().parse_args(argv)
    if len(args.azimuth) > 2:
        raise SystemExit("--azimuth takes one or two values")
    import torch
    from codenerf_amd.edit import load_code_tables
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.scene import load_scene
    from codenerf_amd.trainer import load_hpams
    hpams = load_hpams(args.jsonfile)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    saved = torch.load(os.path.join(exp_root, args.saved_dir, "models.pth"), map_location="cpu", weights_only=True)
    model = CodeNeRF(**hpams["net_hyperparams"], precision=hpams.get("precision", "fp32"))
    model.load_state_dict(saved["model_params"])
    model = model.to(device)
    shape_table, texture_table, ids = load_code_tables(args.saved_dir, exp_root, args.codes)
    try:
        scene, desc = load_scene(args.scene, shape_table, texture_table, model)
    except ValueError as err:
        raise SystemExit(f"--scene {args.scene}: {err}")
    n_samples = int(hpams["N_samples"] if args.n_samples is None else args.n_samples)
    n_fine = int(hpams.get("N_importance", 0) if args.n_importance is None else args.n_importance)
    out = args.out or os.path.join(exp_root, args.saved_dir, "compose")
    meta = render_scene_frames(model, scene, desc, out, frames=args.frames, azimuth=args.azimuth,
                               elevation=args.elevation, radius=args.radius, size=args.size, focal=args.focal,
                               near=args.near, far=args.far, n_samples=n_samples, n_fine=n_fine, labels=args.labels)
    print(f"{len(meta['frames'])} frames of {len(scene)} objects -> {out}")
    return meta


if __name__ == "__main__":
    main()
