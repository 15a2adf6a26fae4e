"""Render edited objects on MI355X: code swaps and blends along a camera orbit,
with depth, median-depth, normal and opacity maps (the reference README's
"Editing Shapes/Textures"; it ships no code for it).

  python render.py --saved_dir srncar [--jsonfile srncar.json] [--gpu 0] [--codes PATH]
         --shape I [J] --texture I [J] [--frames K] [--azimuth A0 [A1]] [--elevation E]
         [--radius r] [--size 128] [--focal 131.25] [--n_importance N] [--aov True] [--out DIR]

--saved_dir names the training run under exps/ whose models.pth holds the
network and the code tables; --jsonfile its hyper-parameters (near, far,
N_samples, N_importance, the network, the precision).

--codes PATH takes the codes from a test-time run's codes.pth
(``optimized_shapecodes`` / ``optimized_texturecodes``; a path, or a path under
the run's directory) instead of the training tables.

--shape and --texture take one or two row indices of the tables.  One index is
that object's code; two are blended, frame k of K with weight k / (K - 1) (0
when K = 1), so the first frame shows I and the last J.  The shape of one
object with the texture of another is ``--shape 0 --texture 1``.

--frames K frames; --azimuth A0 [A1] degrees: frame k looks from
A0 + (A1 - A0) k / K (the end point is left out, so ``0 360`` loops; one value:
a fixed camera); --elevation degrees (default 20); --radius of the camera's
sphere around the origin (default 1.3); --size pixels per side and --focal of
the pinhole camera (defaults 128 and 131.25, SRN's cars).

--n_importance fine samples per ray; left out, the JSON's ``N_importance``
decides, as in optimize.py.  z is the fixed linspace(near, far, N_samples) and
the fine samples are the deterministic ones: frames are reproducible.

--aov True (default False) also writes, next to ``rgb_%03d.png``, the maps
``depth_`` (expected depth), ``depthmed_`` (median depth), ``normal_`` and
``alpha_`` (accumulated opacity) of every frame.

--out DIR (default exps/<saved_dir>/render) receives the PNGs and a
``frames.json`` with every frame's indices, blend weights and pose.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def build_parser():
    from codenerf_amd.utils import str2bool
    ap = argparse.ArgumentParser(description="CodeNeRF: render edited objects")
    ap.add_argument("--gpu", dest="gpu", type=int, default=0)
    ap.add_argument("--saved_dir", dest="saved_dir", default="srncar")
    ap.add_argument("--jsonfile", dest="jsonfile", default="srncar.json")
    ap.add_argument("--codes", dest="codes", default=None, help="a codes.pth to take the codes from")
    ap.add_argument("--shape", dest="shape", type=int, nargs="+", default=[0], help="one index, or two to blend")
    ap.add_argument("--texture", dest="texture", type=int, nargs="+", default=[0], help="one index, or two to blend")
    ap.add_argument("--frames", dest="frames", type=int, default=1)
    ap.add_argument("--azimuth", dest="azimuth", type=float, nargs="+", default=[0.0],
                    help="degrees: a fixed azimuth, or the start and the (excluded) end of a sweep")
    ap.add_argument("--elevation", dest="elevation", type=float, default=20.0)
    ap.add_argument("--radius", dest="radius", type=float, default=1.3)
    ap.add_argument("--size", dest="size", type=int, default=128)
    ap.add_argument("--focal", dest="focal", type=float, default=131.25)
    ap.add_argument("--n_importance", dest="n_importance", type=int, default=None,
                    help="fine samples per ray (default: the JSON's N_importance; 0: coarse only)")
    ap.add_argument("--aov", dest="aov", type=str2bool, default=False,
                    help="also write the depth, median-depth, normal and opacity maps")
    ap.add_argument("--out", dest="out", default=None, help="output directory (default exps/<saved_dir>/render)")
    return ap


def main(argv=None, exp_root="exps"):
    args = build_parser().parse_args(argv)
    for name in ("shape", "texture", "azimuth"):
        if len(getattr(args, name)) > 2:
            raise SystemExit(f"--{name} takes one or two values")
    import torch
    from codenerf_amd.edit import load_code_tables, render_edit
    from codenerf_amd.model import CodeNeRF
    from codenerf_amd.trainer import load_hpams
    hpams = load_hpams(args.jsonfile)
    device = torch.device("cuda", args.gpu)
    torch.cuda.set_device(device)
    saved = torch.load(os.path.join(exp_root, args.saved_dir, "models.pth"), map_location="cpu", weights_only=True)
    model = CodeNeRF(**hpams["net_hyperparams"], precision=hpams.get("precision", "fp32"))
    model.load_state_dict(saved["model_params"])
    model = model.to(device)
    shape_table, texture_table, ids = load_code_tables(args.saved_dir, exp_root, args.codes)
    for name, idx in (("shape", args.shape), ("texture", args.texture)):
        if not all(0 <= i < len(ids) for i in idx):
            raise SystemExit(f"--{name} {idx}: the tables hold {len(ids)} objects")
    n_fine = int(hpams.get("N_importance", 0) if args.n_importance is None else args.n_importance)
    out = args.out or os.path.join(exp_root, args.saved_dir, "render")
    meta = render_edit(model, shape_table, texture_table, args.shape, args.texture, out, frames=args.frames,
                       azimuth=args.azimuth, elevation=args.elevation, radius=args.radius, size=args.size,
                       focal=args.focal, near=hpams["near"], far=hpams["far"], n_samples=hpams["N_samples"],
                       n_fine=n_fine, aov=args.aov)
    print(f"{len(meta['frames'])} frames of shape {[ids[i] for i in args.shape]} / texture "
          f"{[ids[i] for i in args.texture]} -> {out}")
    return meta


if __name__ == "__main__":
    main()
