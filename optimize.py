"""Test-time code optimisation + evaluation on MI355X (reference CLI: optimize.py).

  python optimize.py --saved_dir srncar --tgt_instances 1 [--splits test]
         [--num_opts 200] [--lr 1e-2] [--lr_half_interval 50] [--save_img True]
         [--optimize_pose True [--pose_lr 1e-3] [--pose_noise_deg 0] [--pose_noise_trans 0]]
         [--n_importance N] [--device_metrics True]
         [--mask {none,white,files} [--bg_weight 0] [--sil_coef 0]]
         [--sparse_eval True [--occ_grid 128] [--occ_tau 1e-1] [--occ_dilate 2] [--occ_bound B]]
         [--save_mesh True --mesh_iso S [--mesh_grid 128] [--mesh_bound B]]

--optimize_pose (no reference counterpart) refines every target view's camera
pose together with the codes; the two noise flags perturb the dataset poses it
starts from (SRN ships ground-truth poses).

--n_importance sets the fine samples per ray of the hierarchical (coarse +
fine) renderer; left out, the JSON's ``N_importance`` decides, as in training.
Above 0 every optimisation step (codes, and poses with --optimize_pose) runs
through the fine pass and the evaluation views are rendered with it, with the
deterministic fine samples u_j = (j + 0.5) / N; 0 is the coarse-only loop.

--device_metrics True (default False; no reference counterpart) computes the
evaluation views' PSNR argument and SSIM with the device kernel
(cn_image_metrics) and reads an object's results back once after its last
view, instead of the per-view host metrics; the outputs keep their shape.

--mask (default none; no reference counterpart in code -- the paper's
real-image experiments mask the loss) weights the image loss of the target
views per ray: ``white`` takes every pixel with a channel below 1.0 as
foreground (SRN's white background), ``files`` reads the object's ``mask/``
directory (PNGs named like ``rgb/``, nonzero = foreground).  A foreground ray
weighs 1, a background ray --bg_weight (default 0: background, occluder and
clutter pixels pull neither the codes nor the pose).  --sil_coef (default 0)
adds coef x mean (accumulated opacity - mask)^2 over the rays, the silhouette
term.  The evaluation views are scored unmasked; ``none`` is the plain loop.

--sparse_eval True (default False; no reference counterpart) renders the
evaluation views through an occupancy grid built once per object from its
optimised shape code: --occ_grid cells per axis over [-B, B]^3 (--occ_bound,
default (far - near) / 2), a cell set when the density at its centre reaches
--occ_tau, dilated by --occ_dilate cells.  Samples in empty cells are not
evaluated (density and colour 0); the optimisation steps are untouched.

--save_mesh True (default False; no reference counterpart) writes a coloured
triangle mesh of every optimised object to <save_dir>/<obj_id>/mesh.ply: the
surface where the density equals --mesh_iso (required: it has no default) on a
lattice of --mesh_grid points per axis over [-B, B]^3 (--mesh_bound, default
(far - near) / 2), by marching tetrahedra, with per-vertex normals and colours.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def build_parser():
    from codenerf_amd.utils import str2bool
    ap = argparse.ArgumentParser(description="CodeNeRF")
    ap.add_argument("--gpu", dest="gpu", default=0)
    ap.add_argument("--saved_dir", dest="saved_dir", default="srncar")
    ap.add_argument("--tgt_instances", dest="tgt_instances", nargs="+", default=[1])
    ap.add_argument("--splits", dest="splits", default="test")
    ap.add_argument("--num_opts", dest="num_opts", default=200)
    ap.add_argument("--lr", dest="lr", default=1e-2)
    ap.add_argument("--lr_half_interval", dest="lr_half_interval", default=50)
    ap.add_argument("--save_img", dest="save_img", default=True)
    ap.add_argument("--jsonfile", dest="jsonfile", default="srncar.json")
    ap.add_argument("--batchsize", dest="batchsize", default=2048)
    ap.add_argument("--optimize_pose", dest="optimize_pose", type=str2bool, default=False,
                    help="refine the target views' camera poses together with the codes")
    ap.add_argument("--pose_lr", dest="pose_lr", type=float, default=1e-3)
    ap.add_argument("--pose_noise_deg", dest="pose_noise_deg", type=float, default=0.0,
                    help="rotate each starting pose by this many degrees about a seeded axis")
    ap.add_argument("--pose_noise_trans", dest="pose_noise_trans", type=float, default=0.0,
                    help="shift each starting pose by this length times a seeded normal vector")
    ap.add_argument("--n_importance", dest="n_importance", type=int, default=None,
                    help="fine samples per ray (default: the JSON's N_importance; 0: coarse only)")
    ap.add_argument("--device_metrics", dest="device_metrics", type=str2bool, default=False,
                    help="evaluation PSNR / SSIM on the device, one read-back per object")
    ap.add_argument("--mask", dest="mask", choices=["none", "white", "files"], default="none",
                    help="per-ray weights of the target views' loss: foreground from the white "
                         "background or from the object's mask/ directory")
    ap.add_argument("--bg_weight", dest="bg_weight", type=float, default=0.0,
                    help="weight of a background ray under --mask (foreground rays weigh 1)")
    ap.add_argument("--sil_coef", dest="sil_coef", type=float, default=0.0,
                    help="coefficient of the silhouette term (accumulated opacity against the mask)")
    ap.add_argument("--sparse_eval", dest="sparse_eval", type=str2bool, default=False,
                    help="render the evaluation views through an occupancy grid of the optimised shape code")
    ap.add_argument("--occ_grid", dest="occ_grid", type=int, default=None, help="grid cells per axis")
    ap.add_argument("--occ_tau", dest="occ_tau", type=float, default=None,
                    help="a cell is occupied when the density at its centre reaches this")
    ap.add_argument("--occ_dilate", dest="occ_dilate", type=int, default=None,
                    help="dilate the occupied cells by this many cells (0 to 4)")
    ap.add_argument("--occ_bound", dest="occ_bound", type=float, default=None,
                    help="half edge of the grid's box around the origin (default (far - near) / 2)")
    ap.add_argument("--save_mesh", dest="save_mesh", type=str2bool, default=False,
                    help="write a coloured mesh.ply of every optimised object")
    ap.add_argument("--mesh_grid", dest="mesh_grid", type=int, default=None, help="lattice points per axis")
    ap.add_argument("--mesh_iso", dest="mesh_iso", type=float, default=None,
                    help="density of the extracted surface (required with --save_mesh)")
    ap.add_argument("--mesh_bound", dest="mesh_bound", type=float, default=None,
                    help="half edge of the lattice's box around the origin (default (far - near) / 2)")
    return ap


def main():
    from codenerf_amd.utils import str2bool
    args = build_parser().parse_args()

    from codenerf_amd.optimizer import Optimizer
    tgt = [int(i) for i in args.tgt_instances]
    opt = Optimizer(args.saved_dir, int(args.gpu), tgt, args.splits, args.jsonfile, int(args.batchsize),
                    int(args.num_opts), n_importance=args.n_importance, device_metrics=args.device_metrics,
                    mask=None if args.mask == "none" else args.mask, bg_weight=args.bg_weight,
                    sil_coef=args.sil_coef, sparse_eval=args.sparse_eval, occ_bound=args.occ_bound,
                    save_mesh=args.save_mesh, mesh_iso=args.mesh_iso, mesh_bound=args.mesh_bound,
                    **{k: getattr(args, k) for k in ("occ_grid", "occ_tau", "occ_dilate", "mesh_grid")
                       if getattr(args, k) is not None})
    if args.optimize_pose:
        noise = (args.pose_noise_deg, args.pose_noise_trans) if args.pose_noise_deg or args.pose_noise_trans else None
        opt.optimize_objs(tgt, float(args.lr), int(args.lr_half_interval), str2bool(args.save_img),
                          optimize_pose=True, pose_lr=args.pose_lr, pose_noise=noise)
    else:
        opt.optimize_objs(tgt, float(args.lr), int(args.lr_half_interval), str2bool(args.save_img))


if __name__ == "__main__":
    main()
