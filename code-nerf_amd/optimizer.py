"""Test-time code optimisation and evaluation on the HIP path
(reference: src/optimizer.py; BASELINE config 4).

Same API (``Optimizer(saved_dir, gpu, instance_ids, splits, jsonfile,
batch_size, num_opts).optimize_objs(instance_ids, lr, lr_half_interval,
save_img)``) and loop semantics:

  * codes start at the mean of the trained code tables (:232-233) and only
    the two codes are optimised (AdamW, lr halved every ``lr_half_interval``
    steps by re-creating the optimiser, :104-105,207-218);
  * one step = zero_grad, then every target view's image (chunked MSE + the
    code regulariser on each view's chunk 0) accumulates gradients, then
    one AdamW step (:66-98);
  * evaluation: every view that is not a target, forward only, PSNR from the
    mean of the chunk MSEs and SSIM (:108-130); with torch.distributed the
    views are split across ranks (dp.shard) and the metrics gathered
    (dp.gather_by_key), the z jitter of every view drawn first in view order
    so a split changes no draw;
  * ``codes.pth`` with the reference's keys (:138-145).
With ``N_importance`` > 0 in the JSON (or ``n_importance=``; no reference
counterpart) the steps and the evaluation run the coarse + fine renderer the
model was trained with: ``ImageStep.forward_backward_fine(weight_grads=False)``
with fresh fine draws per view and step, the logged PSNR and the saved image
from the fine composite, and ``ImageStep.render_fine`` with its deterministic
fine samples for the evaluation views.  At 0 nothing below changes.
The model weights are fixed, so the weight-gradient pass is skipped (only the
dX chain and the code gradients run).  SSIM is ``metrics.ssim_legacy`` -- a
restatement of skimage's ``structural_similarity(multichannel=True)`` as the
reference calls it (skimage is not installed: parity unpinned).
``device_metrics=True`` (no reference counterpart) computes each evaluation
view's chunk-mean MSE and that SSIM with ``metrics.image_metrics`` on the
device and reads all of an object's views back at once, instead of one host
synchronisation per chunk, two image copies and a numpy SSIM per view; the
dictionaries and ``codes.pth`` keep their shape and keys.
``mask`` (no reference counterpart in code; the paper's real-image experiments
mask the loss) weights the target views' loss per ray and, with ``sil_coef``,
supervises the accumulated opacity: ``"white"`` takes a pixel as foreground
when any channel of the target is below 1.0 (SRN's white background),
``"files"`` reads the object's ``mask/`` directory.  Target views only:
ray_weight = fg + bg_weight (1 - fg), acc_target = fg, through
``ImageStep.forward_backward[_fine](ray_weight=, acc_target=, sil_coef=)``.
``psnr_opt`` then logs -10 log10 of the MASKED loss's value (weighted MSE +
silhouette term over all pixels of the chunk), not a PSNR of the image; the
evaluation views are scored unmasked.  ``mask=None`` is exactly the loop above.
``sparse_eval=True`` (no reference counterpart) renders the evaluation views
through an occupancy grid (``occupancy.OccupancyGrid``): once an
object's codes are final, one grid of ``occ_grid``^3 cells over the box
[-occ_bound, occ_bound]^3 (None: (far - near) / 2, the radius the sample range
covers around the origin) is built from its optimised shape code (density >=
``occ_tau``, dilated by ``occ_dilate`` cells), and every evaluation view, on
either metrics path, evaluates the MLP only at the samples in its set cells.
Samples outside the box are culled whatever the grid holds, and the default
box holds the sample range of the central ray only: a model with density
beyond it needs a larger ``occ_bound`` (DESIGN.md 8.4 has the figures).
The optimisation steps are untouched: the codes move, so no grid is valid for
them.  The grid's set share and the mean kept share of the samples are left in
``occ_fraction`` / ``occ_kept`` per object; ``codes.pth`` keeps its keys.
``save_mesh=True`` (no reference counterpart) writes, after each object's
optimisation, ``<save_dir>/<obj_id>/mesh.ply``: the surface density =
``mesh_iso`` of the optimised codes on a ``mesh_grid``^3 lattice over
[-mesh_bound, mesh_bound]^3 (None: (far - near) / 2, as the occupancy box),
with normals and colours (``mesh.extract_mesh``).  ``mesh_iso``
has no default: no value has been measured on a real model.  Nothing else
changes: the mesh is taken after the evaluation, on rank 0.
"""
import json
import os
import time

import numpy as np
import torch

from . import dp
from .data import SRN, collate_one
from .mesh import extract_mesh, write_ply
from .metrics import image_metrics, psnr as mse_to_psnr, ssim_legacy
from .model import CodeNeRF
from .occupancy import OccupancyGrid
from .optim import FusedAdamW
from .pose import PoseParam, perturb_pose
from .render import ImageStep
from .trainer import load_hpams
from .utils import get_rays, image_float_to_uint8


# Defaults of the evaluation grid (sparse_eval): DESIGN.md 8.4 has the sweep they come from.
OCC_GRID, OCC_TAU, OCC_DILATE = 128, 1e-1, 2


class Optimizer:
    def __init__(self, saved_dir, gpu=0, instance_ids=(), splits="test", jsonfile="srncar.json",
                 batch_size=2048, num_opts=200, hpams=None, exp_root="exps", dist=None, n_importance=None,
                 device_metrics=False, mask=None, bg_weight=0.0, sil_coef=0.0, sparse_eval=False, occ_grid=OCC_GRID,
                 occ_tau=OCC_TAU, occ_dilate=OCC_DILATE, occ_bound=None, save_mesh=False, mesh_grid=128,
                 mesh_iso=None, mesh_bound=None):
        self.hpams = hpams if hpams is not None else load_hpams(jsonfile)
        # fine samples per ray (the JSON's N_importance, as Trainer reads it;
        # n_importance overrides it); 0: the reference's coarse-only loop
        self.n_fine = int(self.hpams.get("N_importance", 0) if n_importance is None else n_importance)
        # evaluation PSNR / SSIM from the device kernel (metrics.image_metrics),
        # one read-back per object; off: the host loop below, as the reference
        self.device_metrics = bool(device_metrics)
        if mask not in (None, "white", "files"):
            raise ValueError(f"mask must be None, 'white' or 'files', got {mask!r}")
        # per-ray weights / opacity targets of the target views (module docstring)
        self.mask, self.bg_weight, self.sil_coef = mask, float(bg_weight), float(sil_coef)
        if self.bg_weight < 0 or self.sil_coef < 0:
            raise ValueError("bg_weight and sil_coef must not be negative")
        # evaluation views through an occupancy grid of the optimised shape code (module docstring)
        self.sparse_eval = bool(sparse_eval)
        self.occ_grid, self.occ_tau, self.occ_dilate = int(occ_grid), float(occ_tau), int(occ_dilate)
        self.occ_bound = None if occ_bound is None else float(occ_bound)
        if not self.occ_tau >= 0:
            raise ValueError("occ_tau must not be negative")
        if not 0 <= self.occ_dilate <= 4:
            raise ValueError("occ_dilate must be in [0, 4]")
        if self.occ_grid % 32 or not 32 <= self.occ_grid <= 256:
            raise ValueError("occ_grid must be a multiple of 32 in [32, 256]")
        if self.occ_bound is not None and not self.occ_bound > 0:
            raise ValueError("occ_bound must be positive")
        self.occ_fraction, self.occ_kept = {}, {}
        # a coloured mesh of every optimised object (module docstring)
        self.save_mesh = bool(save_mesh)
        self.mesh_grid = int(mesh_grid)
        self.mesh_iso = None if mesh_iso is None else float(mesh_iso)
        self.mesh_bound = None if mesh_bound is None else float(mesh_bound)
        if self.save_mesh and self.mesh_iso is None:
            raise ValueError("save_mesh needs mesh_iso: the density of the surface has no default")
        if self.mesh_iso is not None and not np.isfinite(self.mesh_iso):
            raise ValueError("mesh_iso must be finite")
        if not 2 <= self.mesh_grid <= 512:
            raise ValueError("mesh_grid must be in [2, 512]")
        if self.mesh_bound is not None and not (self.mesh_bound > 0 and np.isfinite(self.mesh_bound)):
            raise ValueError("mesh_bound must be positive")
        self.mesh_counts = {}
        self.device = torch.device("cuda", int(gpu))
        torch.cuda.set_device(self.device)
        self.exp_root = exp_root
        self.dist = dist
        self.world, self.rank = dp.world_rank(dist)
        self.make_model()
        self.load_model_codes(saved_dir)
        self.make_dataloader(splits, len(instance_ids))
        self.B = int(batch_size)
        self.num_opts = int(num_opts)
        self.splits = splits
        self.nviews = str(len(instance_ids))
        self.psnr_eval, self.psnr_opt, self.ssim_eval = {}, {}, {}
        self.step_impl = ImageStep(self.model, chunk=self.B, reg_coef=self.hpams["loss_reg_coef"])

    def _z_vals(self):
        near, far, N = self.hpams["near"], self.hpams["far"], self.hpams["N_samples"]
        half = (far - near) / (2 * N)
        z = torch.linspace(near + half, far - half, N)
        z += torch.rand(N) * (far - near) / (2 * N)
        return z.to(self.device)

    def optimize_objs(self, instance_ids, lr=1e-2, lr_half_interval=50, save_img=True, optimize_pose=False,
                      pose_lr=1e-3, pose_noise=None):
        """optimize_pose (no reference counterpart): every target view's
        camera pose is refined together with the codes -- one ``PoseParam``
        per view, started at the dataset pose (SRN ships ground-truth poses,
        so ``pose_noise = (rotation in degrees, translation[, seed])``
        perturbs the start), each in an AdamW group of its own at ``pose_lr``,
        halved on the codes' schedule.  codes.pth then also holds
        ``optimized_poses`` and the per-view rotation (degrees) / translation
        error against the dataset pose.  Off: exactly the reference loop."""
        self.optimize_pose = bool(optimize_pose)
        self.pose_lr = float(pose_lr)
        self.pose_params = []
        self.optimized_poses, self.pose_rot_err, self.pose_trans_err = {}, {}, {}
        if self.rank == 0:
            with open(os.path.join(self.save_dir, "opt_hpams.json"), "w") as f:
                json.dump({"instance_ids": list(map(int, instance_ids)), "lr": lr,
                           "lr_half_interval": lr_half_interval, "": self.splits}, f, indent=2)
        self.lr, self.lr_half_interval = lr, lr_half_interval
        instance_ids = [int(i) for i in instance_ids]
        n = len(self.dataset)
        self.optimized_shapecodes = torch.zeros(n, self.mean_shape.shape[1])
        self.optimized_texturecodes = torch.zeros(n, self.mean_texture.shape[1])
        for num_obj in range(n):
            focal, H, W, imgs, poses, obj_idx = collate_one(self.dataset[num_obj])
            H, W = int(H), int(W)
            fgs = self._foreground(num_obj, imgs, instance_ids)
            self.nopts = 0
            shapecode = self.mean_shape.to(self.device).clone().detach().requires_grad_()
            texturecode = self.mean_texture.to(self.device).clone().detach().requires_grad_()
            if self.optimize_pose:
                self.pose_params = [self._start_pose(poses[0, iid], pose_noise, num)
                                    for num, iid in enumerate(instance_ids)]
            self.set_optimizers(shapecode, texturecode)
            while self.nopts < self.num_opts:
                shapecode.grad = torch.zeros_like(shapecode)
                texturecode.grad = torch.zeros_like(texturecode)
                for pp in self.pose_params:
                    pp.delta.grad = torch.zeros_like(pp.delta)
                t1 = time.time()
                gens, gts = [], []
                for num, iid in enumerate(instance_ids):
                    tgt_img = imgs[0, iid].reshape(-1, 3).to(self.device)
                    pp = self.pose_params[num] if self.optimize_pose else None
                    rays_o, viewdir = pp.rays(H, W, focal) if pp else get_rays(H, W, focal, poses[0, iid])
                    z_c = self._z_vals()
                    kw = {}
                    if fgs is not None:
                        fg = fgs[num]
                        kw = dict(ray_weight=fg + self.bg_weight * (1 - fg), acc_target=fg, sil_coef=self.sil_coef)
                    if self.n_fine > 0:
                        # the coarse + fine step the model was trained with,
                        # codes only; the logged loss and the image are the fine ones
                        rand_f = torch.rand(H * W, self.n_fine, device=self.device)
                        _, losses, rgb, reg = self.step_impl.forward_backward_fine(
                            rays_o, viewdir, z_c, rand_f, tgt_img, shapecode, texturecode, 0, weight_grads=False,
                            input_grads=pp is not None, **kw)
                    else:
                        losses, rgb, reg = self.step_impl.forward_backward(
                            rays_o, viewdir, z_c, tgt_img, shapecode, texturecode, 0, weight_grads=False,
                            input_grads=pp is not None, **kw)
                    if pp:
                        pp.backward_from_ray_grads(self.step_impl.last_ray_grads)
                    gens.append(rgb.reshape(H, W, 3))
                    gts.append(tgt_img.reshape(H, W, 3))
                self.opts.step()
                self.log_opt_psnr(float(losses.mean()), time.time() - t1, num_obj)
                if save_img and self.rank == 0:
                    self.save_img(gens, gts, self.ids[num_obj], self.nopts)
                self.nopts += 1
                if self.nopts % lr_half_interval == 0:
                    self.set_optimizers(shapecode, texturecode)
            with torch.no_grad():
                # evaluation views (src/optimizer.py:108-130), split across
                # ranks when data parallel; the z jitter of every view is drawn
                # first, in view order, so the split does not change any draw
                views = [num for num in range(imgs.shape[1]) if num not in instance_ids]
                zs = {num: self._z_vals() for num in views}
                local = {}
                mine = dp.shard(views, self.dist)
                grid, kept = None, []
                if self.sparse_eval and mine:
                    bound = self.occ_bound if self.occ_bound is not None else \
                        (self.hpams["far"] - self.hpams["near"]) / 2
                    grid = OccupancyGrid.build(self.model, shapecode, G=self.occ_grid, bound=bound, tau=self.occ_tau,
                                               dilate=self.occ_dilate)
                if self.device_metrics:
                    # (mse, ssim) of every local view, read back once after the last
                    met = torch.empty(len(mine), 2, dtype=torch.float64, device=self.device)
                for k, num in enumerate(mine):
                    tgt_img = imgs[0, num].reshape(-1, 3).to(self.device)
                    rays_o, viewdir = get_rays(H, W, focal, poses[0, num])
                    if self.n_fine > 0:
                        # deterministic fine samples: the split changes no result
                        rgb, _ = self.step_impl.render_fine(rays_o, viewdir, zs[num], self.n_fine, shapecode,
                                                            texturecode, occupancy=grid)
                    else:
                        rgb, _ = self.step_impl.render(rays_o, viewdir, zs[num], shapecode, texturecode,
                                                       occupancy=grid)
                    if grid is not None:
                        kc, kf, tot = self.step_impl.last_sparse
                        kept.append((kc + kf) / tot)
                    if self.device_metrics:
                        image_metrics(rgb, tgt_img, H, W, self.B, out=met[k:k + 1])
                    else:
                        se = ((rgb - tgt_img) ** 2).sum(-1)
                        chunk_mse = [float(se[i:i + self.B].mean()) / 3 for i in range(0, H * W, self.B)]
                        local[num] = (float(-10 * np.log(float(np.mean(chunk_mse))) / np.log(10)),
                                      ssim_legacy(rgb.reshape(H, W, 3).cpu().numpy(),
                                                  tgt_img.reshape(H, W, 3).cpu().numpy()))
                    if save_img:
                        self.save_img([rgb.reshape(H, W, 3)], [tgt_img.reshape(H, W, 3)], self.ids[num_obj], num,
                                      opt=False)
                if self.device_metrics:
                    for num, (mse, ssim) in zip(mine, met.cpu().tolist()):
                        local[num] = (float(mse_to_psnr(mse)), ssim)
                if grid is not None:
                    self.occ_fraction[num_obj] = grid.fraction()
                    self.occ_kept[num_obj] = float(np.mean(kept))
                    print(f"object {num_obj}: occupancy grid {self.occ_grid}^3, {self.occ_fraction[num_obj]:.4f} of "
                          f"the cells set, {self.occ_kept[num_obj]:.4f} of the samples kept over {len(kept)} views")
                for num, (psnr, ssim) in dp.gather_by_key(local, self.dist).items():
                    self.psnr_eval.setdefault(num_obj, []).append(psnr)
                    self.ssim_eval.setdefault(num_obj, []).append(ssim)
            self.optimized_shapecodes[num_obj] = shapecode.detach().cpu()
            self.optimized_texturecodes[num_obj] = texturecode.detach().cpu()
            if self.optimize_pose:
                errs = [pp.errors(poses[0, iid]) for pp, iid in zip(self.pose_params, instance_ids)]
                with torch.no_grad():
                    self.optimized_poses[num_obj] = torch.stack([pp.c2w().cpu() for pp in self.pose_params])
                self.pose_rot_err[num_obj] = [e[0] for e in errs]
                self.pose_trans_err[num_obj] = [e[1] for e in errs]
            self.save_opts(num_obj)
            if self.save_mesh and self.rank == 0:
                self.write_mesh(num_obj, shapecode, texturecode)

    def write_mesh(self, num_obj, shapecode, texturecode):
        """<save_dir>/<obj_id>/mesh.ply of the optimised codes (module docstring)."""
        bound = self.mesh_bound if self.mesh_bound is not None else (self.hpams["far"] - self.hpams["near"]) / 2
        m = extract_mesh(self.model, shapecode, texturecode, n=self.mesh_grid, bound=bound, iso=self.mesh_iso)
        d = os.path.join(self.save_dir, str(self.ids[num_obj]))
        os.makedirs(d, exist_ok=True)
        write_ply(os.path.join(d, "mesh.ply"), m.verts, m.tris, m.normals, m.colors)
        self.mesh_counts[num_obj] = (int(m.verts.shape[0]), int(m.tris.shape[0]))
        print(f"object {num_obj}: mesh at density {self.mesh_iso:g} on {self.mesh_grid}^3 points: "
              f"{m.verts.shape[0]} vertices, {m.tris.shape[0]} triangles")

    def _foreground(self, num_obj, imgs, instance_ids):
        """Foreground {0, 1} of every target view, (H*W,) each on the device,
        in instance_ids order; None without a mask."""
        if self.mask is None:
            return None
        if self.mask == "files":
            m = self.dataset.masks(self.ids[num_obj])
            if m is None:
                raise FileNotFoundError(f"mask='files': object {self.ids[num_obj]} has no mask/ directory under "
                                        f"{self.dataset.data_dir}")
            if tuple(m.shape[1:]) != tuple(imgs.shape[2:4]):
                raise ValueError(f"mask='files': masks of {self.ids[num_obj]} are {tuple(m.shape[1:])}, the images "
                                 f"{tuple(imgs.shape[2:4])}")
            fg = [m[iid] for iid in instance_ids]
        else:
            fg = [(imgs[0, iid] < 1.0).any(-1).float() for iid in instance_ids]
        return [f.reshape(-1).to(self.device) for f in fg]

    def _start_pose(self, c2w, pose_noise, view):
        """PoseParam of one target view: the dataset pose, perturbed by
        pose_noise = (degrees, translation[, seed]) (seed + view index)."""
        c = c2w.reshape(4, 4).to(torch.float32)
        if pose_noise is not None:
            deg, trans = float(pose_noise[0]), float(pose_noise[1])
            seed = int(pose_noise[2]) if len(pose_noise) > 2 else 0
            c = perturb_pose(c, deg, trans, seed + view)
        return PoseParam(c.to(self.device))

    def set_optimizers(self, shapecode, texturecode):
        k = 2 ** (-(self.nopts // self.lr_half_interval))
        lr = self.lr * k
        groups = [{"params": [shapecode], "lr": lr}, {"params": [texturecode], "lr": lr}]
        # pose refinement: one group per view, no decay (it would pull the pose back to its start)
        groups += [{"params": [pp.delta], "lr": self.pose_lr * k, "weight_decay": 0.0}
                   for pp in getattr(self, "pose_params", [])]
        self.opts = FusedAdamW(groups)

    def log_opt_psnr(self, mse, time_spent, num_obj):
        self.psnr_opt.setdefault(num_obj, []).append(float(-10 * np.log(mse) / np.log(10)))

    def log_eval_psnr(self, mse, num_obj):
        self.psnr_eval.setdefault(num_obj, []).append(float(-10 * np.log(mse) / np.log(10)))

    def save_opts(self, num_obj):
        if self.rank != 0:
            return
        torch.save(self.saved_dict(num_obj), os.path.join(self.save_dir, "codes.pth"))

    def saved_dict(self, num_obj):
        """codes.pth: the reference's keys (src/optimizer.py:138-145); pose
        refinement adds its own and nothing when it is off."""
        d = {"ids": [str(i) for i in self.ids], "num_obj": num_obj,
             "optimized_shapecodes": self.optimized_shapecodes,
             "optimized_texturecodes": self.optimized_texturecodes,
             "psnr_eval": self.psnr_eval, "ssim_eval": self.ssim_eval}
        if getattr(self, "optimize_pose", False):
            d.update(optimized_poses=self.optimized_poses, pose_rot_err_deg=self.pose_rot_err,
                     pose_trans_err=self.pose_trans_err)
        return d

    def save_img(self, generated_imgs, gt_imgs, obj_id, instance_num, opt=True):
        from PIL import Image
        H, W = gt_imgs[0].shape[:2]
        nv = len(generated_imgs)
        ret = torch.zeros(nv * H, 2 * W, 3)
        ret[:, :W] = torch.cat([g.detach().cpu() for g in generated_imgs]).reshape(-1, W, 3)
        ret[:, W:] = torch.cat([g.detach().cpu() for g in gt_imgs]).reshape(-1, W, 3)
        d = os.path.join(self.save_dir, str(obj_id))
        os.makedirs(d, exist_ok=True)
        name = f"opt{self.nviews}_{instance_num}.png" if opt else f"{instance_num}_{self.nviews}.png"
        Image.fromarray(image_float_to_uint8(ret.numpy())).save(os.path.join(d, name))

    def make_model(self):
        prec = self.hpams.get("precision", "fp32")
        self.model = CodeNeRF(**self.hpams["net_hyperparams"], precision=prec).to(self.device)

    def load_model_codes(self, saved_dir):
        saved = torch.load(os.path.join(self.exp_root, saved_dir, "models.pth"), map_location="cpu",
                           weights_only=True)
        self.make_save_img_dir(os.path.join(self.exp_root, saved_dir, "test"))
        self.model.load_state_dict(saved["model_params"])
        self.model = self.model.to(self.device)
        self.mean_shape = torch.mean(saved["shape_code_params"]["weight"], dim=0).reshape(1, -1)
        self.mean_texture = torch.mean(saved["texture_code_params"]["weight"], dim=0).reshape(1, -1)

    def make_save_img_dir(self, save_dir):
        # rank 0 picks the first free "test", "test_2", ... and tells the others
        tmp = None
        if self.rank == 0:
            tmp, num = save_dir, 2
            while os.path.isdir(tmp):
                tmp = save_dir + "_" + str(num)
                num += 1
            os.makedirs(tmp)
        if self.world > 1:
            box = [tmp]
            self.dist.broadcast_object_list(box, src=0)
            tmp = box[0]
        self.save_dir = tmp

    def make_dataloader(self, splits, num_instances_per_obj, crop_img=False):
        d = self.hpams["data"]
        obj = d["cat"].split("_")[1]
        self.dataset = SRN(cat=d["cat"], splits=obj + "_" + splits, data_dir=d["data_dir"],
                           num_instances_per_obj=num_instances_per_obj, crop_img=crop_img,
                           n_test_views=int(d.get("n_test_views", 250)))
        self.ids = self.dataset.ids
