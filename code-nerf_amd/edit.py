"""Editing shapes and textures (the reference README's catalogue line "Editing
Shapes/Textures", which the reference ships no code for): load
saved codes, swap or blend them, and render the result along a camera path
with its geometry buffers.

  load_code_tables   the code tables of a training run (models.pth) or the
                     optimised codes of a test-time run (codes.pth)
  blend              (1 - t) a + t b
  orbit_pose         camera on a sphere looking at the origin, as get_rays takes it
  frame_plan         per-frame (shape weight, texture weight, azimuth)
  aov_to_uint8       depth / median depth / normal / opacity maps as images
  render_edit        the frames of render.py

An edit changes geometry or appearance: sigma is taken before the texture code
enters the network (src/model.py:36-53), so a texture swap leaves depth,
opacity, median depth and normal untouched bit for bit and a shape swap moves
them -- the buffers of ``ImageStep.render_aov`` show which of the two a code
change did.
"""
import json
import os

import numpy as np
import torch

from .data import SRN_TO_GL, look_at_srn

AOV_NAMES = {"depth": "depth", "depth_median": "depthmed", "normal": "normal", "acc": "alpha"}


def load_code_tables(saved_dir, exp_root="exps", codes=None):
    """-> (shape table (n, D), texture table (n, D), ids), float32 on the host.
    codes None: the training tables of <exp_root>/<saved_dir>/models.pth, ids
    "0" .. "n-1" (the trainer's object indices).  codes: a codes.pth (a path, or
    a path under <exp_root>/<saved_dir>), its ``optimized_shapecodes`` /
    ``optimized_texturecodes`` and ``ids``."""
    if codes is None:
        saved = torch.load(os.path.join(exp_root, saved_dir, "models.pth"), map_location="cpu", weights_only=True)
        s, t = saved["shape_code_params"]["weight"], saved["texture_code_params"]["weight"]
        ids = [str(i) for i in range(s.shape[0])]
    else:
        path = codes if os.path.exists(codes) else os.path.join(exp_root, saved_dir, codes)
        saved = torch.load(path, map_location="cpu", weights_only=True)
        s, t = saved["optimized_shapecodes"], saved["optimized_texturecodes"]
        ids = [str(i) for i in saved["ids"]]
    s, t = s.detach().to(torch.float32).contiguous(), t.detach().to(torch.float32).contiguous()
    if s.dim() != 2 or s.shape != t.shape:
        raise ValueError(f"code tables must be two (n, D) tensors, got {tuple(s.shape)} and {tuple(t.shape)}")
    return s, t, ids


def blend(a, b, t):
    """(1 - t) a + t b in float32; t = 0 and t = 1 hand back a and b bit for
    bit (signed zeros and non-finite entries included)."""
    a, b, t = a.to(torch.float32), b.to(torch.float32), float(t)
    if t == 0.0:
        return a.clone()
    if t == 1.0:
        return b.clone()
    return (1.0 - t) * a + t * b


def orbit_pose(radius, az_deg, el_deg):
    """Camera-to-world (4, 4) float32 in the convention get_rays takes (OpenGL
    axes): what the SRN loader hands out for a pose file holding
    data.look_at_srn(radius, az_deg, el_deg)."""
    return torch.from_numpy(look_at_srn(radius, az_deg, el_deg) @ SRN_TO_GL).float()


def frame_plan(frames, shape, texture, azimuth):
    """[(t_shape, t_texture, azimuth)] of the K = frames frames.  shape /
    texture: one or two table indices; with two, frame k blends with weight
    k / (K - 1) (0 when K = 1), with one its weight is 0.  azimuth: (A0,) or
    (A0, A1) degrees; frame k looks from A0 + (A1 - A0) k / K -- the end point
    is left out, so a 0 360 sweep loops."""
    K = int(frames)
    if K < 1:
        raise ValueError(f"frames must be at least 1, got {frames}")
    for name, v in (("shape", shape), ("texture", texture), ("azimuth", azimuth)):
        if len(v) not in (1, 2):
            raise ValueError(f"{name} takes one or two values, got {len(v)}")
    a0 = float(azimuth[0])
    a1 = float(azimuth[1]) if len(azimuth) == 2 else a0
    plan = []
    for k in range(K):
        t = k / (K - 1) if K > 1 else 0.0
        plan.append((t if len(shape) == 2 else 0.0, t if len(texture) == 2 else 0.0, a0 + (a1 - a0) * k / K))
    return plan


def _to_uint8(x):
    return np.floor(np.clip(np.nan_to_num(np.asarray(x, dtype=np.float64)), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def rgb_to_uint8(rgb):
    """Colours clipped to [0, 1] and rounded to the nearest of 255 steps (no
    min-max normalisation: frames of one sequence share one scale)."""
    return _to_uint8(rgb)


def aov_to_uint8(name, a, near=0.0, far=1.0):
    """One geometry buffer as an 8-bit image array of the input's shape.
    depth, depth_median: (d - near) / (far - near), clipped; normal (..., 3):
    0.5 + 0.5 n / |n|, mid-grey where n is 0; acc: grey, clipped."""
    a = np.asarray(a, dtype=np.float64)
    if name in ("depth", "depth_median"):
        return _to_uint8((a - near) / (far - near))
    if name == "normal":
        n = np.sqrt((a * a).sum(-1, keepdims=True))
        return _to_uint8(0.5 + 0.5 * np.divide(a, n, out=np.zeros_like(a), where=n > 0))
    if name == "acc":
        return _to_uint8(a)
    raise ValueError(f"unknown buffer {name!r}")


def render_edit(model, shape_table, texture_table, shape, texture, out_dir, frames=1, azimuth=(0.0,),
                elevation=20.0, radius=1.3, size=128, focal=131.25, near=0.8, far=1.8, n_samples=64, n_fine=0,
                aov=False):
    """Render the frames of ``frame_plan`` into out_dir: ``rgb_%03d.png`` and,
    with aov, ``depth_``, ``depthmed_``, ``normal_`` and ``alpha_`` (normals
    through ``ImageStep.render_aov``), plus ``frames.json`` with every frame's
    indices, weights and pose.  z = stratified_z(z_fixed=True) and the fine
    samples are the deterministic ones: nothing is drawn.  -> the frames.json
    content."""
    from PIL import Image
    from .render import ImageStep
    from .utils import get_rays, stratified_z
    dev = next(model.parameters()).device
    step = ImageStep(model)
    H = W = int(size)
    z = stratified_z(near, far, int(n_samples), z_fixed=True).to(dev)
    os.makedirs(out_dir, exist_ok=True)
    code = lambda tab, idx, t: (blend(tab[idx[0]], tab[idx[1]], t) if len(idx) == 2 else tab[idx[0]].clone()).to(dev)
    record = []
    for k, (ts, tt, az) in enumerate(frame_plan(frames, shape, texture, azimuth)):
        pose = orbit_pose(radius, az, elevation)
        rays_o, viewdir = get_rays(H, W, float(focal), pose.to(dev))
        s, t = code(shape_table, shape, ts), code(texture_table, texture, tt)
        if aov:
            out = step.render_aov(rays_o, viewdir, z, s, t, n_fine=int(n_fine))
        elif n_fine:
            out = dict(rgb=step.render_fine(rays_o, viewdir, z, int(n_fine), s, t)[0])
        else:
            out = dict(rgb=step.render(rays_o, viewdir, z, s, t)[0])
        img = lambda a: a.reshape(H, W, -1).squeeze(-1).cpu().numpy()
        Image.fromarray(rgb_to_uint8(img(out["rgb"]))).save(os.path.join(out_dir, f"rgb_{k:03d}.png"))
        if aov:
            for name, stem in AOV_NAMES.items():
                Image.fromarray(aov_to_uint8(name, img(out[name]), near, far)).save(
                    os.path.join(out_dir, f"{stem}_{k:03d}.png"))
        record.append(dict(frame=k, shape=[int(i) for i in shape], texture=[int(i) for i in texture], t_shape=ts,
                           t_texture=tt, azimuth=az, elevation=float(elevation), radius=float(radius),
                           pose=pose.tolist()))
    meta = dict(size=H, focal=float(focal), near=near, far=far, n_samples=int(n_samples), n_importance=int(n_fine),
                aov=bool(aov), frames=record)
    with open(os.path.join(out_dir, "frames.json"), "w") as f:
        json.dump(meta, f, indent=2)
    return meta
