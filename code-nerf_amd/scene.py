"""Several objects in one picture (no reference counterpart).

A scene is 1..8 objects.  Each has its own shape and texture code, an
``occupancy.OccupancyGrid`` built for that shape code in the object's own frame
-- the box outside which the trained field is undefined, so the object
contributes nothing there -- and a similarity transform from its frame to the
world: ``x_world = scale * rotation @ x_obj + translation``.
``ImageStep.render_scene`` renders it with correct mutual occlusion and, per
pixel, every object's share of the opacity and the instance label.

A scene file is JSON::

    {"objects": [{"shape": 0, "texture": 0, "translation": [0.3, 0, 0],
                  "rotation_deg": [30, 0, 0], "scale": 1.0, "bound": 0.5,
                  "occ_grid": 128, "occ_tau": 0.1, "occ_dilate": 2}, ...]}

``shape`` / ``texture``: a row of the code tables, or ``[i, j, t]`` for the blend
``edit.blend(table[i], table[j], t)``; ``rotation_deg``: yaw, pitch, roll of
``rotation_zyx``; ``bound``: half the side of the object's box; the ``occ_*``
keys are optional (the Optimizer's defaults).
"""
import json
import math

import numpy as np
import torch

from .occupancy import OccupancyGrid

MAX_OBJECTS = 8
ENTRY_KEYS = ("shape", "texture", "translation", "rotation_deg", "scale", "bound")


def rotation_zyx(yaw, pitch, roll):
    """Rz(yaw) Ry(pitch) Rx(roll), degrees -> (3, 3) float64."""
    a, b, c = (math.radians(float(v)) for v in (yaw, pitch, roll))
    rz = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[math.cos(b), 0.0, math.sin(b)], [0.0, 1.0, 0.0], [-math.sin(b), 0.0, math.cos(b)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(c), -math.sin(c)], [0.0, math.sin(c), math.cos(c)]])
    return rz @ ry @ rx


def check_transform(rotation, translation, scale):
    """-> (rotation (3, 3), translation (3,), scale) as float64 / float, or
    ValueError: the rotation must be orthonormal within 1e-4 with det > 0, the
    translation finite, the scale finite and positive."""
    rot = np.asarray(rotation, dtype=np.float64)
    if rot.shape != (3, 3):
        raise ValueError(f"rotation must be 3x3, got shape {rot.shape}")
    if not np.isfinite(rot).all() or np.abs(rot @ rot.T - np.eye(3)).max() > 1e-4:
        raise ValueError("rotation must be orthonormal within 1e-4 (R R^T = I)")
    if not np.linalg.det(rot) > 0:
        raise ValueError("rotation must have a positive determinant (no reflection)")
    t = np.asarray(translation, dtype=np.float64).reshape(-1)
    if t.shape != (3,) or not np.isfinite(t).all():
        raise ValueError("translation must be 3 finite values")
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"scale must be finite and positive, got {scale}")
    return rot, t, scale


class SceneObject:
    def __init__(self, shape_code, texture_code, grid, rotation=None, translation=(0.0, 0.0, 0.0), scale=1.0):
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("a scene object needs an OccupancyGrid (its box bounds the object)")
        self.rotation, self.translation, self.scale = check_transform(
            np.eye(3) if rotation is None else rotation, translation, scale)
        self.shape_code, self.texture_code, self.grid = shape_code, texture_code, grid
        # 1 / s as the kernels get it: a float32 value
        self.inv_s = float(np.float32(1.0 / self.scale))

    def transform_row(self):
        """The 13 floats of cn_scene_rays: rotation row-major, translation, 1 / s."""
        return [float(np.float32(v)) for v in self.rotation.reshape(-1)] + \
               [float(np.float32(v)) for v in self.translation] + [self.inv_s]

    def radius(self):
        """Of the sphere around the world origin that holds the object's box."""
        c = np.asarray(self.grid.center, dtype=np.float64)
        return float(np.linalg.norm(self.translation + self.scale * (self.rotation @ c))
                     + math.sqrt(3.0) * self.scale * self.grid.bound)


class Scene:
    def __init__(self, objects):
        objects = list(objects)
        if not 1 <= len(objects) <= MAX_OBJECTS:
            raise ValueError(f"a scene holds 1 to {MAX_OBJECTS} objects, got {len(objects)}")
        if not all(isinstance(o, SceneObject) for o in objects):
            raise ValueError("a scene holds SceneObject instances")
        self.objects = objects

    def __len__(self):
        return len(self.objects)

    def transforms(self):
        return [o.transform_row() for o in self.objects]

    def inv_s(self):
        return [o.inv_s for o in self.objects]

    def depth_range(self, camera_distance):
        """(near, far) = (max(d - rho, 0.05), d + rho) for a camera at distance
        d from the world origin, rho = max_k(|t_k| + sqrt(3) s_k bound_k)."""
        d = float(camera_distance)
        rho = max(o.radius() for o in self.objects)
        return max(d - rho, 0.05), d + rho


def _code_spec(v, n, name):
    """An index, or [i, j, t] -> (i,) or (i, j, t)."""
    if isinstance(v, bool):
        raise ValueError(f"{name}: an index or [i, j, t], got {v!r}")
    if isinstance(v, int):
        spec = (v,)
    elif isinstance(v, (list, tuple)) and len(v) == 3 and all(isinstance(i, int) and not isinstance(i, bool)
                                                              for i in v[:2]):
        spec = (v[0], v[1], float(v[2]))
        if not math.isfinite(spec[2]):
            raise ValueError(f"{name}: the blend weight must be finite")
    else:
        raise ValueError(f"{name}: an index or [i, j, t], got {v!r}")
    for i in spec[:2]:
        if not 0 <= i < n:
            raise ValueError(f"{name} {i}: the tables hold {n} objects")
    return spec


def parse_scene(desc, n_codes):
    """Validate a scene description (the parsed JSON) against tables of
    n_codes rows -> a list of dicts: shape, texture (index tuples), rotation
    (3, 3), translation (3,), scale, bound, occ_grid, occ_tau, occ_dilate."""
    from .optimizer import OCC_DILATE, OCC_GRID, OCC_TAU
    if not isinstance(desc, dict) or not isinstance(desc.get("objects"), list):
        raise ValueError('a scene file is {"objects": [...]}')
    entries = desc["objects"]
    if not 1 <= len(entries) <= MAX_OBJECTS:
        raise ValueError(f"a scene holds 1 to {MAX_OBJECTS} objects, got {len(entries)}")
    out = []
    for k, e in enumerate(entries):
        who = f"object {k}"
        if not isinstance(e, dict):
            raise ValueError(f"{who}: an object entry is a JSON object")
        missing = [key for key in ENTRY_KEYS if key not in e]
        if missing:
            raise ValueError(f"{who}: missing {missing}")
        unknown = sorted(set(e) - set(ENTRY_KEYS) - {"occ_grid", "occ_tau", "occ_dilate"})
        if unknown:
            raise ValueError(f"{who}: unknown keys {unknown}")
        try:
            deg = [float(v) for v in e["rotation_deg"]]
            if len(deg) != 3:
                raise ValueError("rotation_deg takes yaw, pitch and roll")
            rot, t, s = check_transform(rotation_zyx(*deg), e["translation"], e["scale"])
            bound = float(e["bound"])
            if not (math.isfinite(bound) and bound > 0):
                raise ValueError(f"bound must be finite and positive, got {bound}")
            G, tau, dil = int(e.get("occ_grid", OCC_GRID)), float(e.get("occ_tau", OCC_TAU)), \
                int(e.get("occ_dilate", OCC_DILATE))
            if G % 32 or not 32 <= G <= 256:
                raise ValueError("occ_grid must be a multiple of 32 in [32, 256]")
            if not tau >= 0:
                raise ValueError("occ_tau must not be negative")
            if not 0 <= dil <= 4:
                raise ValueError("occ_dilate must be in [0, 4]")
            out.append(dict(shape=_code_spec(e["shape"], n_codes, "shape"),
                            texture=_code_spec(e["texture"], n_codes, "texture"), rotation=rot, translation=t,
                            scale=s, bound=bound, occ_grid=G, occ_tau=tau, occ_dilate=dil))
        except (TypeError, ValueError) as err:
            raise ValueError(f"{who}: {err}") from None
    return out


def load_scene(path, shape_table, texture_table, model):
    """Read a JSON scene file and build every object's grid with
    OccupancyGrid.build on the model's device -> (Scene, the file's content)."""
    from .edit import blend
    with open(path) as f:
        desc = json.load(f)
    dev = next(model.parameters()).device
    code = lambda tab, spec: (tab[spec[0]].clone() if len(spec) == 1 else blend(tab[spec[0]], tab[spec[1]], spec[2]))
    objects = []
    for e in parse_scene(desc, shape_table.shape[0]):
        s = code(shape_table, e["shape"]).to(dev, torch.float32)
        t = code(texture_table, e["texture"]).to(dev, torch.float32)
        grid = OccupancyGrid.build(model, s, G=e["occ_grid"], bound=e["bound"], tau=e["occ_tau"],
                                   dilate=e["occ_dilate"])
        objects.append(SceneObject(s, t, grid, e["rotation"], e["translation"], e["scale"]))
    return Scene(objects), desc
