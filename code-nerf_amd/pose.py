"""Camera-pose refinement at test time (no reference counterpart: the
reference lists "Pose Optimizing" as not done).

``PoseParam`` holds a 6-vector ``delta = (omega, tau)`` around a starting pose:

    c2w(delta) = [ Exp(omega) R0 | t0 + tau ]

with Exp the matrix exponential of the hat matrix of ``omega`` (an axis-angle
rotation applied on the world side).  The 6-vector is not a hot path: it lives
under plain torch autograd on the device.  The hot path is the renderer's
gradient with respect to the rays (``ImageStep.forward_backward(...,
input_grads=True)`` -> ``last_ray_grads``), pushed through the HIP backward of
the ray generation (``utils.get_rays``) into ``delta.grad``.
"""
import numpy as np
import torch


def hat(w):
    """(3,) -> the skew-symmetric matrix with hat(w) v = w x v."""
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]),
                        torch.stack([w[2], z, -w[0]]),
                        torch.stack([-w[1], w[0], z])])


class PoseParam:
    def __init__(self, c2w0):
        c = torch.as_tensor(c2w0).detach().reshape(-1, 4, 4)[0].to(torch.float32).clone()
        self.c2w0 = c
        self.delta = torch.zeros(6, dtype=torch.float32, device=c.device, requires_grad=True)
        self._rays = None

    def c2w(self):
        """The 4x4 pose at the current delta (differentiable in delta).  The
        rotation is formed in float64 and rounded once, so it stays orthonormal
        to float32 rounding however delta was reached."""
        R0, t0 = self.c2w0[:3, :3], self.c2w0[:3, 3]
        E = torch.linalg.matrix_exp(hat(self.delta[:3].to(torch.float64)))
        R = (E @ R0.to(torch.float64)).to(torch.float32)
        top = torch.cat([R, (t0 + self.delta[3:])[:, None]], 1)
        return torch.cat([top, self.c2w0[3:4]], 0)

    def rays(self, H, W, focal):
        """Rays of the current pose for one render (detached); the graph back
        to delta is kept for backward_from_ray_grads."""
        from .utils import get_rays
        self._rays = get_rays(H, W, focal, self.c2w())
        return self._rays[0].detach(), self._rays[1].detach()

    def backward_from_ray_grads(self, ray_grads):
        """Accumulates d loss / d delta into ``delta.grad`` from (d_rays_o,
        d_viewdirs) of the rays handed out by the last ``rays`` call."""
        if self._rays is None:
            raise RuntimeError("backward_from_ray_grads: call rays() first")
        ro, vd = self._rays
        self._rays = None
        torch.autograd.backward([ro, vd], [ray_grads[0].to(ro), ray_grads[1].to(vd)])

    @torch.no_grad()
    def errors(self, c2w_ref):
        """(rotation error in degrees, translation error) against a pose."""
        return pose_errors(self.c2w(), c2w_ref)


def pose_errors(c2w, c2w_ref):
    a = torch.as_tensor(c2w).detach().reshape(-1, 4, 4)[0].to("cpu", torch.float64)
    b = torch.as_tensor(c2w_ref).detach().reshape(-1, 4, 4)[0].to("cpu", torch.float64)
    cos = ((a[:3, :3].T @ b[:3, :3]).trace() - 1.0) / 2.0
    return float(torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0)))), float(torch.linalg.norm(a[:3, 3] - b[:3, 3]))


def perturb_pose(c2w, rot_deg, trans, seed):
    """c2w rotated by ``rot_deg`` degrees about a seeded normal axis (on the
    world side) and translated by ``trans`` times a seeded normal vector
    (numpy PCG64: the same on every machine).  -> float32 (4, 4) tensor."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    shift = rng.standard_normal(3) * float(trans)
    c = torch.as_tensor(c2w).detach().reshape(-1, 4, 4)[0].to("cpu", torch.float64).clone()
    w = torch.tensor(axis * np.deg2rad(float(rot_deg)), dtype=torch.float64)
    c[:3, :3] = torch.linalg.matrix_exp(hat(w)) @ c[:3, :3]
    c[:3, 3] += torch.tensor(shift, dtype=torch.float64)
    return c.to(torch.float32)
