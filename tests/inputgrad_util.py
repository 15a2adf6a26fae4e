"""Helpers of the input-gradient / pose tests (test infrastructure).

The accuracy bar of these tests is computed, not fixed ("Input
gradients and pose refinement"): ``err_emu`` is the rel-L2 distance between a
float64 replay of the oracle and the oracle run in fp32 under the operand
rounding that restates what the kernels read for a plan; the GPU result must
be within twice that of the float64 replay.  The factor 2 covers what the
restatement does not model: the kernel's own sin / cos, its summation order
and the hi + lo split of the input layers' weights.
"""
import contextlib

import numpy as np
import torch

from oracle import ref_cpu
from oracle.params import look_at_pose, make_codes, make_params

PLANS = ["fp32", "bf16", "bf16x3", "bf16x3f"]
MARGIN = 2.0

# What the kernels read, per plan: the plan's operand rounding plus, wherever
# the stored dA plane is bf16, the upstream gradient of the two input layers
# as its stored hi part.  Written before the first GPU run; not tuned.
_INPUT_LAYERS_HI = {"encoding_xyz.0": {"bw_dy": "b"}, "encoding_viewdir.0": {"bw_dy": "b"}}
EMU = {
    "fp32": None,
    "bf16": dict(layer_ops=_INPUT_LAYERS_HI),
    "bf16x3": dict(ops=ref_cpu.OPS_BF16X3, layer_ops=_INPUT_LAYERS_HI),
    "bf16x3f": dict(ops=ref_cpu.OPS_BF16X3F, layer_ops=_INPUT_LAYERS_HI),
}


def emu_context(plan):
    kw = EMU[plan]
    return contextlib.nullcontext() if kw is None else ref_cpu.bf16_operands(**kw)


def dev():
    return torch.device("cuda", 0)


def rel_l2(a, b):
    """||a - b|| / ||b|| (b: the more accurate value)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def net_params(sb, tb=1, seed=3, sigma_shift=0.0):
    return make_params(seed, sigma_bias_shift=sigma_shift, shape_blocks=sb, texture_blocks=tb)


def model(params, sb, tb=1, precision="fp32"):
    from codenerf_amd.model import CodeNeRF
    m = CodeNeRF(sb, tb, precision=precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    return m.to(dev())


def codes(obj=1):
    s, t = make_codes(3, 2)
    return s, t, obj


def tparams(params, dtype):
    return {k: torch.tensor(v, dtype=dtype) for k, v in params.items()}


def camera_rays(H, W, radius=1.3, az=35.0, el=20.0):
    """fp32 rays of the oracle's get_rays for a look-at pose, focal 1.2 H."""
    c2w = look_at_pose(radius, az, el)
    ro, vd = ref_cpu.get_rays(H, W, 1.2 * H, c2w)
    return ro.contiguous(), vd.contiguous(), c2w


def seeded(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------ mode A
def sample_inputs(M, seed=11):
    """Points in the scene box, unit view directions, random upstream grads."""
    rng = seeded(seed)
    xyz = rng.uniform(-1.0, 1.0, (M, 3)).astype(np.float32)
    v = rng.standard_normal((M, 3))
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    dsig = rng.standard_normal(M).astype(np.float32)
    drgb = rng.standard_normal((M, 3)).astype(np.float32)
    return xyz, v, dsig, drgb


# A per-sample gradient is discontinuous where a pre-activation crosses 0 (the
# ReLU kink): a sample whose float64 pre-activation lies within fp32 rounding
# of 0 gets, from ANY fp32 arithmetic, either side's gradient -- an O(1)
# difference in that one sample that says nothing about accuracy (the CPU
# oracle in fp32 flips such samples too, different ones per BLAS build).  They
# are left out of the per-sample comparisons, chosen from the float64 replay
# alone: |pre| < KINK x the layer's rms pre-activation.  An fp32 dot product
# over K <= 283 terms is good to ~sqrt(K) 2^-24 ~ 1e-6 of that scale (bound
# K 2^-24 ~ 1.7e-5), so 1e-5 is ~10 typical errors; it drops ~1 % of samples.
KINK = 1e-5


def oracle_sample_grads(params, sb, tb, xyz, v, dsig, drgb, dtype, plan=None, with_kink=False):
    """Autograd of codenerf_forward with respect to (xyz, viewdir) for the
    upstream gradients (dsig, drgb); float64, or fp32 under a plan's emulation.
    with_kink: also the mask [M] of samples at a ReLU kink (see KINK)."""
    from unittest import mock
    p = tparams(params, dtype)
    s, t, obj = codes()
    M = xyz.shape[0]
    x = torch.tensor(xyz, dtype=dtype, requires_grad=True)
    d = torch.tensor(v, dtype=dtype, requires_grad=True)
    kink = torch.zeros(M, dtype=torch.bool)
    relu = torch.nn.functional.relu

    def spy(pre, *a, **k):
        if with_kink and pre.dim() == 2 and pre.shape[0] == M:       # a per-sample layer (not a latent layer)
            q = pre.detach()
            kink.logical_or_((q.abs() < KINK * q.pow(2).mean().sqrt()).any(1))
        return relu(pre, *a, **k)

    with (emu_context(plan) if plan else contextlib.nullcontext()), mock.patch.object(torch.nn.functional, "relu", spy):
        sig, rgb = ref_cpu.codenerf_forward(p, x, d, torch.tensor(s[obj:obj + 1], dtype=dtype),
                                            torch.tensor(t[obj:obj + 1], dtype=dtype), shape_blocks=sb,
                                            texture_blocks=tb)
        loss = (sig[..., 0] * torch.tensor(dsig, dtype=dtype)).sum() + (rgb * torch.tensor(drgb, dtype=dtype)).sum()
        loss.backward()
    if with_kink:
        return x.grad.numpy(), d.grad.numpy(), kink.numpy()
    return x.grad.numpy(), d.grad.numpy()


def gpu_sample_grads(m, xyz, v, dsig, drgb, act_M=0, row0=0):
    """The HIP path through the engine: codes forward, pose backward, input
    gradients, on explicit points (mode A) -> (d_xyz [M,3], d_viewdir [M,3])."""
    eng = m.engine()
    params = m.param_list()
    M = xyz.shape[0]
    s, t, obj = codes()
    d = dev()
    x, vd = torch.tensor(xyz, device=d), torch.tensor(v, device=d)
    eng.ensure_packed(params, bwd=True)
    blob, _ = eng.latent_fwd(params, torch.tensor(s[obj], device=d), torch.tensor(t[obj], device=d))
    act = eng.new_act(max(M, act_M))
    eng.mlp_fwd(blob, M, xyz=x, viewdir=vd, act=act, act_M=act_M, act_row0=row0, codes=True)
    eng.mlp_bwd(blob, M, torch.tensor(dsig, device=d), torch.tensor(drgb, device=d), act, act_M=act_M, row0=row0,
                pose=True)
    dxyz, dvd, _, _ = eng.mlp_input_grad(act, M, xyz=x, viewdir=vd, act_M=act_M, row0=row0)
    torch.cuda.synchronize()
    return dxyz[:M].cpu().numpy(), dvd[:M].cpu().numpy(), dxyz[M:].cpu().numpy(), dvd[M:].cpu().numpy()


# ------------------------------------------------------------------ mode B
def oracle_ray_grads(params, sb, tb, ro, vd, z, gt, chunk, dtype, plan=None, reg_coef=1e-4):
    """Gradient of the summed chunk losses of ref_cpu.image_step with respect
    to (rays_o, viewdirs); also the chunk losses."""
    p = tparams(params, dtype)
    s, t, obj = codes()
    st, tt = torch.tensor(s, dtype=dtype), torch.tensor(t, dtype=dtype)
    o = ro.detach().to(dtype).clone().requires_grad_()
    d = vd.detach().to(dtype).clone().requires_grad_()
    with (emu_context(plan) if plan else contextlib.nullcontext()):
        losses, _ = ref_cpu.image_step(p, st, tt, obj, o, d, z.to(dtype), gt.to(dtype), chunk=chunk,
                                       reg_coef=reg_coef, net=dict(shape_blocks=sb, texture_blocks=tb))
    return o.grad.numpy(), d.grad.numpy(), losses


def gpu_image_step(m, ro, vd, z, gt, chunk, input_grads=True, weight_grads=False, step=None, reg=True):
    """ImageStep.forward_backward on the device -> dict of results."""
    from codenerf_amd.render import ImageStep
    s, t, obj = codes()
    d = dev()
    st = torch.nn.Parameter(torch.tensor(s, device=d))
    tt = torch.nn.Parameter(torch.tensor(t, device=d))
    for p in m.parameters():
        p.grad = None
    step = step or ImageStep(m, chunk=chunk, reg_coef=1e-4)
    kw = dict(input_grads=True) if input_grads else {}
    losses, rgb, _ = step.forward_backward(ro.to(d), vd.to(d), z.to(d), gt.to(d), st, tt, obj, reg=reg,
                                           weight_grads=weight_grads, **kw)
    torch.cuda.synchronize()
    out = dict(step=step, losses=losses.cpu().numpy(), rgb=rgb.cpu().numpy(), ds=st.grad.cpu().numpy(),
               dt=tt.grad.cpu().numpy(),
               dparams=[None if p.grad is None else p.grad.cpu().numpy() for p in m.parameters()])
    if input_grads:
        out["d_ro"], out["d_vd"] = (g.cpu().numpy() for g in step.last_ray_grads)
    return out
