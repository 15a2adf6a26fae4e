"""GPU: the fine pass at test time -- cn_composite_fine_fwd, ImageStep.render_fine,
the codes-only / pose step through forward_backward_fine, and the Optimizer flow.

The reference has no fine pass: the oracle is the CPU
restatement in oracle/ref_cpu.py (merge_samples, volume_rendering,
composite_weights, sample_pdf, fine_image_step) on identical inputs.

Bars (each one an existing bar of the quantity it checks):
  * composite rgb / depth / acc: rtol 1e-5, atol 1e-6 (the loss kernel's rgb
    bar in test_gpu_fine.py), and the rgb bit for bit the loss kernel's;
  * render_fine at fp32: fine z within 1e-4, rgb / depth rtol 1e-4, atol 1e-6
    on the GPU's own z_f; bf16 max |d| < 3e-2, bf16x3 / bf16x3f 1e-4 relative
    (denominator floored at 1e-2) on one z_f computed on the CPU;
  * the codes-only fine step: rgb / losses rtol 1e-4, code-table gradients
    rtol 2e-3, atol 2e-6 max(1, max|g|) (test_fine_train_step_fp32_matches_oracle);
  * ray and pose gradients: err_gpu <= inputgrad_util.MARGIN x err_emu, both
    rel-L2 against the float64 autograd of fine_image_step (z_f a constant).
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import inputgrad_util as U
from golden_util import case_params, load
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ a
def _composite_inputs(Nc, Nf, per_ray_z):
    """max(R) = 257 rays, made once per shape; smaller R take the first rays.
    Ray 0: ties (a coarse sample precedes a fine one at equal z); ray 1: zero
    density everywhere; ray 2: an opaque wall."""
    g = torch.Generator().manual_seed(Nc * 13 + Nf + int(per_ray_z))
    R = 257
    if per_ray_z:
        zc = torch.sort(0.8 + torch.rand(R, Nc, generator=g), -1).values
    else:
        zc = torch.linspace(0.8, 1.8, Nc)
    zf = torch.sort(0.8 + torch.rand(R, Nf, generator=g), -1).values
    zf[0, :4] = zc[0, 3] if per_ray_z else zc[3]
    zf[0] = torch.sort(zf[0]).values                 # the four tied samples stay; z_f stays ascending
    sc = torch.rand(R, Nc, generator=g) * 6
    sf = torch.rand(R, Nf, generator=g) * 6
    sc[1], sf[1] = 0.0, 0.0
    sc[2, Nc // 2] = 1e4
    rc = torch.randn(R, Nc, 3, generator=g)
    rf = torch.randn(R, Nf, 3, generator=g)
    return zc, zf, sc, sf, rc, rf


def _composite_oracle(Nc, Nf, per_ray_z):
    zc, zf, sc, sf, rc, rf = _composite_inputs(Nc, Nf, per_ray_z)
    z_m, s_m, r_m = ref_cpu.merge_samples(zc, zf, (sc, sf), (rc, rf))
    out = {wb: ref_cpu.volume_rendering(s_m, r_m, z_m, white_bg=wb) for wb in (True, False)}
    return (zc, zf, sc, sf, rc, rf), out, ref_cpu.composite_weights(s_m, z_m).sum(-1)


@pytest.mark.parametrize("white_bg", [True, False])
@pytest.mark.parametrize("per_ray_z", [False, True])
@pytest.mark.parametrize("Nc,Nf", [(5, 3), (64, 64), (96, 160), (128, 128)])
@pytest.mark.parametrize("R", [1, 5, 257])
def test_composite_fine_fwd_matches_oracle(R, Nc, Nf, per_ray_z, white_bg):
    from codenerf_amd.engine import composite_fine_fwd, render_loss_fine
    (zc, zf, sc, sf, rc, rf), out, acc_ref = _cached(("comp", Nc, Nf, per_ray_z),
                                                     lambda: _composite_oracle(Nc, Nf, per_ray_z))
    rgb_ref, depth_ref = out[white_bg]
    dv = _dev()
    # one ray per launch cannot hold the three special rays at once: each goes alone
    for rows in ([slice(0, 1), slice(1, 2), slice(2, 3)] if R == 1 else [slice(0, R)]):
        n = rows.stop - rows.start
        t = lambda x: x[rows].contiguous().to(dv)
        z_c = t(zc) if per_ray_z else zc.to(dv)
        args = (t(sc), t(rc), z_c, Nc, t(sf), t(rf), t(zf), Nf, n)
        rgb, depth, acc = composite_fine_fwd(*args, white_bg=white_bg, acc=True)
        rgb2, depth2 = composite_fine_fwd(*args, white_bg=white_bg)
        gt = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(dv)
        dsc, drc = torch.zeros(n * Nc, device=dv), torch.zeros(n * Nc, 3, device=dv)
        dsf, drf = torch.empty(n * Nf, device=dv), torch.empty(n * Nf, 3, device=dv)
        rgb_loss, _ = render_loss_fine(*args, gt, 100, dsc, drc, dsf, drf, white_bg)
        torch.cuda.synchronize()
        np.testing.assert_allclose(rgb.cpu().numpy(), rgb_ref[rows].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(depth.cpu().numpy(), depth_ref[rows].numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(acc.cpu().numpy(), acc_ref[rows].numpy(), rtol=1e-5, atol=1e-6)
        assert torch.equal(rgb, rgb_loss), "the forward-only rgb must be the loss kernel's, bit for bit"
        assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2)        # acc pointer given or NULL


# ------------------------------------------------------------------ b
def test_composite_fine_fwd_refusals():
    """Host checks: nothing is launched (the pointers are never dereferenced)."""
    from codenerf_amd import _lib
    L, d = _lib.lib(), ctypes.c_void_p(256)

    def call(zc_stride, Nc, Nf, R=4):
        return L.cn_composite_fine_fwd(d, d, d, zc_stride, Nc, d, d, d, Nf, R, 1, d, d, None, None)

    assert call(0, 129, 128) == -1
    assert b"cn_composite_fine_fwd" in L.cn_last_error() and b"256 samples" in L.cn_last_error()
    assert call(7, 64, 64) == -1
    assert b"zc_stride must be 0 or Nc" in L.cn_last_error()
    assert call(0, 64, 0) == -1
    assert b"Nc and Nf must be positive" in L.cn_last_error()
    assert L.cn_composite_fine_fwd(d, d, d, 0, 64, d, d, d, 64, 4, 1, None, d, None, None) == -1
    assert b"NULL argument" in L.cn_last_error()
    assert _lib.ABI_VERSION == 4 and L.cn_abi_version() == 4


# ------------------------------------------------------------------ c, d
FINE_CASES = [("n64_16x16", 64, 0), ("n64_16x16", 64, 1), ("n64_16x16", 64, 3),
              ("ragged_48x48_n16", 40, 0), ("ragged_48x48_n16", 40, 1), ("ragged_48x48_n16", 40, 3)]


def _case(case, nrays):
    g = load(case)
    if nrays:
        g = dict(g)
        for k in ("rays_o", "viewdir", "gt"):
            g[k] = g[k][:nrays]
    return g


def _model(g, precision):
    from codenerf_amd.model import CodeNeRF
    m = CodeNeRF(3, 1, precision=precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in case_params(g).items()})
    return m.to(_dev())


def _oracle_coarse(g):
    """fp32 oracle: (sigma_c (R,Nc), rgb_c (R,Nc,3)) of the case's coarse samples."""
    p = ref_cpu.param_tensors(case_params(g), requires_grad=False)
    ro, vd, z = torch.tensor(g["rays_o"]), torch.tensor(g["viewdir"]), torch.tensor(g["z_vals"])
    oi = int(g["obj_idx"])
    s, t = torch.tensor(g["shape_table"])[oi][None], torch.tensor(g["texture_table"])[oi][None]
    with torch.no_grad():
        xyz = ro[:, None, :] + vd[:, None, :] * z[..., None]
        sig, rgb = ref_cpu.codenerf_forward(p, xyz, vd[:, None, :].expand(-1, z.shape[-1], -1), s, t)
    return sig[..., 0], rgb


def _oracle_render_fine(g, coarse, zf):
    """fp32 oracle of render_fine on given fine samples -> (rgb, depth)."""
    p = ref_cpu.param_tensors(case_params(g), requires_grad=False)
    ro, vd, z = torch.tensor(g["rays_o"]), torch.tensor(g["viewdir"]), torch.tensor(g["z_vals"])
    oi = int(g["obj_idx"])
    s, t = torch.tensor(g["shape_table"])[oi][None], torch.tensor(g["texture_table"])[oi][None]
    with torch.no_grad():
        xyz = ro[:, None, :] + vd[:, None, :] * zf[..., None]
        sig_f, rgb_f = ref_cpu.codenerf_forward(p, xyz, vd[:, None, :].expand(-1, zf.shape[-1], -1), s, t)
        z_m, s_m, r_m = ref_cpu.merge_samples(z, zf, (coarse[0], sig_f[..., 0]), (coarse[1], rgb_f))
        return ref_cpu.volume_rendering(s_m, r_m, z_m)


def _render_fine(g, precision, Nf, **kw):
    from codenerf_amd.render import ImageStep
    m = _model(g, precision)
    step = ImageStep(m, chunk=int(g["chunk"]))
    t = lambda k: torch.tensor(g[k], device=_dev())
    oi = int(g["obj_idx"])
    rgb, depth = step.render_fine(t("rays_o"), t("viewdir"), t("z_vals"), Nf, t("shape_table")[oi],
                                  t("texture_table")[oi], **kw)
    torch.cuda.synchronize()
    return rgb, depth, step.last_z_f


@pytest.mark.parametrize("case,Nf,nrays", FINE_CASES)
def test_render_fine_fp32_matches_oracle(case, Nf, nrays):
    g = _case(case, nrays)
    R = g["rays_o"].shape[0]
    coarse = _cached(("coarse", case, nrays), lambda: _oracle_coarse(g))
    rgb, depth, zf = _render_fine(g, "fp32", Nf)
    assert zf.shape == (R, Nf) and rgb.shape == (R, 3) and depth.shape == (R,)
    # its own deterministic sampling u_j = (j + 0.5) / Nf agrees with the oracle's
    zf_ref = ref_cpu.sample_pdf(coarse[0], torch.tensor(g["z_vals"]), torch.full((R, Nf), 0.5))
    dz = float((zf.cpu() - zf_ref).abs().max())
    print(f"{case} nrays {nrays}: fine z max|d| {dz:.2e}")
    assert dz < 1e-4
    rgb_r, depth_r = _oracle_render_fine(g, coarse, zf.cpu())
    print(f"  rgb max|d| {float((rgb.cpu() - rgb_r).abs().max()):.2e} depth max|d| "
          f"{float((depth.cpu() - depth_r).abs().max()):.2e}")
    np.testing.assert_allclose(rgb.cpu().numpy(), rgb_r.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(depth.cpu().numpy(), depth_r.numpy(), rtol=1e-4, atol=1e-6)
    # rand_f None draws nothing: it is rand_f = 0.5
    rgb2, depth2, zf2 = _render_fine(g, "fp32", Nf, rand_f=torch.full((R, Nf), 0.5))
    assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2) and torch.equal(zf, zf2)


@pytest.mark.parametrize("case,Nf,nrays", FINE_CASES)
@pytest.mark.parametrize("plan", ["bf16", "bf16x3", "bf16x3f"])
def test_render_fine_other_plans(plan, case, Nf, nrays):
    """One z_f, computed on the CPU, for every plan: rgb against the fp32
    oracle on it, at the bar the plan carries for the coarse render."""
    g = _case(case, nrays)
    R = g["rays_o"].shape[0]
    coarse = _cached(("coarse", case, nrays), lambda: _oracle_coarse(g))
    zf = _cached(("zf", case, nrays),
                 lambda: ref_cpu.sample_pdf(coarse[0], torch.tensor(g["z_vals"]), torch.full((R, Nf), 0.5)))
    ref = _cached(("render", case, nrays), lambda: _oracle_render_fine(g, coarse, zf))[0].numpy().astype(np.float64)
    rgb, _, used = _render_fine(g, plan, Nf, z_f=zf)
    assert torch.equal(used.cpu(), zf)
    rgb = rgb.cpu().numpy()
    d = float(np.abs(rgb - ref).max())
    rel = float((np.abs(rgb - ref) / np.maximum(np.abs(ref), 1e-2)).max())
    print(f"{plan} {case} nrays {nrays}: rgb max|d| {d:.2e} max rel {rel:.2e}")
    if plan == "bf16":
        assert d < 3e-2
    else:
        assert rel <= 1e-4


def _codes_step(g, Nf, rnd, **kw):
    from codenerf_amd.render import ImageStep
    m = _model(g, "fp32")
    st = torch.nn.Parameter(torch.tensor(g["shape_table"], device=_dev()))
    tt = torch.nn.Parameter(torch.tensor(g["texture_table"], device=_dev()))
    step = ImageStep(m, chunk=int(g["chunk"]), reg_coef=1e-4)
    t = lambda k: torch.tensor(g[k], device=_dev())
    lc, lf, rgb, _ = step.forward_backward_fine(t("rays_o"), t("viewdir"), t("z_vals"), rnd.to(_dev()), t("gt"), st, tt,
                                                int(g["obj_idx"]), weight_grads=False, **kw)
    torch.cuda.synchronize()
    return m, st, tt, lc, lf, rgb, step


@pytest.mark.parametrize("case,Nf,nrays", FINE_CASES)
def test_codes_only_fine_step_fp32_matches_oracle(case, Nf, nrays):
    g = _case(case, nrays)
    R = g["rays_o"].shape[0]
    rnd = torch.rand(R, Nf, generator=torch.Generator().manual_seed(5))
    m, st, tt, lc, lf, rgb, step = _codes_step(g, Nf, rnd)
    zf = step.last_z_f
    p = ref_cpu.param_tensors(case_params(g))
    st_r = torch.tensor(g["shape_table"], requires_grad=True)
    tt_r = torch.tensor(g["texture_table"], requires_grad=True)
    ro, vd, z = torch.tensor(g["rays_o"]), torch.tensor(g["viewdir"]), torch.tensor(g["z_vals"])
    lc_r, lf_r, rgb_r = ref_cpu.fine_image_step(p, st_r, tt_r, int(g["obj_idx"]), ro, vd, z, zf.cpu(),
                                                torch.tensor(g["gt"]), chunk=int(g["chunk"]))
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max())
    print(f"{case} nrays {nrays}: rgb max rel {rel(rgb.cpu().numpy(), rgb_r.numpy()):.2e} coarse loss "
          f"{rel(lc.cpu().numpy(), np.array(lc_r)):.2e} fine loss {rel(lf.cpu().numpy(), np.array(lf_r)):.2e}")
    np.testing.assert_allclose(rgb.cpu().numpy(), rgb_r.numpy(), rtol=1e-4)
    np.testing.assert_allclose(lc.cpu().numpy(), np.array(lc_r), rtol=1e-4)
    np.testing.assert_allclose(lf.cpu().numpy(), np.array(lf_r), rtol=1e-4)
    for tab, ref in ((st, st_r), (tt, tt_r)):
        a, b = tab.grad.cpu().numpy(), ref.grad.numpy()
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-6 * max(1.0, np.abs(b).max()))
    # the weights are fixed: nothing reaches their gradients
    for k, prm in m.named_parameters():
        assert prm.grad is None or not bool(prm.grad.any()), k


def test_codes_only_fine_step_refuses_recompute():
    from codenerf_amd.render import ImageStep
    g = _case("n64_16x16", 3)
    m = _model(g, "fp32")
    st = torch.nn.Parameter(torch.tensor(g["shape_table"], device=_dev()))
    tt = torch.nn.Parameter(torch.tensor(g["texture_table"], device=_dev()))
    step = ImageStep(m, chunk=int(g["chunk"]))
    step.recompute = True
    t = lambda k: torch.tensor(g[k], device=_dev())
    with pytest.raises(ValueError):
        step.forward_backward_fine(t("rays_o"), t("viewdir"), t("z_vals"), torch.zeros(3, 64, device=_dev()), t("gt"),
                                   st, tt, int(g["obj_idx"]), weight_grads=False)


# ------------------------------------------------------------------ e
NF_POSE = 16


def _fine_z_cpu(params, ro, vd, z, seed):
    """Fine samples from the fp32 oracle's coarse densities, seeded draws."""
    s, t, obj = U.codes()
    rnd = torch.tensor(U.seeded(seed).uniform(0.0, 1.0, (ro.shape[0], NF_POSE)).astype(np.float32))
    with torch.no_grad():
        xyz = ro[:, None, :] + vd[:, None, :] * z[..., None]
        sig, _ = ref_cpu.codenerf_forward(U.tparams(params, torch.float32), xyz,
                                          vd[:, None, :].expand(-1, z.shape[-1], -1), torch.tensor(s[obj:obj + 1]),
                                          torch.tensor(t[obj:obj + 1]))
        return ref_cpu.sample_pdf(sig[..., 0], z, rnd).contiguous()


def _oracle_fine_ray_grads(params, ro, vd, z, zf, gt, chunk, dtype, plan=None, reg_coef=1e-4):
    """Autograd of fine_image_step with respect to (rays_o, viewdirs); z_f a constant."""
    s, t, obj = U.codes()
    o = ro.detach().to(dtype).clone().requires_grad_()
    d = vd.detach().to(dtype).clone().requires_grad_()
    with (U.emu_context(plan) if plan else contextlib.nullcontext()):
        ref_cpu.fine_image_step(U.tparams(params, dtype), torch.tensor(s, dtype=dtype), torch.tensor(t, dtype=dtype),
                                obj, o, d, z.to(dtype), zf.to(dtype), gt.to(dtype), chunk=chunk, reg_coef=reg_coef)
    return o.grad.numpy(), d.grad.numpy()


def _gpu_fine_step(m, ro, vd, z, zf, gt, chunk, weight_grads, reg=True):
    from codenerf_amd.render import ImageStep
    s, t, obj = U.codes()
    d = U.dev()
    st = torch.nn.Parameter(torch.tensor(s, device=d))
    tt = torch.nn.Parameter(torch.tensor(t, device=d))
    for p in m.parameters():
        p.grad = None
    step = ImageStep(m, chunk=chunk, reg_coef=1e-4)
    step.last_ray_grads = None
    step.forward_backward_fine(ro.to(d), vd.to(d), z.to(d), torch.zeros(zf.shape, device=d), gt.to(d), st, tt, obj,
                               reg=reg, z_f=zf.to(d), weight_grads=weight_grads, input_grads=True)
    torch.cuda.synchronize()
    return step


def _scene(name):
    from test_gpu_inputgrad import _scene as scene
    return scene(name)


def _check(tag, gpu, emu, exact):
    e_gpu, e_emu = U.rel_l2(gpu, exact), U.rel_l2(emu, exact)
    print(f"{tag}: err_gpu {e_gpu:.3e} err_emu {e_emu:.3e} ratio {e_gpu / max(e_emu, 1e-300):.2f}")
    assert e_gpu <= U.MARGIN * e_emu, (tag, e_gpu, e_emu)


@pytest.mark.parametrize("weight_grads", [False, True], ids=["codes", "weights"])
@pytest.mark.parametrize("name", ["straddle_8x8_n48", "shared_5x5_n16", "perray_8x8_n32"])
@pytest.mark.parametrize("plan", U.PLANS)
def test_fine_ray_grads(plan, name, weight_grads):
    params = U.net_params(3, sigma_shift=2.0)
    ro, vd, z, gt = _scene(name)
    zf = _cached(("e_zf", name), lambda: _fine_z_cpu(params, ro, vd, z, 17))
    exact = _cached(("e64", name), lambda: _oracle_fine_ray_grads(params, ro, vd, z, zf, gt, 32, torch.float64))
    emu = _cached(("eemu", name, plan),
                  lambda: _oracle_fine_ray_grads(params, ro, vd, z, zf, gt, 32, torch.float32, plan))
    step = _gpu_fine_step(U.model(params, 3, precision=plan), ro, vd, z, zf, gt, 32, weight_grads)
    d_ro, d_vd = (g.cpu().numpy() for g in step.last_ray_grads)
    assert d_ro.shape == (ro.shape[0], 3) and d_vd.shape == (ro.shape[0], 3)
    path = "weights" if weight_grads else "codes"
    _check(f"fine d_rays_o {plan} {name} {path}", d_ro, emu[0], exact[0])
    _check(f"fine d_viewdirs {plan} {name} {path}", d_vd, emu[1], exact[1])


def test_fine_ray_parts_are_concatenated():
    """Two ray parts (max_rays) leave the ray gradients of the one-part run."""
    from codenerf_amd.render import ImageStep
    params = U.net_params(3, sigma_shift=2.0)
    ro, vd, z, gt = _scene("straddle_8x8_n48")
    zf = _cached(("e_zf", "straddle_8x8_n48"), lambda: _fine_z_cpu(params, ro, vd, z, 17))
    m = U.model(params, 3)
    one = _gpu_fine_step(m, ro, vd, z, zf, gt, 32, False).last_ray_grads
    s, t, obj = U.codes()
    d = U.dev()
    st = torch.nn.Parameter(torch.tensor(s, device=d))
    tt = torch.nn.Parameter(torch.tensor(t, device=d))
    step = ImageStep(m, chunk=32, reg_coef=1e-4, max_rays=32)
    step.forward_backward_fine(ro.to(d), vd.to(d), z.to(d), torch.zeros(zf.shape, device=d), gt.to(d), st, tt, obj,
                               z_f=zf.to(d), weight_grads=False, input_grads=True)
    assert step.last_ray_grads[0].shape == (64, 3) and step.last_z_f.shape == (64, NF_POSE)
    assert torch.equal(one[0], step.last_ray_grads[0]) and torch.equal(one[1], step.last_ray_grads[1])


def _pose_fine_refs():
    from test_gpu_pose import _pose_scene
    H, W, focal, z, gt, c2w0, delta0 = _pose_scene()
    params = U.net_params(3, sigma_shift=2.0)

    def c2w_of(delta, dtype):
        from codenerf_amd.pose import hat
        c0 = torch.tensor(c2w0, dtype=dtype)
        R = torch.linalg.matrix_exp(hat(delta[:3])) @ c0[:3, :3]
        return torch.cat([torch.cat([R, (c0[:3, 3] + delta[3:])[:, None]], 1), c0[3:4]], 0)

    with torch.no_grad():
        ro, vd = ref_cpu.get_rays(H, W, focal, c2w_of(torch.tensor(delta0), torch.float32))
    zf = _fine_z_cpu(params, ro, vd, z, 19)

    def delta_grad(dtype, plan=None):
        delta = torch.tensor(delta0, dtype=dtype, requires_grad=True)
        ro, vd = ref_cpu.get_rays(H, W, focal, c2w_of(delta, dtype))
        s, t, obj = U.codes()
        with (U.emu_context(plan) if plan else contextlib.nullcontext()):
            ref_cpu.fine_image_step(U.tparams(params, dtype), torch.tensor(s, dtype=dtype),
                                    torch.tensor(t, dtype=dtype), obj, ro, vd, z.to(dtype), zf.to(dtype),
                                    gt.to(dtype), chunk=H * W, reg_coef=0.0)
        return delta.grad.numpy()

    return params, zf, delta_grad


@pytest.mark.parametrize("plan", U.PLANS)
def test_fine_pose_param_chain(plan):
    """delta.grad through PoseParam -> get_rays -> the codes-only fine step ->
    two input-gradient launches -> get_rays backward, against the float64
    oracle end to end (the 8 x 8 x 32 scene of test_pose_param_chain, Nf 16)."""
    from codenerf_amd.pose import PoseParam
    from test_gpu_pose import _pose_scene
    H, W, focal, z, gt, c2w0, delta0 = _pose_scene()
    params, zf, delta_grad = _cached("pose_refs", _pose_fine_refs)
    exact = _cached("pose64", lambda: delta_grad(torch.float64))
    emu = delta_grad(torch.float32, plan)
    pp = PoseParam(torch.tensor(c2w0, device=U.dev()))
    with torch.no_grad():
        pp.delta.copy_(torch.tensor(delta0))
    ro, vd = pp.rays(H, W, focal)
    step = _gpu_fine_step(U.model(params, 3, precision=plan), ro, vd, z, zf, gt, H * W, False, reg=False)
    pp.backward_from_ray_grads(step.last_ray_grads)
    _check(f"fine delta.grad {plan}", pp.delta.grad.cpu().numpy(), emu, exact)


# ------------------------------------------------------------------ f
def _hpams(root, **extra):
    hp = {"net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "W": 256, "num_xyz_freq": 10,
                              "num_dir_freq": 4, "latent_dim": 256},
          "data": {"cat": "srn_cars", "splits": "cars_train", "data_dir": root, "n_train_views": 4,
                   "n_test_views": 3},
          "N_samples": 16, "near": 0.8, "far": 1.8, "loss_reg_coef": 1e-4,
          "lr_schedule": [{"type": "step", "lr": 1e-4, "interval": 3}, {"type": "step", "lr": 1e-3, "interval": 3}],
          "check_points": 1000, "precision": "fp32"}
    hp.update(extra)
    return hp


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The synthetic SRN set of test_optimizer_flow_with_pose, trained once
    with the fine pass (N_samples 16 + N_importance 8)."""
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.trainer import Trainer
    base = tmp_path_factory.mktemp("fine_opt")
    root, exps = str(base / "data"), str(base / "exps")
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=2, n_views=4, H=32, W=32, focal=32.8, seed=3)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    Trainer("t", 0, hpams=_hpams(root, N_importance=8), batch_size=512, check_iter=0, exp_root=exps).training(0, 2, 1)
    return root, exps


@pytest.mark.parametrize("optimize_pose", [False, True], ids=["codes", "pose"])
def test_optimizer_flow_with_the_fine_pass(trained, optimize_pose):
    from codenerf_amd.optimizer import Optimizer
    root, exps = trained
    opt = Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root, N_importance=8), batch_size=512, num_opts=4,
                    exp_root=exps)
    assert opt.n_fine == 8
    kw = dict(optimize_pose=True, pose_lr=1e-3, pose_noise=(2.0, 0.01, 7)) if optimize_pose else {}
    opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False, **kw)
    out = torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu", weights_only=True)
    keys = {"ids", "num_obj", "optimized_shapecodes", "optimized_texturecodes", "psnr_eval", "ssim_eval"}
    if optimize_pose:
        keys |= {"optimized_poses", "pose_rot_err_deg", "pose_trans_err"}
    assert set(out) == keys
    assert len(opt.psnr_opt[0]) == 4 and np.isfinite(opt.psnr_opt[0]).all()
    # three test views, two of them targets: one evaluation view
    assert len(out["psnr_eval"][0]) == 1 and np.isfinite(out["psnr_eval"][0]).all()
    assert len(out["ssim_eval"][0]) == 1 and np.isfinite(out["ssim_eval"][0]).all()
    assert opt.step_impl.last_z_f.shape == (32 * 32, 8)         # the evaluation went through render_fine
    assert torch.isfinite(out["optimized_shapecodes"]).all() and torch.isfinite(out["optimized_texturecodes"]).all()
    if optimize_pose:
        assert all(float(pp.delta.detach().abs().max()) > 0 for pp in opt.pose_params)


def test_optimizer_n_importance_override_and_off(trained):
    """n_importance overrides the JSON; N_importance 0 and the key left out
    are the same coarse-only loop: two seeded runs give the same codes."""
    from codenerf_amd.optimizer import Optimizer
    root, exps = trained
    assert Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root, N_importance=8), batch_size=512, num_opts=1,
                     exp_root=exps, n_importance=0).n_fine == 0
    assert Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root), batch_size=512, num_opts=1, exp_root=exps,
                     n_importance=4).n_fine == 4
    codes = []
    for hp in (_hpams(root, N_importance=0), _hpams(root)):
        torch.manual_seed(0)
        opt = Optimizer("t", 0, [0, 1], "test", hpams=hp, batch_size=512, num_opts=3, exp_root=exps)
        assert opt.n_fine == 0
        opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False)
        assert getattr(opt.step_impl, "last_z_f", None) is None
        codes.append((opt.optimized_shapecodes.clone(), opt.optimized_texturecodes.clone(),
                      list(opt.psnr_eval[0])))
    assert torch.equal(codes[0][0], codes[1][0]) and torch.equal(codes[0][1], codes[1][1])
    assert codes[0][2] == codes[1][2]
