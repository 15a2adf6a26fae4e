"""Pose gradients and pose refinement on the GPU: the get_rays backward against
float64 autograd of the oracle, the PoseParam chain end to end (pose -> rays ->
image loss), and a pose-recovery run."""
import contextlib

import numpy as np
import pytest
import torch

import inputgrad_util as U
from oracle import ref_cpu
from oracle.params import look_at_pose

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("focal_f64", [False, True])
@pytest.mark.parametrize("H,W", [(7, 5), (16, 16)])
def test_get_rays_bwd(H, W, focal_f64):
    """Closed form with a float64 reduction: rtol 1e-5 of max |d_c2w| (the bar
    of the compositing-backward test)."""
    from codenerf_amd import engine as E
    rng = U.seeded(21)
    c2w = look_at_pose(1.3, 35, 20)
    g_ro = rng.standard_normal((H * W, 3)).astype(np.float32)
    g_vd = rng.standard_normal((H * W, 3)).astype(np.float32)
    f = 1.2 * H
    c = torch.tensor(c2w, dtype=torch.float64, requires_grad=True)
    focal = torch.tensor([f], dtype=torch.float64) if focal_f64 else f
    ro, vd = ref_cpu.get_rays(H, W, focal, c)
    torch.autograd.backward([ro, vd], [torch.tensor(g_ro, dtype=torch.float64), torch.tensor(g_vd, dtype=torch.float64)])
    want = c.grad[:3].numpy()
    d = U.dev()
    got = E.get_rays_bwd(H, W, f, focal_f64, torch.tensor(c2w, device=d)[:3].contiguous(),
                         torch.tensor(g_ro, device=d), torch.tensor(g_vd, device=d)).cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"get_rays_bwd {H}x{W} f64={focal_f64}: max err {err:.3e} of max |d_c2w|")
    assert err <= 1e-5


def test_get_rays_autograd():
    """utils.get_rays with a c2w that requires grad goes through the HIP
    backward; without, it is the plain forward (same bits)."""
    from codenerf_amd.utils import get_rays
    d = U.dev()
    c2w = torch.tensor(look_at_pose(1.3, 35, 20), device=d)
    ro0, vd0 = get_rays(7, 5, 8.4, c2w)
    c = c2w.clone().requires_grad_()
    ro, vd = get_rays(7, 5, 8.4, c)
    assert torch.equal(ro, ro0) and torch.equal(vd, vd0) and not ro0.requires_grad
    (ro.sum() + (vd * vd0).sum()).backward()
    assert c.grad.shape == (4, 4) and not c.grad[3].any()
    np.testing.assert_allclose(c.grad[:3, 3].cpu().numpy(), 35.0, rtol=1e-6)


# ------------------------------------------------------------------ 7
def _pose_scene():
    H = W = 8
    N = 32
    rng = U.seeded(9)
    gt = torch.tensor(rng.uniform(0.0, 1.0, (H * W, 3)).astype(np.float32))
    delta = (0.03 * rng.standard_normal(6)).astype(np.float32)
    return H, W, 1.2 * H, torch.linspace(0.8, 1.8, N), gt, look_at_pose(1.3, 35, 20), delta


def _oracle_delta_grad(params, dtype, plan=None):
    from codenerf_amd.pose import hat
    H, W, focal, z, gt, c2w0, delta0 = _pose_scene()
    delta = torch.tensor(delta0, dtype=dtype, requires_grad=True)
    c0 = torch.tensor(c2w0, dtype=dtype)
    R = torch.linalg.matrix_exp(hat(delta[:3])) @ c0[:3, :3]
    c2w = torch.cat([torch.cat([R, (c0[:3, 3] + delta[3:])[:, None]], 1), c0[3:4]], 0)
    ro, vd = ref_cpu.get_rays(H, W, focal, c2w)
    s, t, obj = U.codes()
    with (U.emu_context(plan) if plan else contextlib.nullcontext()):
        ref_cpu.image_step(U.tparams(params, dtype), torch.tensor(s, dtype=dtype), torch.tensor(t, dtype=dtype), obj,
                           ro, vd, z.to(dtype), gt.to(dtype), chunk=H * W, reg_coef=0.0)
    return delta.grad.numpy()


@pytest.mark.parametrize("plan", U.PLANS)
def test_pose_param_chain(plan):
    """delta.grad through PoseParam -> HIP get_rays -> ImageStep -> input
    gradients -> get_rays backward, against the float64 oracle end to end."""
    from codenerf_amd.pose import PoseParam
    H, W, focal, z, gt, c2w0, delta0 = _pose_scene()
    params = U.net_params(3, sigma_shift=2.0)
    exact = _oracle_delta_grad(params, torch.float64)
    emu = _oracle_delta_grad(params, torch.float32, plan)
    m = U.model(params, 3, precision=plan)
    pp = PoseParam(torch.tensor(c2w0, device=U.dev()))
    with torch.no_grad():
        pp.delta.copy_(torch.tensor(delta0))
    ro, vd = pp.rays(H, W, focal)
    r = U.gpu_image_step(m, ro, vd, z, gt, H * W, reg=False)
    pp.backward_from_ray_grads(r["step"].last_ray_grads)
    got = pp.delta.grad.cpu().numpy()
    e_gpu, e_emu = U.rel_l2(got, exact), U.rel_l2(emu, exact)
    print(f"delta.grad {plan}: err_gpu {e_gpu:.3e} err_emu {e_emu:.3e} ratio {e_gpu / e_emu:.2f}")
    assert e_gpu <= U.MARGIN * e_emu, (e_gpu, e_emu)


def test_optimizer_flow_with_pose(tmp_path):
    """Optimizer.optimize_objs(optimize_pose=True) on a synthetic SRN set: the
    loop runs, every view's pose moves, codes.pth gains the pose keys."""
    import os
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.optimizer import Optimizer
    from codenerf_amd.trainer import Trainer
    root = str(tmp_path / "data")
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=2, n_views=4, H=32, W=32, focal=32.8, seed=3)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    hp = {"net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "W": 256, "num_xyz_freq": 10,
                              "num_dir_freq": 4, "latent_dim": 256},
          "data": {"cat": "srn_cars", "splits": "cars_train", "data_dir": root, "n_train_views": 4,
                   "n_test_views": 3},
          "N_samples": 16, "near": 0.8, "far": 1.8, "loss_reg_coef": 1e-4,
          "lr_schedule": [{"type": "step", "lr": 1e-4, "interval": 3}, {"type": "step", "lr": 1e-3, "interval": 3}],
          "check_points": 1000, "N_importance": 0, "precision": "fp32"}
    exps = str(tmp_path / "exps")
    Trainer("t", 0, hpams=hp, batch_size=512, check_iter=0, exp_root=exps).training(0, 2, 1)
    opt = Optimizer("t", 0, [0, 1], "test", hpams=hp, batch_size=512, num_opts=4, exp_root=exps)
    opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False, optimize_pose=True, pose_lr=1e-3,
                      pose_noise=(2.0, 0.01, 7))
    out = torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu", weights_only=True)
    assert set(out) == {"ids", "num_obj", "optimized_shapecodes", "optimized_texturecodes", "psnr_eval",
                        "ssim_eval", "optimized_poses", "pose_rot_err_deg", "pose_trans_err"}
    assert out["optimized_poses"][0].shape == (2, 4, 4)
    assert len(out["pose_rot_err_deg"][0]) == 2 and np.isfinite(out["pose_rot_err_deg"][0]).all()
    # started 2 degrees off; four small steps leave it near there, moved
    assert all(1.0 < e < 3.0 for e in out["pose_rot_err_deg"][0])
    assert all(float(pp.delta.detach().abs().max()) > 0 for pp in opt.pose_params)
    assert len(opt.psnr_opt[0]) == 4 and np.isfinite(opt.psnr_opt[0]).all()


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("plan", U.PLANS)
def test_pose_recovery(plan):
    """16 x 16 image rendered by the oracle at the true pose; the start is 3
    degrees and 0.02 off; 60 Adam steps on delta (codes fixed, one chunk, no
    regulariser).  Gate (fp32 plan): loss <= 0.1 x initial and rotation error
    <= 1 degree -- the oracle alone on the CPU: loss 1.02e-6 -> 2.4e-9,
    3.00 -> 0.105 degrees.  Translation is not recovered on this random-weight
    scene (0.035 -> 0.049 on the CPU): printed, not gated.  The loss scale of
    1e-6 sits under the bf16 rgb error, so the other plans print their trace
    ungated."""
    from codenerf_amd.pose import PoseParam, perturb_pose, pose_errors
    from codenerf_amd.render import ImageStep
    H = W = 16
    focal = 1.2 * H
    z = torch.linspace(0.8, 1.8, 32)
    params = U.net_params(3, sigma_shift=2.0)
    s, t, obj = U.codes()
    true = look_at_pose(1.3, 35, 20)
    with torch.no_grad():
        ro, vd = ref_cpu.get_rays(H, W, focal, true)
        xyz = ro[:, None, :] + vd[:, None, :] * z[:, None]
        sig, rgbs = ref_cpu.codenerf_forward(U.tparams(params, torch.float32), xyz, vd[:, None, :].expand(-1, 32, -1),
                                             torch.tensor(s[obj:obj + 1]), torch.tensor(t[obj:obj + 1]))
        gt, _ = ref_cpu.volume_rendering(sig, rgbs, z)
    d = U.dev()
    m = U.model(params, 3, precision=plan)
    st = torch.nn.Parameter(torch.tensor(s, device=d))
    tt = torch.nn.Parameter(torch.tensor(t, device=d))
    step = ImageStep(m, chunk=H * W, reg_coef=0.0)
    pp = PoseParam(perturb_pose(true, 3.0, 0.02, 4).to(d))
    opt = torch.optim.Adam([pp.delta], lr=5e-3)
    gt_d, z_d = gt.to(d), z.to(d)
    trace = []
    for it in range(61):
        rot, tr = pp.errors(true)
        opt.zero_grad()
        ro_d, vd_d = pp.rays(H, W, focal)
        losses, _, _ = step.forward_backward(ro_d, vd_d, z_d, gt_d, st, tt, obj, reg=False, weight_grads=False,
                                             input_grads=True)
        trace.append((float(losses.mean()), rot, tr))
        if it == 60:
            break
        pp.backward_from_ray_grads(step.last_ray_grads)
        opt.step()
    for it in (0, 10, 20, 40, 60):
        print(f"pose recovery {plan} step {it}: loss {trace[it][0]:.3e} rot {trace[it][1]:.3f} deg "
              f"trans {trace[it][2]:.4f}")
    assert abs(trace[0][1] - 3.0) < 1e-2 and np.isfinite([x[0] for x in trace]).all()
    if plan == "fp32":
        assert trace[60][0] <= 0.1 * trace[0][0], (trace[0], trace[60])
        assert trace[60][1] <= 1.0, trace[60]
