"""CPU tier of pose refinement: the PoseParam parametrisation under plain torch
autograd, and the optimize.py / codes.pth surface with the feature off."""
import importlib.util
import os

import numpy as np
import torch

from oracle.params import look_at_pose

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c2w0():
    return torch.tensor(look_at_pose(1.3, 35, 20))


def test_zero_delta_is_the_start_pose():
    from codenerf_amd import PoseParam
    c = _c2w0()
    pp = PoseParam(c)
    assert pp.delta.shape == (6,) and pp.delta.requires_grad
    assert torch.equal(pp.c2w().detach(), c)
    assert pp.errors(c) == (0.0, 0.0)


def test_rotation_stays_orthonormal():
    from codenerf_amd.pose import PoseParam
    pp = PoseParam(_c2w0())
    rng = np.random.Generator(np.random.PCG64(2))
    worst = 0.0
    for _ in range(100):
        with torch.no_grad():
            pp.delta += torch.tensor(0.1 * rng.standard_normal(6), dtype=torch.float32)
        R = pp.c2w().detach()[:3, :3].double()
        worst = max(worst, float((R.T @ R - torch.eye(3, dtype=torch.float64)).abs().max()))
        assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-6
    assert worst < 1e-6, worst
    assert torch.equal(pp.c2w().detach()[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))


def test_delta_grad_matches_finite_difference():
    """A quadratic in c2w: autograd through PoseParam against a float64
    central difference of the same parametrisation."""
    from codenerf_amd.pose import PoseParam, hat
    c0 = _c2w0()
    rng = np.random.Generator(np.random.PCG64(3))
    A = torch.tensor(rng.standard_normal((4, 4)))
    d0 = 0.2 * rng.standard_normal(6)

    def f64(delta):
        d = torch.tensor(delta, dtype=torch.float64)
        R = torch.linalg.matrix_exp(hat(d[:3])) @ c0[:3, :3].double()
        c = torch.cat([torch.cat([R, (c0[:3, 3].double() + d[3:])[:, None]], 1), c0[3:4].double()], 0)
        return float(((c - A) ** 2).sum())

    pp = PoseParam(c0)
    with torch.no_grad():
        pp.delta.copy_(torch.tensor(d0, dtype=torch.float32))
    ((pp.c2w().double() - A) ** 2).sum().backward()
    base = pp.delta.detach().double().numpy()
    fd = np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-5
        fd[k] = (f64(base + e) - f64(base - e)) / 2e-5
    np.testing.assert_allclose(pp.delta.grad.numpy(), fd, rtol=1e-4, atol=1e-5)


def test_perturb_pose_is_seeded_and_sized():
    from codenerf_amd.pose import perturb_pose, pose_errors
    c = _c2w0()
    a, b = perturb_pose(c, 3.0, 0.02, 4), perturb_pose(c, 3.0, 0.02, 4)
    assert torch.equal(a, b) and not torch.equal(a, perturb_pose(c, 3.0, 0.02, 5))
    rot, tr = pose_errors(a, c)
    assert abs(rot - 3.0) < 1e-3 and 0.0 < tr < 0.02 * 5


def _optimize_module():
    spec = importlib.util.spec_from_file_location("optimize_cli", os.path.join(REPO, "optimize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_flags():
    ap = _optimize_module().build_parser()
    txt = ap.format_help()
    for flag in ("--optimize_pose", "--pose_lr", "--pose_noise_deg", "--pose_noise_trans"):
        assert flag in txt, flag
    a = ap.parse_args([])
    # the reference CLI's flags keep their dests and (untyped) defaults
    assert {k: getattr(a, k) for k in ("gpu", "saved_dir", "tgt_instances", "splits", "num_opts", "lr",
                                       "lr_half_interval", "save_img", "jsonfile", "batchsize")} == dict(
        gpu=0, saved_dir="srncar", tgt_instances=[1], splits="test", num_opts=200, lr=1e-2, lr_half_interval=50,
        save_img=True, jsonfile="srncar.json", batchsize=2048)
    assert a.optimize_pose is False and a.pose_lr == 1e-3 and a.pose_noise_deg == 0.0 and a.pose_noise_trans == 0.0
    b = ap.parse_args(["--optimize_pose", "True", "--pose_noise_deg", "3"])
    assert b.optimize_pose is True and b.pose_noise_deg == 3.0


def test_codes_pth_keys_unchanged_when_off():
    from codenerf_amd.optimizer import Optimizer
    o = Optimizer.__new__(Optimizer)
    o.ids = ["a"]
    o.optimized_shapecodes = o.optimized_texturecodes = torch.zeros(1, 256)
    o.psnr_eval, o.ssim_eval = {}, {}
    ref_keys = ["ids", "num_obj", "optimized_shapecodes", "optimized_texturecodes", "psnr_eval", "ssim_eval"]
    assert list(o.saved_dict(0)) == ref_keys
    o.optimize_pose = False
    assert list(o.saved_dict(0)) == ref_keys
    o.optimize_pose = True
    o.optimized_poses, o.pose_rot_err, o.pose_trans_err = {}, {}, {}
    assert list(o.saved_dict(0)) == ref_keys + ["optimized_poses", "pose_rot_err_deg", "pose_trans_err"]
