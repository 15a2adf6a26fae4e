"""Input gradients on the GPU: per-sample d_xyz / d_viewdir (cn_mlp_input_grad
behind cn_mlp_bwd_pose) and the per-ray sums behind ImageStep, against a
float64 replay of the oracle.

The bar is computed per case (inputgrad_util): err_gpu <= 2 err_emu, both
rel-L2 against the float64 replay, err_emu from the oracle in fp32 under the
plan's operand rounding.  Every case prints both errors.  The per-sample
comparisons leave out the ~1 % of samples whose float64 pre-activation sits at
a ReLU kink (inputgrad_util.KINK): there the gradient is discontinuous and any
fp32 arithmetic, the CPU oracle's included, lands on either side.
"""
import numpy as np
import pytest
import torch

import inputgrad_util as U

pytestmark = pytest.mark.gpu

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _check(tag, gpu, emu, exact):
    e_gpu, e_emu = U.rel_l2(gpu, exact), U.rel_l2(emu, exact)
    print(f"{tag}: err_gpu {e_gpu:.3e} err_emu {e_emu:.3e} ratio {e_gpu / max(e_emu, 1e-300):.2f}")
    assert e_gpu <= U.MARGIN * e_emu, (tag, e_gpu, e_emu)
    return e_gpu, e_emu


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("M", [400, 3072])
@pytest.mark.parametrize("sb", [3, 2])
@pytest.mark.parametrize("plan", U.PLANS)
def test_per_sample_grads(plan, sb, M):
    """Mode A, random upstream gradients, every plan and both nets; M = 400
    pads to 512 (rows >= M must come back 0), M = 3072 is whole tiles over
    several workgroups."""
    params = U.net_params(sb)
    xyz, v, dsig, drgb = U.sample_inputs(M)
    exact = _cached(("s64", sb, M), lambda: U.oracle_sample_grads(params, sb, 1, xyz, v, dsig, drgb, torch.float64,
                                                                  with_kink=True))
    emu = _cached(("semu", plan, sb, M),
                  lambda: U.oracle_sample_grads(params, sb, 1, xyz, v, dsig, drgb, torch.float32, plan))
    gx, gv, px, pv = U.gpu_sample_grads(U.model(params, sb, precision=plan), xyz, v, dsig, drgb)
    assert not px.any() and not pv.any()
    ok = ~exact[2]          # samples at a ReLU kink are not comparable (inputgrad_util.KINK)
    assert ok.sum() >= 0.97 * M
    _check(f"d_xyz {plan} ({sb},1) M={M}", gx[ok], emu[0][ok], exact[0][ok])
    _check(f"d_viewdir {plan} ({sb},1) M={M}", gv[ok], emu[1][ok], exact[1][ok])


# ------------------------------------------------------------------ 2
_XYZ_GROUPS = {"raw": list(range(0, 3)), "sin": list(range(3, 33)), "cos": list(range(33, 63)),
               "top": [30, 31, 32, 60, 61, 62]}
_DIR_GROUPS = {"raw": list(range(0, 3)), "sin": list(range(3, 15)), "cos": list(range(15, 27))}


@pytest.mark.parametrize("which,group", [("xyz", g) for g in _XYZ_GROUPS] + [("dir", g) for g in _DIR_GROUPS])
def test_slot_mapping(which, group):
    """fp32 plan, all input columns of one encoding zeroed but one term
    family: that family is the whole gradient, so a dropped or mis-slotted
    family is a 100 % error."""
    M = 400
    params = dict(U.net_params(3))
    if which == "xyz":
        w = params["encoding_xyz.0.weight"].copy()
        keep = np.zeros(63, bool)
        keep[_XYZ_GROUPS[group]] = True
        w[:, ~keep] = 0
        params["encoding_xyz.0.weight"] = w
    else:
        w = params["encoding_viewdir.0.weight"].copy()
        keep = np.ones(283, bool)
        keep[256:] = False
        keep[[256 + c for c in _DIR_GROUPS[group]]] = True
        w[:, ~keep] = 0
        params["encoding_viewdir.0.weight"] = w
    xyz, v, dsig, drgb = U.sample_inputs(M)
    exact = U.oracle_sample_grads(params, 3, 1, xyz, v, dsig, drgb, torch.float64, with_kink=True)
    emu = U.oracle_sample_grads(params, 3, 1, xyz, v, dsig, drgb, torch.float32, "fp32")
    gx, gv, _, _ = U.gpu_sample_grads(U.model(params, 3), xyz, v, dsig, drgb)
    k = 0 if which == "xyz" else 1
    ok = ~exact[2]
    assert ok.sum() >= 0.97 * M and np.linalg.norm(exact[k][ok]) > 0
    _check(f"slot {which}/{group}", (gx, gv)[k][ok], emu[k][ok], exact[k][ok])


# ------------------------------------------------------------------ 3
def _scene(name):
    """(ro, vd, z, gt) of a ray case; chunk 32 everywhere."""
    H, W, N, per_ray = {"straddle_8x8_n48": (8, 8, 48, False), "shared_5x5_n16": (5, 5, 16, False),
                        "perray_8x8_n32": (8, 8, 32, True)}[name]
    ro, vd, _ = U.camera_rays(H, W)
    rng = U.seeded(5)
    z = torch.linspace(0.8, 1.8, N)
    if per_ray:
        z = (z[None, :] + torch.tensor(rng.uniform(0.0, 1.0 / (2 * N), (H * W, N)), dtype=torch.float32)).contiguous()
    gt = torch.tensor(rng.uniform(0.0, 1.0, (H * W, 3)).astype(np.float32))
    return ro, vd, z, gt


def _ray_refs(name, plan, sb):
    params = U.net_params(sb, sigma_shift=2.0)
    ro, vd, z, gt = _scene(name)
    exact = _cached(("r64", name, sb), lambda: U.oracle_ray_grads(params, sb, 1, ro, vd, z, gt, 32, torch.float64))
    emu = _cached(("remu", name, plan, sb),
                  lambda: U.oracle_ray_grads(params, sb, 1, ro, vd, z, gt, 32, torch.float32, plan))
    return params, (ro, vd, z, gt), exact, emu


@pytest.mark.parametrize("name,sb", [("straddle_8x8_n48", 3), ("shared_5x5_n16", 3), ("perray_8x8_n32", 3),
                                     ("straddle_8x8_n48", 2)])
@pytest.mark.parametrize("plan", U.PLANS)
def test_per_ray_grads(plan, name, sb):
    """Mode B through ImageStep.forward_backward(input_grads=True,
    weight_grads=False), chunk 32: a ray straddling slabs (N = 48), two rays
    per slab with M = 400 and a ragged last chunk (5 x 5 x 16), per-ray z."""
    params, scene, exact, emu = _ray_refs(name, plan, sb)
    r = U.gpu_image_step(U.model(params, sb, precision=plan), *scene, 32)
    # (sanity only: the same scene was rendered; bf16 rgb is good to ~3e-2 absolute)
    np.testing.assert_allclose(r["losses"], exact[2], rtol=0.15 if plan == "bf16" else 1e-3)
    _check(f"d_rays_o {plan} {name} ({sb},1)", r["d_ro"], emu[0], exact[0])
    _check(f"d_viewdirs {plan} {name} ({sb},1)", r["d_vd"], emu[1], exact[1])


@pytest.mark.parametrize("plan", U.PLANS)
def test_rows_of_a_larger_workspace(plan):
    """The C-ABI path with act_row0 = 256 and act_M > M computes what the same
    call at row 0 of a workspace of its own does, bit for bit."""
    params = U.net_params(3)
    xyz, v, dsig, drgb = U.sample_inputs(400)
    m = U.model(params, 3, precision=plan)
    a = U.gpu_sample_grads(m, xyz, v, dsig, drgb)
    b = U.gpu_sample_grads(m, xyz, v, dsig, drgb, act_M=1024, row0=256)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_bad_rows_are_refused():
    import ctypes
    from codenerf_amd import _lib
    m = U.model(U.net_params(3), 3)
    eng = m.engine()
    eng.ensure_packed(m.param_list())
    L, d = eng.L, ctypes.c_void_p(256)          # never dereferenced: validation comes first
    args = (d, d, None, None, None, 0, 0, d, d, None, None, None)
    assert L.cn_mlp_input_grad(eng._plan, d, d, 512, 128, 256, *args) == -1
    assert b"multiple of the tile" in L.cn_last_error()
    assert L.cn_mlp_input_grad(eng._plan, d, d, 512, 256, 400, *args) == -1
    assert b"exceed the activation workspace" in L.cn_last_error()
    assert L.cn_mlp_input_grad(eng._plan, d, d, 512, 0, 0, *args) == -1
    assert _lib.ABI_VERSION == 4


@pytest.mark.parametrize("plan", U.PLANS)
def test_weight_path_keeps_its_gradients(plan):
    """weight_grads=True with input_grads=True: the ray gradients come from
    the training backward's planes (same bar), and the parameter and code
    gradients are bit-identical to the call without input_grads."""
    name, sb = "straddle_8x8_n48", 3
    params, scene, exact, emu = _ray_refs(name, plan, sb)
    m = U.model(params, sb, precision=plan)
    off = U.gpu_image_step(m, *scene, 32, input_grads=False, weight_grads=True)
    on = U.gpu_image_step(m, *scene, 32, input_grads=True, weight_grads=True)
    for a, b in zip(off["dparams"] + [off["ds"], off["dt"], off["losses"], off["rgb"]],
                    on["dparams"] + [on["ds"], on["dt"], on["losses"], on["rgb"]]):
        np.testing.assert_array_equal(a, b)
    _check(f"d_rays_o {plan} weight path", on["d_ro"], emu[0], exact[0])
    _check(f"d_viewdirs {plan} weight path", on["d_vd"], emu[1], exact[1])


def test_ray_parts_are_concatenated():
    """An image rendered in two ray parts (max_rays) leaves the ray gradients
    of the one-part run, in ray order."""
    from codenerf_amd.render import ImageStep
    params, scene, _, _ = _ray_refs("straddle_8x8_n48", "fp32", 3)
    m = U.model(params, 3)
    one = U.gpu_image_step(m, *scene, 32)
    two = U.gpu_image_step(m, *scene, 32, step=ImageStep(m, chunk=32, reg_coef=1e-4, max_rays=32))
    assert two["d_ro"].shape == (64, 3)
    np.testing.assert_array_equal(one["d_ro"], two["d_ro"])
    np.testing.assert_array_equal(one["d_vd"], two["d_vd"])
    np.testing.assert_array_equal(one["losses"], two["losses"])


# ------------------------------------------------------------------ 4, 5
@pytest.mark.parametrize("plan", ["fp32", "bf16"])
def test_deterministic(plan):
    from codenerf_amd import engine as E
    params, scene, _, _ = _ray_refs("straddle_8x8_n48", plan, 3)
    m = U.model(params, 3, precision=plan)
    a = U.gpu_image_step(m, *scene, 32)
    b = U.gpu_image_step(m, *scene, 32)
    np.testing.assert_array_equal(a["d_ro"], b["d_ro"])
    np.testing.assert_array_equal(a["d_vd"], b["d_vd"])
    c2w = torch.tensor(U.camera_rays(8, 8)[2], device=U.dev())[:3].contiguous()
    g = [torch.tensor(a[k], device=U.dev()) for k in ("d_ro", "d_vd")]
    d1 = E.get_rays_bwd(8, 8, 9.6, False, c2w, *g)
    d2 = E.get_rays_bwd(8, 8, 9.6, False, c2w, *g)
    assert torch.equal(d1, d2) and torch.isfinite(d1).all()


@pytest.mark.parametrize("plan", ["fp32", "bf16"])
def test_off_means_off(plan):
    """forward_backward(weight_grads=False) without input_grads gives the same
    bits before and after a pose call on the same ImageStep."""
    params, scene, _, _ = _ray_refs("shared_5x5_n16", plan, 3)
    m = U.model(params, 3, precision=plan)
    before = U.gpu_image_step(m, *scene, 32, input_grads=False)
    U.gpu_image_step(m, *scene, 32, input_grads=True, step=before["step"])
    after = U.gpu_image_step(m, *scene, 32, input_grads=False, step=before["step"])
    for k in ("losses", "rgb", "ds", "dt"):
        np.testing.assert_array_equal(before[k], after[k])
