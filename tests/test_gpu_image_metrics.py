"""GPU: the device evaluation metrics -- cn_image_metrics through
codenerf_amd.metrics.image_metrics, and Optimizer(device_metrics=True).

The definition is metrics.ssim_legacy (float64 numpy / scipy) on the same
float32 arrays, and a float64 numpy restatement of the chunk-mean MSE.

Bars:
  * ssim: |d| <= 1e-10.  Both sides are float64 and differ in summation order
    only; the worst cancellation, uxx - ux^2 at magnitude <= 1, is divided by
    C2 = 3.6e-3: about 1e-13, three orders inside the bar;
  * mse and the chunk means: 1e-12 relative to the float64 restatement (sums
    of <= 3 * 128 * 128 non-negative terms: <= n eps / 2 = 5.5e-12 for any
    order in the worst case, ~ sqrt(n) eps = 5e-14 for the tree sums here);
  * mse against the Optimizer's present fp32 expression: 1e-5 relative (fp32
    rounding of sums of <= 6144 terms);
  * identical images: ssim within 1e-12 of 1, mse exactly 0;
  * constant images 0.3 against 0.5: the closed form of tests/test_metrics.py
    on the float32 values within 1e-12, mse within 1e-8 of 0.04 (float32(0.3)
    is off by <= 1.5e-8, d mse = 2 * 0.2 * that = 6e-9);
  * a view's numbers do not depend on the views beside it, and a repeated
    call gives the same bits.
"""
import os

import numpy as np
import pytest
import torch

from codenerf_amd.metrics import image_metrics, psnr, ssim_legacy

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (8, 23), (32, 32), (37, 70)]        # (7, 7): one window; (37, 70): no multiple of a tile
KINDS = ["noise", "white", "const"]
CASES = [(H, W, V, chunk, kind) for (H, W) in SHAPES for V in (1, 3) for chunk in (2048, 100, "above")
         for kind in KINDS] + [(128, 128, 3, 2048, "noise")]

_cache = {}


def _dev():
    return torch.device("cuda", 0)


def _images(kind, H, W, V=3):
    """float32 (V, H*W, 3) pairs, made once per (kind, shape); V = 1 takes view 0."""
    key = ("img", kind, H, W)
    if key not in _cache:
        rng = np.random.default_rng(H * 1000 + W)
        if kind == "noise":
            a = rng.random((V, H, W, 3))
            b = np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1)
        elif kind == "white":
            # the SRN look: white background, a textured rectangle
            a = np.ones((V, H, W, 3))
            a[:, H // 4:H - H // 4, W // 4:W - W // 4] = rng.random((V, H - 2 * (H // 4), W - 2 * (W // 4), 3))
            b = np.clip(a + rng.normal(0, 0.05, a.shape), 0, 1)
        else:
            a, b = np.full((V, H, W, 3), 0.3), np.full((V, H, W, 3), 0.5)
        _cache[key] = (a.astype(np.float32).reshape(V, H * W, 3), b.astype(np.float32).reshape(V, H * W, 3))
    return _cache[key]


def _reference(kind, H, W, chunk):
    """Per view: ssim_legacy, the float64 chunk means and their mean."""
    key = ("ref", kind, H, W, chunk)
    if key not in _cache:
        a, b = _images(kind, H, W)
        ssim = [ssim_legacy(x.reshape(H, W, 3), y.reshape(H, W, 3)) for x, y in zip(a, b)]
        d2 = (a.astype(np.float64) - b.astype(np.float64)) ** 2
        cm = np.array([[d2[v, i:i + chunk].mean() for i in range(0, H * W, chunk)] for v in range(a.shape[0])])
        _cache[key] = (np.array(ssim), cm, cm.mean(axis=1))
    return _cache[key]


def _present_loop_mse(rgb, tgt, B):
    """The Optimizer's present fp32 expression, on the device."""
    se = ((rgb - tgt) ** 2).sum(-1)
    return float(np.mean([float(se[i:i + B].mean()) / 3 for i in range(0, rgb.shape[0], B)]))


def _run(a, b, H, W, chunk):
    img, gt = torch.tensor(a, device=_dev()), torch.tensor(b, device=_dev())
    V = 1 if img.dim() == 2 else img.shape[0]
    cm = torch.full((V, -(-H * W // chunk)), float("nan"), dtype=torch.float64, device=_dev())
    out = image_metrics(img, gt, H, W, chunk, chunk_mse=cm)
    assert out.shape == (V, 2) and out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy(), cm.cpu().numpy(), img, gt


@pytest.mark.parametrize("H,W,V,chunk,kind", CASES)
def test_image_metrics_match_the_host_definition(H, W, V, chunk, kind):
    chunk = H * W + 5 if chunk == "above" else chunk
    a, b = (x[:V] for x in _images(kind, H, W))
    ssim_ref, cm_ref, mse_ref = (x[:V] for x in _reference(kind, H, W, chunk))
    out, cm, img, gt = _run(a, b, H, W, chunk)
    d_ssim = np.abs(out[:, 1] - ssim_ref).max()
    r_mse = (np.abs(out[:, 0] - mse_ref) / mse_ref).max()
    r_cm = (np.abs(cm - cm_ref) / cm_ref).max()
    loop = np.array([_present_loop_mse(img[v], gt[v], chunk) for v in range(V)])
    r_loop = (np.abs(out[:, 0] - loop) / loop).max()
    print(f"{H}x{W} V {V} chunk {chunk} {kind}: ssim max|d| {d_ssim:.2e} mse rel {r_mse:.2e} chunk rel {r_cm:.2e} "
          f"vs fp32 loop rel {r_loop:.2e}")
    assert cm.shape == cm_ref.shape
    assert d_ssim <= 1e-10
    assert r_mse <= 1e-12 and r_cm <= 1e-12
    assert r_loop <= 1e-5
    if kind == "const":
        p, q, C1 = float(np.float32(0.3)), float(np.float32(0.5)), (0.01 * 2.0) ** 2
        assert np.abs(out[:, 1] - (2 * p * q + C1) / (p * p + q * q + C1)).max() <= 1e-12
        assert np.abs(out[:, 0] - 0.04).max() <= 1e-8


def test_one_view_may_be_two_dimensional():
    a, b = _images("noise", 8, 23)
    full, _, _, _ = _run(a[:1], b[:1], 8, 23, 100)
    flat, _, _, _ = _run(a[0], b[0], 8, 23, 100)
    assert np.array_equal(full, flat)


@pytest.mark.parametrize("kind", ["noise", "white"])
@pytest.mark.parametrize("H,W", [(7, 7), (37, 70)])
def test_identical_images(H, W, kind):
    a, _ = _images(kind, H, W)
    out, cm, _, _ = _run(a, a, H, W, 100)
    print(f"{H}x{W} {kind}: max|ssim - 1| {np.abs(out[:, 1] - 1).max():.2e}")
    assert np.abs(out[:, 1] - 1.0).max() <= 1e-12
    assert (out[:, 0] == 0.0).all() and (cm == 0.0).all()


@pytest.mark.parametrize("H,W,chunk", [(37, 70, 100), (37, 70, 2048), (128, 128, 2048)])
def test_a_view_does_not_depend_on_its_batch(H, W, chunk):
    a, b = _images("white", H, W)
    out3, cm3, _, _ = _run(a, b, H, W, chunk)
    again, cm_again, _, _ = _run(a, b, H, W, chunk)
    assert np.array_equal(out3, again) and np.array_equal(cm3, cm_again)
    for v in range(3):
        out1, cm1, _, _ = _run(a[v:v + 1], b[v:v + 1], H, W, chunk)
        assert np.array_equal(out1[0], out3[v]) and np.array_equal(cm1[0], cm3[v]), v


def test_out_is_a_slice_of_a_larger_buffer():
    a, b = _images("noise", 32, 32)
    img, gt = torch.tensor(a, device=_dev()), torch.tensor(b, device=_dev())
    buf = torch.full((5, 2), float("nan"), dtype=torch.float64, device=_dev())
    ret = image_metrics(img[1], gt[1], 32, 32, 2048, out=buf[2:3])
    assert ret.data_ptr() == buf[2:3].data_ptr()
    alone = image_metrics(img[1:2], gt[1:2], 32, 32, 2048)
    assert torch.equal(buf[2:3], alone)
    assert torch.isnan(buf[:2]).all() and torch.isnan(buf[3:]).all()
    # psnr of column 0 is the loop's PSNR
    assert abs(psnr(float(buf[2, 0])) - (-10 * np.log10(_reference("noise", 32, 32, 2048)[2][1]))) < 1e-9


def test_arguments_are_checked():
    from codenerf_amd._lib import CnError
    x = torch.zeros(49, 3, device=_dev())
    with pytest.raises(ValueError):
        image_metrics(x, x[:48], 7, 7, 2048)
    with pytest.raises(ValueError):
        image_metrics(x.double(), x.double(), 7, 7, 2048)
    with pytest.raises(ValueError):
        image_metrics(x, x, 7, 7, 2048, out=torch.zeros(1, 2, device=_dev()))
    with pytest.raises(CnError, match="at least 7"):
        image_metrics(torch.zeros(36, 3, device=_dev()), torch.zeros(36, 3, device=_dev()), 6, 6, 2048)
    with pytest.raises(CnError, match="chunk"):
        image_metrics(x, x, 7, 7, 0)


# ------------------------------------------------------------------ Optimizer
def _hpams(root):
    return {"net_hyperparams": {"shape_blocks": 3, "texture_blocks": 1, "W": 256, "num_xyz_freq": 10,
                                "num_dir_freq": 4, "latent_dim": 256},
            "data": {"cat": "srn_cars", "splits": "cars_train", "data_dir": root, "n_train_views": 4,
                     "n_test_views": 3},
            "N_samples": 16, "N_importance": 8, "near": 0.8, "far": 1.8, "loss_reg_coef": 1e-4,
            "lr_schedule": [{"type": "step", "lr": 1e-4, "interval": 3}, {"type": "step", "lr": 1e-3, "interval": 3}],
            "check_points": 1000, "precision": "fp32"}


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A synthetic SRN set (32 x 32; three test views, two of them targets: one
    evaluation view), trained once with the fine pass."""
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.trainer import Trainer
    base = tmp_path_factory.mktemp("device_metrics")
    root, exps = str(base / "data"), str(base / "exps")
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=2, n_views=4, H=32, W=32, focal=32.8, seed=3)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    Trainer("t", 0, hpams=_hpams(root), batch_size=512, check_iter=0, exp_root=exps).training(0, 2, 1)
    return root, exps


@pytest.mark.parametrize("n_importance", [0, 8], ids=["coarse", "fine"])
def test_optimizer_with_device_metrics(trained, n_importance):
    from codenerf_amd.optimizer import Optimizer
    root, exps = trained
    runs = []
    for flag in (False, True):
        torch.manual_seed(0)
        opt = Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root), batch_size=512, num_opts=3, exp_root=exps,
                        n_importance=n_importance, device_metrics=flag)
        assert opt.device_metrics is flag and opt.n_fine == n_importance
        opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False)
        runs.append((opt, torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu",
                                     weights_only=True)))
    (host, saved_h), (dev, saved_d) = runs
    assert torch.equal(host.optimized_shapecodes, dev.optimized_shapecodes)
    assert torch.equal(host.optimized_texturecodes, dev.optimized_texturecodes)
    assert set(saved_h) == set(saved_d) >= {"psnr_eval", "ssim_eval", "optimized_shapecodes"}
    assert list(saved_d["psnr_eval"]) == list(saved_h["psnr_eval"]) == [0]
    ps_h, ps_d = np.array(saved_h["psnr_eval"][0]), np.array(saved_d["psnr_eval"][0])
    ss_h, ss_d = np.array(saved_h["ssim_eval"][0]), np.array(saved_d["ssim_eval"][0])
    assert ps_h.shape == ps_d.shape == ss_h.shape == ss_d.shape == (1,)
    print(f"n_importance {n_importance}: psnr {ps_h} / {ps_d} dB, ssim max|d| {np.abs(ss_h - ss_d).max():.2e}")
    assert np.isfinite(ps_d).all() and np.abs(ps_h - ps_d).max() <= 1e-4
    assert np.abs(ss_h - ss_d).max() <= 1e-10
    assert isinstance(saved_d["psnr_eval"][0][0], float) and isinstance(saved_d["ssim_eval"][0][0], float)
