"""GPU: rendering through an occupancy grid -- cn_occupancy_build, cn_sparse_mark,
cn_sparse_gather, cn_sparse_scatter, ImageStep.render / render_fine with a grid,
OccupancyGrid.build and the Optimizer's sparse evaluation.

The reference has no occupancy grid.  The kernels are compared, exactly, with
the numpy restatement of their definition in tests/occupancy_util.py; the
renders with the definition itself: the dense render of the same plan in which
the density and colour of every culled sample are 0 (the dense MLP forward in
ray mode, zeroed with the already verified keep mask, through the existing
compositing entries).

Bars:
  * grid words, keep words, counts, gathered points and view directions,
    scattered values: bit for bit;
  * render / render_fine with a grid against the definition, and an all-ones
    grid against the dense render: rtol 1e-4, atol 1e-6 on rgb and depth (the
    fp32 forward bar of test_gpu_fine_opt.py) for the fp32 and the bf16x3f plan
    alike -- both sides run the same plan on bit-identical points;
  * the Optimizer's evaluation metrics with an all-ones grid against the run
    without: the same bar on PSNR and SSIM; the optimised codes bit for bit.

Scene (occupancy_util): 16 x 16 rays from look_at_pose(1.3, 35, 20), z the
stratified midpoints of [0.8, 1.8], a 32^3 grid over [-0.5, 0.5]^3 whose set
cells are those with their centre within 0.35 of (0.1, 0, -0.05): at N = 64,
12.0 % of the samples are kept (1970, not a multiple of 256) and 70.7 % of the
rays keep none.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import occupancy_util as U
from golden_util import case_params, load

pytestmark = pytest.mark.gpu

G, BOUND = 32, 0.5
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _words(w):
    """uint32 words -> the int32 tensor the wrappers take."""
    return _t(np.ascontiguousarray(w, dtype=np.uint32).view(np.int32))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ build
@pytest.mark.parametrize("dilate", [0, 1, 2, 4])
@pytest.mark.parametrize("Gb", [32, 64])
def test_occupancy_build_random(Gb, dilate):
    from codenerf_amd.engine import occupancy_build
    sigma = _cached(("sigma", Gb), lambda: np.random.default_rng(Gb).random(Gb ** 3, dtype=np.float32))
    tau = 0.999                               # ~0.1 % of the cells occupied before dilation
    bits = occupancy_build(_t(sigma), Gb, tau, dilate)
    ref = U.build_bits(sigma, Gb, tau, dilate)
    share = U.unpack_cells(ref, Gb).mean()
    print(f"G {Gb} dilate {dilate}: {share:.4f} of the cells set")
    assert 0 < share < 1
    assert np.array_equal(_u32(bits), ref)


@pytest.mark.parametrize("dilate", [0, 2, 4])
def test_occupancy_build_edges(dilate):
    from codenerf_amd.engine import occupancy_build
    f32 = np.float32
    corner = np.zeros((G, G, G), f32)
    corner[G - 1, 0, G - 1] = 1.0             # the clamp at three faces
    nan = np.zeros((G, G, G), f32)
    nan[7, 31, 0] = np.nan                    # NaN counts as occupied
    at_tau = np.zeros((G, G, G), f32)
    at_tau[10, 11, 12] = 0.5                  # sigma == tau is occupied
    at_tau[20, 20, 20] = np.nextafter(f32(0.5), f32(0))
    for name, s in (("corner", corner), ("nan", nan), ("at_tau", at_tau), ("empty", np.zeros((G, G, G), f32)),
                    ("full", np.ones((G, G, G), f32))):
        bits = _u32(occupancy_build(_t(s.reshape(-1)), G, 0.5, dilate))
        ref = U.build_bits(s.reshape(-1), G, 0.5, dilate)
        assert np.array_equal(bits, ref), name
        n = int(U.unpack_cells(bits, G).sum())
        side = dilate + 1
        want = {"corner": side ** 3, "nan": (2 * dilate + 1) * side * side, "empty": 0, "full": G ** 3,
                "at_tau": (2 * dilate + 1) ** 3}[name]
        assert n == want, (name, n, want)


# ------------------------------------------------------------------ mark
def _grid(kind):
    n = G ** 3 // 32
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "ones":
        return np.full(n, 0xFFFFFFFF, np.uint32)
    if kind == "ball":
        return U.ball_bits(G, BOUND)
    rng = np.random.default_rng(11)           # "random": about 30 % of the words set, to random bits
    w = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.where(rng.random(n) < 0.3, w, 0).astype(np.uint32)


def _shape(name):
    """-> (rays_o, rays_d, z): 'HxN' shared z, 'HxNp' per-ray z, '1xN' one ray."""
    def make():
        H, N = name.rstrip("p").split("x")
        H, N = int(H), int(N)
        ro, rd = U.rays(H)
        if H == 1:
            ro, rd = (a[100:101].copy() for a in U.rays(16))
        z = U.midpoints(N)
        if name.endswith("p"):
            shift = np.random.default_rng(5).random((ro.shape[0], 1), dtype=np.float32) * np.float32(0.01)
            z = (z[None, :] + shift).astype(np.float32)
            z[3, N // 2] = np.nan             # a NaN point is not kept
            z[4, :] = 9.0                     # a ray wholly outside the box
        return ro, rd, z
    return _cached(("shape", name), make)


LO, INV_CELL = U.grid_geometry(G, (0, 0, 0), BOUND)
MARK_SHAPES = ["16x64", "17x65", "16x256", "16x1", "1x64", "1x1", "17x65p", "16x64p"]


@pytest.mark.parametrize("keep_last", [0, 1])
@pytest.mark.parametrize("grid", ["zero", "ones", "random", "ball"])
@pytest.mark.parametrize("shape", MARK_SHAPES)
def test_sparse_mark(shape, grid, keep_last):
    from codenerf_amd.engine import sparse_mark
    ro, rd, z = _shape(shape)
    R, N = ro.shape[0], z.shape[-1]
    words = _cached(("grid", grid), lambda: _grid(grid))
    keep, count = sparse_mark(_t(ro), _t(rd), _t(z), R, N, _words(words), G, LO, INV_CELL, keep_last)
    ref = U.keep_mask(ro, rd, z, words, G, LO, INV_CELL, keep_last)
    ref_words, ref_count = U.pack_keep(ref)
    assert np.array_equal(_u32(keep), ref_words)
    assert np.array_equal(count.cpu().numpy(), ref_count)
    if grid == "zero":
        assert int(count.sum()) == (R if keep_last else 0)
    if grid == "ones" and not keep_last and not shape.endswith("p"):
        x = U.points(ro, rd, z).astype(np.float64)
        inside = (np.abs(x) < BOUND - 1e-4).all(-1)            # kept means inside the box
        outside = (np.abs(x) > BOUND + 1e-4).any(-1)
        assert ref[inside].all() and not ref[outside].any()
    if shape == "16x64" and grid == "ball" and not keep_last:
        share, empty = ref.mean(), (ref.sum(1) == 0).mean()
        print(f"scene: {share:.4f} of the samples kept ({ref.sum()}), {empty:.4f} of the rays keep none")
        assert 0.05 <= share <= 0.30 and 0 < empty < 1 and ref.sum() % 256


# ------------------------------------------------------------------ gather / scatter
def _marked(shape, grid, keep_last=1):
    from codenerf_amd.engine import sparse_mark
    ro, rd, z = _shape(shape)
    R, N = ro.shape[0], z.shape[-1]
    words = _cached(("grid", grid), lambda: _grid(grid))
    ref = U.keep_mask(ro, rd, z, words, G, LO, INV_CELL, keep_last)
    keep, count = sparse_mark(_t(ro), _t(rd), _t(z), R, N, _words(words), G, LO, INV_CELL, keep_last)
    incl = torch.cumsum(count, 0, dtype=torch.int32)
    assert np.array_equal(_u32(keep), U.pack_keep(ref)[0])
    return ro, rd, z, R, N, ref, keep, incl - count, int(incl[-1])


GS_CASES = [("16x64", "ball", 0), ("16x64", "ball", 1), ("17x65", "random", 1), ("17x65p", "ones", 1),
            ("16x256", "random", 0), ("1x1", "zero", 1), ("16x1", "zero", 1)]


@pytest.mark.parametrize("shape,grid,keep_last", GS_CASES)
def test_sparse_gather(shape, grid, keep_last):
    from codenerf_amd import _lib
    from codenerf_amd.engine import sparse_gather
    ro, rd, z, R, N, ref, keep, off, Mk = _marked(shape, grid, keep_last)
    assert Mk == ref.sum() and Mk > 0
    x = U.points(ro, rd, z)
    want_xyz = x[ref]                                           # ray-major, samples ascending
    want_vd = np.broadcast_to(rd[:, None, :], x.shape)[ref]
    xyz, vd = sparse_gather(_t(ro), _t(rd), _t(z), R, N, keep, off, Mk)
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), want_xyz.view(np.uint32))
    assert np.array_equal(vd.cpu().numpy().view(np.uint32), want_vd.view(np.uint32))
    # rows beyond Mk are not written
    L = _lib.lib()
    pad = 64
    bx = torch.full((Mk + pad, 3), -7.0, device=_dev())
    bv = torch.full((Mk + pad, 3), -7.0, device=_dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    tro, trd, tz = _t(ro), _t(rd), _t(z)
    rc = L.cn_sparse_gather(p(tro), p(trd), p(tz), 0 if z.ndim == 1 else N, R, N, p(keep), p(off), p(bx), p(bv),
                            _lib.stream_ptr(_dev()))
    assert rc == 0, L.cn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bx[:Mk], xyz) and torch.equal(bv[:Mk], vd)
    assert bool((bx[Mk:] == -7.0).all()) and bool((bv[Mk:] == -7.0).all())


@pytest.mark.parametrize("shape,grid,keep_last", GS_CASES)
def test_sparse_scatter(shape, grid, keep_last):
    from codenerf_amd.engine import sparse_scatter
    ro, rd, z, R, N, ref, keep, off, Mk = _marked(shape, grid, keep_last)
    rng = np.random.default_rng(3)
    sig_k = (rng.random(Mk, dtype=np.float32) + np.float32(0.5))
    rgb_k = (rng.random((Mk, 3), dtype=np.float32) + np.float32(0.5))
    sig = torch.full((R * N,), float("nan"), device=_dev())
    rgb = torch.full((R * N, 3), float("nan"), device=_dev())
    out = sparse_scatter(keep, off, R, N, _t(sig_k), _t(rgb_k), sigma=sig, rgb=rgb)
    assert out[0] is sig and out[1] is rgb
    want_s = np.zeros((R, N), np.float32)
    want_c = np.zeros((R, N, 3), np.float32)
    want_s[ref] = sig_k
    want_c[ref] = rgb_k
    assert np.array_equal(sig.cpu().numpy().view(np.uint32), want_s.reshape(-1).view(np.uint32))
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), want_c.reshape(-1, 3).view(np.uint32))


# ------------------------------------------------------------------ render
def _model(precision):
    from codenerf_amd.model import CodeNeRF
    g = load("n64_16x16")
    m = CodeNeRF(3, 1, precision=precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in case_params(g).items()})
    oi = int(g["obj_idx"])
    return m.to(_dev()), _t(g["shape_table"][oi]), _t(g["texture_table"][oi])


def _ball_grid():
    from codenerf_amd.occupancy import OccupancyGrid
    return OccupancyGrid(_words(_cached(("grid", "ball"), lambda: _grid("ball"))), G, (0, 0, 0), BOUND)


def _zeroed(sig, rgb, keep, n):
    k = _t(keep.reshape(-1))
    return sig[:n] * k, rgb[:n] * k[:, None]


def _expected(m, s, t, ro, rd, z, Nf, grid):
    """The definition: dense MLP forward in ray mode, culled samples zeroed,
    the existing compositing -> (rgb, depth, fine z or None, kept coarse, kept fine)."""
    from codenerf_amd import engine as E
    eng = m.engine()
    params = m.param_list()
    eng.ensure_packed(params, bwd=False)
    blob, _ = eng.latent_fwd(params, s, t)
    R, Nc = ro.shape[0], z.shape[-1]
    words = _u32(grid.bits)
    lo, ic = np.array(grid.lo, np.float32), np.float32(grid.inv_cell)
    tro, trd, tz = _t(ro), _t(rd), _t(z)
    sig, rgb = eng.mlp_fwd(blob, R * Nc, rays_o=tro, rays_d=trd, z=tz, z_stride=0, n_samples=Nc)
    kc = U.keep_mask(ro, rd, z, words, grid.G, lo, ic, True)
    sig_c, rgb_c = _zeroed(sig, rgb, kc.astype(np.float32), R * Nc)
    if not Nf:
        c, d = E.composite_fwd(sig_c, rgb_c, tz, R, Nc, True)
        return c, d, None, int(kc.sum()), 0
    zf = E.sample_pdf(sig_c, tz, R, Nc, torch.full((R, Nf), 0.5, device=_dev()))
    sig, rgb = eng.mlp_fwd(blob, R * Nf, rays_o=tro, rays_d=trd, z=zf, z_stride=Nf, n_samples=Nf)
    kf = U.keep_mask(ro, rd, zf.cpu().numpy(), words, grid.G, lo, ic, False)
    sig_f, rgb_f = _zeroed(sig, rgb, kf.astype(np.float32), R * Nf)
    c, d = E.composite_fine_fwd(sig_c, rgb_c, tz, Nc, sig_f, rgb_f, zf, Nf, R, True)
    return c, d, zf, int(kc.sum()), int(kf.sum())


def _close(tag, got, want):
    a, b = got.cpu().numpy(), want.cpu().numpy()
    print(f"  {tag}: max|d| {np.abs(a - b).max():.2e} bit-identical {np.array_equal(a, b)}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)


RENDER_SHAPES = [(16, 64, 64), (17, 64, 64), (16, 5, 3), (17, 5, 3)]


@pytest.mark.parametrize("H,Nc,Nf", RENDER_SHAPES)
@pytest.mark.parametrize("plan", ["fp32", "bf16x3f"])
def test_render_with_a_grid_is_the_definition(plan, H, Nc, Nf):
    from codenerf_amd.render import ImageStep
    m, s, t = _cached(("model", plan), lambda: _model(plan))
    ro, rd = U.rays(H)
    z = U.midpoints(Nc)
    grid = _ball_grid()
    R = H * H
    step = ImageStep(m)
    print(f"{plan} {H}x{H} Nc {Nc} Nf {Nf}")
    # coarse only
    c_ref, d_ref, _, kc, _ = _expected(m, s, t, ro, rd, z, 0, grid)
    c, d = step.render(_t(ro), _t(rd), _t(z), s, t, occupancy=grid)
    assert step.last_sparse == (kc, 0, R * Nc)
    _close("render rgb", c, c_ref)
    _close("render depth", d, d_ref)
    if Nc == 64:
        assert 0.05 <= (kc - R) / (R * Nc) <= 0.30            # without the always-kept last samples
    # coarse + fine: the expected path's fine z handed in, then its own sample_pdf
    c_ref, d_ref, zf, kc2, kf = _expected(m, s, t, ro, rd, z, Nf, grid)
    assert kc2 == kc
    c, d = step.render_fine(_t(ro), _t(rd), _t(z), Nf, s, t, z_f=zf, occupancy=grid)
    assert step.last_sparse == (kc, kf, R * (Nc + Nf))
    _close("render_fine(z_f=) rgb", c, c_ref)
    _close("render_fine(z_f=) depth", d, d_ref)
    c, d = step.render_fine(_t(ro), _t(rd), _t(z), Nf, s, t, occupancy=grid)
    _close("render_fine own z_f", step.last_z_f, zf)
    # its own fine z may differ in the last bits: the expected composite of ITS samples
    if not torch.equal(step.last_z_f, zf):
        zf2 = step.last_z_f
        words, lo, ic = _u32(grid.bits), np.array(grid.lo, np.float32), np.float32(grid.inv_cell)
        kf = int(U.keep_mask(ro, rd, zf2.cpu().numpy(), words, G, lo, ic, False).sum())
    assert step.last_sparse == (kc, kf, R * (Nc + Nf))
    _close("render_fine rgb", c, c_ref)
    _close("render_fine depth", d, d_ref)
    # the culled render is not the dense one: a grid that culls nothing could not pass for this one
    dense, _ = step.render(_t(ro), _t(rd), _t(z), s, t)
    assert not torch.equal(dense, step.render(_t(ro), _t(rd), _t(z), s, t, occupancy=grid)[0])


@pytest.mark.parametrize("H,Nc,Nf", [(16, 64, 64), (17, 5, 3)])
@pytest.mark.parametrize("plan", ["fp32", "bf16x3f"])
def test_an_all_ones_grid_is_the_dense_render(plan, H, Nc, Nf):
    from codenerf_amd.occupancy import OccupancyGrid
    from codenerf_amd.render import ImageStep
    m, s, t = _cached(("model", plan), lambda: _model(plan))
    ro, rd = (_t(a) for a in U.rays(H))
    z = _t(U.midpoints(Nc))
    grid = OccupancyGrid(_words(_grid("ones")), G, (0, 0, 0), 10.0)
    R = H * H
    step = ImageStep(m)
    print(f"{plan} {H}x{H} Nc {Nc} Nf {Nf}")
    c_ref, d_ref = step.render(ro, rd, z, s, t)
    assert step.last_sparse is None
    c, d = step.render(ro, rd, z, s, t, occupancy=grid)
    assert step.last_sparse == (R * Nc, 0, R * Nc)
    _close("render rgb", c, c_ref)
    _close("render depth", d, d_ref)
    c_ref, d_ref = step.render_fine(ro, rd, z, Nf, s, t)
    zf = step.last_z_f
    c, d = step.render_fine(ro, rd, z, Nf, s, t, z_f=zf, occupancy=grid)
    assert step.last_sparse == (R * Nc, R * Nf, R * (Nc + Nf))
    _close("render_fine rgb", c, c_ref)
    _close("render_fine depth", d, d_ref)


def test_nothing_kept_skips_the_mlp():
    """Fine samples of an all-zero grid: Mk = 0, no MLP launch, zeros."""
    from codenerf_amd.occupancy import OccupancyGrid
    from codenerf_amd.render import ImageStep
    m, s, t = _cached(("model", "fp32"), lambda: _model("fp32"))
    ro, rd = (_t(a) for a in U.rays(16))
    z = _t(U.midpoints(5))
    grid = OccupancyGrid(_words(_grid("zero")), G, (0, 0, 0), BOUND)
    step = ImageStep(m)
    c, d = step.render_fine(ro, rd, z, 3, s, t, occupancy=grid)
    assert step.last_sparse == (256, 0, 256 * 8)
    # only the last coarse sample of every ray is left, and it is opaque
    assert bool(torch.isfinite(c).all())
    np.testing.assert_allclose(d.cpu().numpy(), float(U.midpoints(5)[-1]), rtol=1e-6)


# ------------------------------------------------------------------ OccupancyGrid.build
def test_occupancy_grid_build():
    from codenerf_amd.occupancy import OccupancyGrid
    m, s, t = _cached(("model", "fp32"), lambda: _model("fp32"))

    def densities(Gs):
        xyz = OccupancyGrid.cell_centers(Gs, (0, 0, 0), BOUND, device=_dev())
        vd = torch.zeros_like(xyz)
        vd[:, 0] = 1.0
        with torch.no_grad():
            sig, _ = m(xyz, vd, s, t)
        return sig.reshape(-1).cpu().numpy()

    sig = densities(G)
    tau = float(np.median(sig))
    for dilate in (0, 1):
        grid = OccupancyGrid.build(m, s, G=G, bound=BOUND, tau=tau, dilate=dilate)
        ref = U.build_bits(sig, G, tau, dilate)
        assert np.array_equal(_u32(grid.bits), ref)
        assert grid.fraction() == U.unpack_cells(ref, G).mean()
    assert 0.3 < OccupancyGrid.build(m, s, G=G, bound=BOUND, tau=tau, dilate=0).fraction() < 0.7
    sig2 = densities(2 * G).reshape(G, 2, G, 2, G, 2).max(axis=(1, 3, 5)).reshape(-1)
    grid = OccupancyGrid.build(m, s, G=G, bound=BOUND, tau=tau, dilate=0, supersample=2)
    assert np.array_equal(_u32(grid.bits), U.build_bits(sig2, G, tau, 0))
    assert not np.array_equal(sig2, sig)
    grid = OccupancyGrid.build(m, s, G=G, bound=BOUND, tau=0.0, dilate=0)
    assert grid.fraction() == 1.0 and bool((grid.bits == -1).all())


# ------------------------------------------------------------------ Optimizer
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
    """The synthetic SRN set of test_gpu_fine_opt.py, trained once with the fine pass."""
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.trainer import Trainer
    base = tmp_path_factory.mktemp("sparse_opt")
    root, exps = str(base / "data"), str(base / "exps")
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=2, n_views=4, H=32, W=32, focal=32.8, seed=3)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    Trainer("t", 0, hpams=_hpams(root, N_importance=8), batch_size=512, check_iter=0, exp_root=exps).training(0, 2, 1)
    return root, exps


@pytest.mark.parametrize("device_metrics", [False, True], ids=["host_metrics", "device_metrics"])
@pytest.mark.parametrize("n_fine", [0, 8], ids=["coarse", "fine"])
def test_optimizer_sparse_eval_with_a_full_grid(trained, n_fine, device_metrics):
    from codenerf_amd.optimizer import Optimizer
    root, exps = trained
    runs = []
    for sparse in (False, True):
        torch.manual_seed(0)
        opt = Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root, N_importance=n_fine), batch_size=512, num_opts=3,
                        exp_root=exps, device_metrics=device_metrics, sparse_eval=sparse, occ_grid=32, occ_tau=0.0,
                        occ_bound=10.0)
        opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False)
        out = torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu", weights_only=True)
        assert set(out) == {"ids", "num_obj", "optimized_shapecodes", "optimized_texturecodes", "psnr_eval",
                            "ssim_eval"}
        runs.append((opt, out))
    (off, out_off), (on, out_on) = runs
    assert torch.equal(out_off["optimized_shapecodes"], out_on["optimized_shapecodes"])
    assert torch.equal(out_off["optimized_texturecodes"], out_on["optimized_texturecodes"])
    assert off.step_impl.last_sparse is None and off.occ_fraction == {}
    total = 32 * 32 * (16 + n_fine)
    assert on.step_impl.last_sparse == (32 * 32 * 16, 32 * 32 * n_fine, total)
    assert on.occ_fraction == {0: 1.0} and on.occ_kept == {0: 1.0}
    for key in ("psnr_eval", "ssim_eval"):
        a, b = np.array(out_on[key][0]), np.array(out_off[key][0])
        print(f"{key}: on {a} off {b} |d| {np.abs(a - b).max():.2e}")
        assert a.shape == (1,) and np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)
