"""GPU: mesh extraction -- cn_mesh_count, cn_mesh_emit, mesh.marching_tets,
mesh.extract_mesh and the Optimizer's save_mesh.

The reference has no mesh extraction.  The kernels are compared, bit for bit,
with the numpy restatement of their definition in tests/mesh_util.py (itself
checked on analytic fields by test_mesh_restatement.py); extract_mesh with the
restatement applied to the density the engine returns for the same lattice and
with the same engine calls made directly.

Bars:
  * vflags, vcount, tcount, vertices, triangles: bit for bit; the canary rows
    after Nv and Nt untouched;
  * the sphere at 33^3: 7118 vertices, 14232 triangles, closed, chi = 2, volume
    over 4/3 pi 0.7^3 in (0.98, 1) (linear interpolation of a field that is
    concave along every edge puts the crossings inside the sphere); the torus
    at (33, 33, 17): 4872 vertices, 9744 triangles, chi = 0;
  * extract_mesh's vertices, triangles, normals and colours: bit for bit, on
    the fp32 and the bf16x3f plan; for fp32 the gradient behind the normals
    against the float64 replay at test_gpu_inputgrad.py's bar (err_gpu <=
    inputgrad_util.MARGIN err_emu);
  * mesh.ply of the Optimizer equals extract_mesh of the saved codes; PSNR,
    SSIM and the codes are bit-identical to the run with the flag off.
"""
import os

import numpy as np
import pytest
import torch

import inputgrad_util as IU
import mesh_util as U

pytestmark = pytest.mark.gpu

F = np.float32
CANARY = 3                      # rows after Nv / Nt that must stay untouched
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _gpu(field, iso, lo=(0.0, 0.0, 0.0), s=(1.0, 1.0, 1.0)):
    """count -> prefix sums -> emit into buffers with canary rows -> dict as mesh_util.marching_tets."""
    from codenerf_amd import engine as E
    f = _t(np.ascontiguousarray(field, dtype=F).reshape(-1))
    vflags, vcount, tcount = E.mesh_count(f, field.shape, iso)
    vsum, tsum = torch.cumsum(vcount, 0, dtype=torch.int32), torch.cumsum(tcount, 0, dtype=torch.int32)
    Nv, Nt = int(vsum[-1]), int(tsum[-1])
    vert = torch.full((Nv + CANARY, 3), -7.5, dtype=torch.float32, device=_dev())
    tri = torch.full((Nt + CANARY, 3), -7, dtype=torch.int32, device=_dev())
    E.mesh_emit(f, field.shape, iso, lo, s, vflags, vsum - vcount, tsum - tcount, Nv, Nt, vert=vert, tri=tri)
    torch.cuda.synchronize()
    assert bool((vert[Nv:] == -7.5).all()) and bool((tri[Nt:] == -7).all()), "canary rows written"
    return dict(vflags=vflags.cpu().numpy(), vcount=vcount.cpu().numpy(), tcount=tcount.cpu().numpy(),
                verts=vert[:Nv].cpu().numpy(), tris=tri[:Nt].cpu().numpy())


def _same(got, want, tag=""):
    for k in ("vflags", "vcount", "tcount", "tris"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)
    assert got["verts"].dtype == F and got["verts"].tobytes() == want["verts"].tobytes(), (tag, "verts")


def _check(field, iso, lo=(0.0, 0.0, 0.0), s=(1.0, 1.0, 1.0), tag=""):
    from codenerf_amd.mesh import marching_tets
    want = U.marching_tets(field, iso, lo, s)
    got = _gpu(field, iso, lo, s)
    _same(got, want, tag)
    v, t = marching_tets(_t(np.ascontiguousarray(field, dtype=F)), field.shape, iso, lo, s)
    assert v.dtype == torch.float32 and t.dtype == torch.int32
    assert tuple(v.shape) == want["verts"].shape and tuple(t.shape) == want["tris"].shape
    assert v.cpu().numpy().tobytes() == want["verts"].tobytes() and np.array_equal(t.cpu().numpy(), want["tris"])
    return want


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("inside,outside,iso", [(1.0, -1.0, 0.0), (0.0, -1.0, 0.0)], ids=["pm1", "exact_iso"])
def test_all_256_patterns_of_one_cube(inside, outside, iso):
    """Every inside / outside pattern of a (2, 2, 2) lattice; 'exact_iso': the inside values equal iso."""
    lo, s = (-0.25, 0.5, 1.0), (0.3, 0.7, 1.1)
    total = 0
    for pat in range(256):
        f = np.array([inside if (pat >> i) & 1 else outside for i in range(8)], dtype=F).reshape(2, 2, 2)
        want = U.marching_tets(f, iso, lo, s)
        _same(_gpu(f, iso, lo, s), want, pat)
        assert U.POP[pat] in (0, 8) or len(want["tris"]) > 0
        total += len(want["tris"])
    assert total > 0


@pytest.mark.parametrize("dims", [(2, 3, 65), (33, 2, 7), (5, 5, 5), (7, 9, 12)], ids=lambda d: "x".join(map(str, d)))
def test_random_lattices(dims):
    f = np.random.default_rng(sum(dims)).standard_normal(dims).astype(F)
    want = _check(f, 0.1, (-0.3, 0.2, -1.0), (0.11, 0.07, 0.013), dims)
    assert len(want["tris"]) > 100


def test_sphere_33():
    dims = (33, 33, 33)
    lo, s = U.lattice_geometry(dims)
    m = _check(U.sphere(dims), 0.0, lo, s, "sphere")
    nv, nt = len(m["verts"]), len(m["tris"])
    ratio = U.signed_volume(m["verts"], m["tris"]) / (4.0 / 3.0 * np.pi * 0.7 ** 3)
    print(f"sphere 33^3: {nv} vertices, {nt} triangles, volume ratio {ratio:.4f}")
    assert (nv, nt) == (7118, 14232)
    assert U.is_closed_oriented(m["tris"]) and U.euler(nv, m["tris"]) == 2
    assert 0.98 < ratio < 1.0


def test_torus_33_33_17():
    dims = (33, 33, 17)
    lo, s = U.lattice_geometry(dims)
    m = _check(U.torus(dims), 0.0, lo, s, "torus")
    nv, nt = len(m["verts"]), len(m["tris"])
    assert (nv, nt) == (4872, 9744)
    assert U.is_closed_oriented(m["tris"]) and U.euler(nv, m["tris"]) == 0


def test_rounded_random_field():
    m = _check(U.rounded_random(), 0.0, tag="rounded")
    assert (len(m["verts"]), len(m["tris"])) == (338, 676) and U.is_closed_oriented(m["tris"])


def test_nan_inf_and_values_equal_to_iso():
    f = np.random.default_rng(5).standard_normal((6, 5, 7)).astype(F)
    f[1, 1, 1], f[5, 4, 6], f[2, 3, 4], f[3, 3, 3] = np.nan, np.nan, np.inf, -np.inf
    f[4, 2, 2] = f[0, 0, 0] = f[2, 2, 2] = 0.25
    m = _check(f, 0.25, (-1.0, -1.0, -1.0), (0.4, 0.5, 0.3), "special")
    assert np.isfinite(m["verts"]).all() and len(m["tris"]) > 0


@pytest.mark.parametrize("value", [-1.0, 1.0], ids=["all_outside", "all_inside"])
def test_no_surface_skips_emit(value, monkeypatch):
    from codenerf_amd import engine as E
    from codenerf_amd.mesh import marching_tets
    f = np.full((3, 4, 5), value, dtype=F)
    vflags, vcount, tcount = E.mesh_count(_t(f.reshape(-1)), f.shape, 0.0)
    assert not bool(vflags.any()) and not bool(vcount.any()) and not bool(tcount.any())

    def no_emit(*a, **k):
        raise AssertionError("emit launched for an empty surface")

    monkeypatch.setattr(E, "mesh_emit", no_emit)
    v, t = marching_tets(_t(f), f.shape, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda


# ------------------------------------------------------------------ extract_mesh
def _model(plan):
    params = IU.net_params(3)
    return params, IU.model(params, 3, precision=plan)


def _direct(m, n, bound):
    """The same quantities through the engine, call by call: the density of
    the lattice, then at given vertices the gradient, the normals, the colours."""
    s, t, obj = IU.codes()
    eng = m.engine()
    params = m.param_list()
    eng.ensure_packed(params, bwd=True)
    blob, _ = eng.latent_fwd(params, _t(s[obj]), _t(t[obj]))
    lo = tuple(float(F(0.0) - F(bound)) for _ in range(3))
    sp = float(F(2.0 * bound / (n - 1)))
    ax = U.axis_positions(n, lo[0], sp)
    xyz = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    vd = torch.zeros(n ** 3, 3, device=_dev())
    vd[:, 2] = 1.0
    sig, _ = eng.mlp_fwd(blob, n ** 3, xyz=_t(xyz), viewdir=vd)
    field = sig[:n ** 3].cpu().numpy().reshape(n, n, n)

    def at(verts):
        M = verts.shape[0]
        x = _t(verts)
        v = torch.zeros(M, 3, device=_dev())
        v[:, 2] = 1.0
        act = eng.new_act(M)
        eng.mlp_fwd(blob, M, xyz=x, viewdir=v, act=act, codes=True)
        Mp = eng.pad(M)
        eng.mlp_bwd(blob, M, torch.ones(Mp, device=_dev()), torch.zeros(Mp, 3, device=_dev()), act, pose=True)
        dxyz, _, _, _ = eng.mlp_input_grad(act, M, xyz=x, viewdir=v)
        d = dxyz[:M]
        nrm = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt()
        nor = torch.where((nrm > 0)[:, None], -d / nrm[:, None], torch.zeros_like(d))
        view = torch.where((nor != 0).any(1, keepdim=True), -nor, v)
        _, rgb = eng.mlp_fwd(blob, M, xyz=x, viewdir=view.contiguous())
        return d.cpu().numpy(), nor.cpu().numpy(), rgb[:M].cpu().numpy()

    return field, lo, sp, at


@pytest.mark.parametrize("n", [33, 17])
@pytest.mark.parametrize("plan", ["fp32", "bf16x3f"])
def test_extract_mesh(plan, n):
    from codenerf_amd.mesh import extract_mesh
    params, m = _cached(("model", plan), lambda: _model(plan))
    s, t, obj = IU.codes()
    bound = 0.5
    field, lo, sp, at = _direct(m, n, bound)
    iso = float(np.median(field))
    want = U.marching_tets(field, iso, lo, (sp, sp, sp))
    nv, nt = len(want["verts"]), len(want["tris"])
    print(f"{plan} n {n}: iso {iso:.4g}, {nv} vertices, {nt} triangles")
    assert nv > n * n and nt > n * n
    mesh = extract_mesh(m, _t(s[obj]), _t(t[obj]), n=n, bound=bound, iso=iso)
    assert mesh.verts.cpu().numpy().tobytes() == want["verts"].tobytes()
    assert np.array_equal(mesh.tris.cpu().numpy(), want["tris"])
    d, nor, rgb = at(want["verts"])
    assert mesh.normals.cpu().numpy().tobytes() == nor.tobytes()
    assert mesh.colors.cpu().numpy().tobytes() == rgb.tobytes()
    length = np.linalg.norm(nor.astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0)) and (length > 0).mean() > 0.99
    assert np.isfinite(rgb).all()                 # the rgb head is linear: write_ply clips
    # without normals the colours are those of the fixed view direction; without colours there are none
    plain = extract_mesh(m, _t(s[obj]), _t(t[obj]), n=n, bound=bound, iso=iso, normals=False)
    assert plain.normals is None and plain.verts.cpu().numpy().tobytes() == want["verts"].tobytes()
    eng = m.engine()
    blob, _ = eng.latent_fwd(m.param_list(), _t(s[obj]), _t(t[obj]))
    v = torch.zeros(nv, 3, device=_dev())
    v[:, 2] = 1.0
    _, rgb0 = eng.mlp_fwd(blob, nv, xyz=_t(want["verts"]), viewdir=v)
    assert torch.equal(plain.colors, rgb0[:nv])
    assert extract_mesh(m, _t(s[obj]), _t(t[obj]), n=n, bound=bound, iso=iso, colors=False).colors is None
    if plan == "fp32" and n == 17:
        # the gradient behind the normals against the float64 replay, at test_gpu_inputgrad.py's bar
        xyz = want["verts"]
        vd = np.zeros_like(xyz)
        vd[:, 2] = 1.0
        dsig, drgb = np.ones(nv, F), np.zeros((nv, 3), F)
        exact = IU.oracle_sample_grads(params, 3, 1, xyz, vd, dsig, drgb, torch.float64, with_kink=True)
        emu = IU.oracle_sample_grads(params, 3, 1, xyz, vd, dsig, drgb, torch.float32, "fp32")
        ok = ~exact[2]
        assert ok.sum() >= 0.97 * nv
        e_gpu, e_emu = IU.rel_l2(d[ok], exact[0][ok]), IU.rel_l2(emu[0][ok], exact[0][ok])
        print(f"d_xyz at the vertices: err_gpu {e_gpu:.3e} err_emu {e_emu:.3e}")
        assert e_gpu <= IU.MARGIN * e_emu


def test_extract_mesh_in_several_chunks(monkeypatch):
    """The lattice, the normals and the colours evaluated 4096 points per
    launch (2, 3 and 3 launches at n = 17) give the bits of the single launches."""
    from codenerf_amd import mesh, occupancy
    _, m = _cached(("model", "fp32"), lambda: _model("fp32"))
    s, t, obj = IU.codes()
    field, _, _, _ = _direct(m, 17, 0.5)
    iso = float(np.median(field))
    one = mesh.extract_mesh(m, _t(s[obj]), _t(t[obj]), n=17, iso=iso)
    monkeypatch.setattr(occupancy, "CHUNK", 4096)
    monkeypatch.setattr(mesh, "CHUNK", 4096)
    assert 2 * 4096 < one.verts.shape[0] <= 3 * 4096 and 4096 < 17 ** 3
    many = mesh.extract_mesh(m, _t(s[obj]), _t(t[obj]), n=17, iso=iso)
    for a, b in zip(one, many):
        assert torch.equal(a, b)


def test_extract_mesh_needs_iso():
    from codenerf_amd.mesh import extract_mesh
    _, m = _cached(("model", "fp32"), lambda: _model("fp32"))
    s, t, obj = IU.codes()
    with pytest.raises(TypeError):
        extract_mesh(m, _t(s[obj]), _t(t[obj]), n=17)
    # a surface the field never reaches: empty tensors
    mesh = extract_mesh(m, _t(s[obj]), _t(t[obj]), n=17, iso=1e30)
    assert all(tuple(x.shape) == (0, 3) for x in mesh)


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
    """The synthetic SRN set of test_gpu_sparse.py, trained once."""
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.trainer import Trainer
    base = tmp_path_factory.mktemp("mesh_opt")
    root, exps = str(base / "data"), str(base / "exps")
    make_synthetic_srn(root, "srn_cars", "cars_train", n_obj=2, n_views=4, H=32, W=32, focal=32.8, seed=3)
    make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    Trainer("t", 0, hpams=_hpams(root, N_importance=0), batch_size=512, check_iter=0, exp_root=exps).training(0, 2, 1)
    return root, exps


def test_optimizer_save_mesh(trained):
    from codenerf_amd.mesh import colors_to_uint8, extract_mesh, read_ply
    from codenerf_amd.optimizer import Optimizer
    root, exps = trained

    def run(**kw):
        torch.manual_seed(0)
        opt = Optimizer("t", 0, [0, 1], "test", hpams=_hpams(root, N_importance=0), batch_size=512, num_opts=3,
                        exp_root=exps, **kw)
        opt.optimize_objs([0, 1], lr=1e-2, lr_half_interval=2, save_img=False)
        return opt, torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu", weights_only=True)

    off, out_off = run()
    obj = str(off.ids[0])
    assert not os.path.exists(os.path.join(off.save_dir, obj, "mesh.ply")) and off.mesh_counts == {}
    # a density the optimised object's field crosses: the median over the lattice
    sc, tc = out_off["optimized_shapecodes"][0], out_off["optimized_texturecodes"][0]
    probe = extract_mesh(off.model, sc, tc, n=33, bound=0.5, iso=1e30)
    assert probe.verts.shape[0] == 0
    from codenerf_amd.mesh import lattice_geometry, lattice_points
    from codenerf_amd.occupancy import eval_density
    eng = off.model.engine()
    blob, _ = eng.latent_fwd(off.model.param_list(), sc.to(_dev()), tc.to(_dev()))
    lo, sp = lattice_geometry(33, 0.5)
    iso = float(eval_density(eng, blob, 33 ** 3, lambda a, b: lattice_points(33, lo, sp, a, b, _dev())).median())

    on, out_on = run(save_mesh=True, mesh_grid=33, mesh_iso=iso)
    assert set(out_on) == set(out_off)
    for key in ("optimized_shapecodes", "optimized_texturecodes"):
        assert torch.equal(out_on[key], out_off[key])
    for key in ("psnr_eval", "ssim_eval"):
        assert out_on[key] == out_off[key] and len(out_on[key][0]) == 1
    path = os.path.join(on.save_dir, obj, "mesh.ply")
    assert os.path.exists(path)
    v, t, nrm, col = read_ply(path)
    want = extract_mesh(on.model, out_on["optimized_shapecodes"][0], out_on["optimized_texturecodes"][0], n=33,
                        bound=(1.8 - 0.8) / 2, iso=iso)
    print(f"mesh.ply: iso {iso:.4g}, {len(v)} vertices, {len(t)} triangles")
    assert len(v) > 0 and on.mesh_counts == {0: (len(v), len(t))}
    assert v.tobytes() == want.verts.cpu().numpy().tobytes() and np.array_equal(t, want.tris.cpu().numpy())
    assert nrm.tobytes() == want.normals.cpu().numpy().tobytes()
    assert np.array_equal(col, colors_to_uint8(want.colors.cpu().numpy()))
