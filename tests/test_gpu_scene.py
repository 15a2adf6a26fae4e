"""GPU: several objects in one scene -- cn_scene_rays, cn_scene_combine,
cn_scene_composite, ImageStep.render_scene, compose.py.

Yardsticks:
  * cn_scene_rays, cn_scene_combine: the float32 numpy restatement of
    tests/scene_util.py, bit for bit (any NaN standing for any NaN);
  * cn_scene_composite: rgb / depth / acc are cn_composite_fwd's (acc = the sum
    of its weights output) and cn_composite_fine_fwd's on the combined planes,
    bit for bit, with or without the labels;
  * coarse obj_acc: sum w f restated in numpy from the device's own weights
    (float32 f, float32 products, float64 sum), max |d| <= 2^-23, by the
    argument of tests/test_gpu_aov.py: a float64 sum of at most 256 terms is
    good to 3e-14 of sum |w f| <= 1, so the two differ only by the final
    float32 rounding of a value of at most 1;
  * merged obj_acc: against the float64 restatement, e <= 2 max(e_rgb, 2^-23),
    e_rgb the error of cn_composite_fine_fwd's rgb (black background) against
    the same restatement on the same inputs: the shares lie in [0, 1] as the
    colours do, and the factor 2 covers the division per share;
  * instance: the restatement's on every ray it decides (scene_util.labels; at
    most 2 % of a shape's rays may be undecided);
  * |sum_k obj_acc - acc| <= K 2^-23;
  * render_scene with one object, identity, s = 1: the same launches made by
    hand through engine.*, bit for bit; against the dense definition rtol 1e-4,
    atol 1e-6 (tests/test_gpu_sparse.py's bar: the same plan on the same points);
  * render_scene with three objects against the oracle (ref_cpu's forward on the
    restated object rays, culled by the restated keep mask, combined in float64
    and composited by ref_cpu): rtol 1e-4 and atol K x 1e-6 on rgb and depth,
    the project's fp32 forward bar with its absolute part scaled by K because
    the scene's density is a sum of K terms, each within that bar.
"""
import json
import os

import numpy as np
import pytest
import torch

import inputgrad_util as IU
import occupancy_util as U
import scene_util as S
from golden_util import case_params, load
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -23
G, BOUND = 32, 0.5
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(_dev())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ cn_scene_rays
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("R", [1, 5, 257])
def test_scene_rays(R, K):
    from codenerf_amd.engine import scene_rays
    rng = np.random.default_rng(100 * R + K)
    ro = rng.uniform(-2, 2, (R, 3)).astype(F)
    rd = rng.standard_normal((R, 3)).astype(F)
    rows = np.stack([S.transform_row(S.random_rotation(rng), rng.uniform(-0.3, 0.3, 3), rng.uniform(0.5, 2.0))
                     for _ in range(K)])
    o, d = scene_rays(_t(ro), _t(rd), rows.tolist())
    want_o, want_d = S.scene_rays(ro, rd, rows)
    assert o.shape == d.shape == (K, R, 3)
    assert S.same_bits(o.cpu().numpy(), want_o) and S.same_bits(d.cpu().numpy(), want_d)


def test_scene_rays_identity():
    from codenerf_amd.engine import scene_rays
    ro, rd = U.rays(16)
    o, d = scene_rays(_t(ro), _t(rd), [S.transform_row(np.eye(3), np.zeros(3), 1.0).tolist()])
    o, d = o[0].cpu().numpy(), d[0].cpu().numpy()
    assert np.array_equal(o, ro) and np.array_equal(d, rd)          # up to the sign of a zero
    nz = (ro != 0) & (rd != 0)
    assert S.same_bits(o[nz], ro[nz]) and S.same_bits(d[nz], rd[nz])


# ------------------------------------------------------------------ cn_scene_combine
@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("M", [1, 255, 256, 257, 257 * 65])
def test_scene_combine(M, K):
    from codenerf_amd.engine import scene_combine
    rng = np.random.default_rng(10 * M + K)
    sig = (rng.uniform(0, 6, (K, M)) * (rng.uniform(0, 1, (K, M)) < 0.6)).astype(F)    # 40 % zeros per object
    rgb = rng.uniform(-1, 1, (K, M, 3)).astype(F)
    if M > 1:
        sig[:, M // 2] = 0                       # a sample nobody occupies
        sig[K - 1, M // 3] = np.nan              # a NaN density: NaN sigma, 0 colour
    inv_s = list(S.INV_S[:K])
    s, c = scene_combine(_t(sig), _t(rgb), inv_s)
    want_s, want_c = S.combine(sig, rgb, inv_s)
    s, c = s.cpu().numpy(), c.cpu().numpy()
    assert s.shape == (M,) and c.shape == (M, 3)
    assert S.same_bits(s, want_s) and S.same_bits(c, want_c)
    if M > 1:
        assert s[M // 2] == 0 and not c[M // 2].any() and np.isnan(s[M // 3]) and not c[M // 3].any()
    if K == 1:                                   # s = 1: the identity wherever sigma > 0
        pos = sig[0] > 0
        assert S.same_bits(s[pos], sig[0][pos]) and S.same_bits(c[pos], rgb[0][pos])


# ------------------------------------------------------------------ cn_scene_composite
def _case(Nc, Nf, per_ray_z, K):
    d = S.inputs(Nc, Nf, per_ray_z, K)
    ref = {wb: S.restate_inputs(d, wb) for wb in (False, True)}
    und = ref[False]["undecided"]
    print(f"({Nc}, {Nf}) per-ray z {per_ray_z} K {K}: {int(und.sum())} of {S.R_MAX} rays undecided")
    assert und.sum() <= S.MAX_UNDECIDED * S.R_MAX
    return d, ref


def _row_sets(R):
    """One ray per launch cannot hold the special rays at once: each goes alone."""
    return [slice(k, k + 1) for k in range(4)] if R == 1 else [slice(0, R)]


def _launch(d, rows, Nc, Nf, per_ray_z, white_bg, labels=True):
    from codenerf_amd.engine import scene_composite
    n = rows.stop - rows.start
    t = lambda x: _t(x[rows])
    tk = lambda x: _t(x[:, rows].reshape(x.shape[0], -1))
    z_c = t(d["zc"]) if per_ray_z else _t(d["zc"])
    args = {}
    if Nf:
        args.update(sigma_f=t(d["sf"]), rgb_f=t(d["rf"]), z_f=t(d["zf"]), Nf=Nf, obj_f=tk(d["of"]) if labels else None)
    out = scene_composite(t(d["sc"]), t(d["rc"]), z_c, Nc, n, d["inv_s"], white_bg,
                          obj_c=tk(d["oc"]) if labels else None, labels=labels, **args)
    return out, (t(d["sc"]), t(d["rc"]), z_c)


@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("per_ray_z", [False, True])
@pytest.mark.parametrize("Nc,Nf", S.SHAPES)
def test_scene_composite(Nc, Nf, per_ray_z, K):
    from codenerf_amd.engine import composite_fine_fwd, composite_fwd
    d, ref = _case(Nc, Nf, per_ray_z, K)
    dv = _dev()
    for R in (1, 5, 257):
        for white_bg in (True, False):
            r = ref[white_bg]
            for rows in _row_sets(R):
                n = rows.stop - rows.start
                out, (sc, rc, z_c) = _launch(d, rows, Nc, Nf, per_ray_z, white_bg)
                t = lambda x: _t(x[rows])
                # ---- rgb, depth, acc: the existing kernels' bits on the combined planes
                if Nf:
                    fine = (sc, rc, z_c, Nc, t(d["sf"]), t(d["rf"]), t(d["zf"]), Nf, n)
                    rgb, depth, acc = composite_fine_fwd(*fine, white_bg=white_bg, acc=True)
                else:
                    w = torch.empty(n, Nc, dtype=torch.float32, device=dv)
                    rgb, depth = composite_fwd(sc, rc, z_c, n, Nc, white_bg, weights=w)
                    acc = w.double().sum(-1).float()
                torch.cuda.synchronize()
                assert _bits(out["rgb"], rgb) and _bits(out["depth"], depth) and _bits(out["acc"], acc)
                # ---- the same without the labels
                o2, _ = _launch(d, rows, Nc, Nf, per_ray_z, white_bg, labels=False)
                assert o2["obj_acc"] is None and o2["instance"] is None
                assert all(_bits(o2[k], out[k]) for k in ("rgb", "depth", "acc"))
                # ---- obj_acc
                oa = out["obj_acc"].cpu().numpy().astype(np.float64)
                assert out["obj_acc"].shape == (n, K) and out["instance"].dtype == torch.int32
                if Nf:
                    rgb0 = composite_fine_fwd(*fine, white_bg=False)[0].cpu().numpy().astype(np.float64)
                    e_rgb = np.abs(rgb0 - ref[False]["rgb"][rows]).max()
                    e_oa = np.abs(oa - r["obj_acc"][rows]).max()
                    print(f"R {R} ({Nc}, {Nf}) K {K} rows {rows.start}: e_obj_acc {e_oa:.3e} e_rgb {e_rgb:.3e}")
                    assert e_oa <= 2 * max(e_rgb, EPS)
                else:
                    want = S.obj_acc_from_weights(w.cpu().numpy(), d["sc"][rows], d["oc"][:, rows], d["inv_s"])
                    e_oa = np.abs(oa - want).max()
                    print(f"R {R} N {Nc} K {K} rows {rows.start}: obj_acc max|d| {e_oa:.3e} against the device's weights")
                    assert e_oa <= EPS
                e_sum = np.abs(oa.sum(-1) - out["acc"].cpu().numpy().astype(np.float64)).max()
                assert e_sum <= K * EPS, e_sum
                # ---- instance: the restatement's on every ray it decides
                ok = ~r["undecided"][rows]
                inst = out["instance"].cpu().numpy()
                assert np.array_equal(inst[ok], r["instance"][rows][ok])
                # the special rays
                for k in range(rows.start, min(rows.stop, 3 + K)):
                    i = k - rows.start
                    if k == 1:
                        assert out["acc"][i] == 0 and not oa[i].any() and inst[i] == -1
                    if k == 2:
                        assert out["acc"][i] > 0.99
                    if k >= 3:                   # object k - 3 alone
                        assert inst[i] == k - 3 and not np.delete(oa[i], k - 3).any()


def test_scene_composite_ties_and_threshold():
    """Two objects with the same planes tie: the lower index wins; acc_min decides the background."""
    from codenerf_amd.engine import scene_composite
    d = S.inputs(64, 0, False, 1)
    rows = slice(0, 64)
    n = 64
    oc = np.repeat(d["oc"][:, rows].reshape(1, -1), 2, 0)
    ck = np.repeat(d["rc"][rows].reshape(1, -1, 3), 2, 0)
    sc, rc = S.combine(oc, ck, [1.0, 1.0])
    out = scene_composite(_t(sc), _t(rc), _t(d["zc"]), 64, n, [1.0, 1.0], True, obj_c=_t(oc), acc_min=0.0)
    oa = out["obj_acc"].cpu().numpy()
    assert np.array_equal(oa[:, 0], oa[:, 1]) and not out["instance"].any()
    acc = out["acc"].cpu().numpy()
    hi = scene_composite(_t(sc), _t(rc), _t(d["zc"]), 64, n, [1.0, 1.0], True, obj_c=_t(oc), acc_min=2.0)
    assert (hi["instance"] == -1).all() and _bits(hi["obj_acc"], out["obj_acc"])
    mid = float(np.median(acc))
    at = scene_composite(_t(sc), _t(rc), _t(d["zc"]), 64, n, [1.0, 1.0], True, obj_c=_t(oc), acc_min=mid)
    assert np.array_equal(at["instance"].cpu().numpy(), np.where(acc >= F(mid), 0, -1))


# ------------------------------------------------------------------ render_scene
H, NC, NF = 16, 32, 16


def _model(precision):
    from codenerf_amd.model import CodeNeRF
    g = load("n64_16x16")
    m = CodeNeRF(3, 1, precision=precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in case_params(g).items()})
    return m.to(_dev()), g


def _grid(kind):
    from codenerf_amd.occupancy import OccupancyGrid
    if kind == "full":
        return OccupancyGrid.full(G, BOUND, device=_dev())
    return OccupancyGrid(_t(U.ball_bits(G, BOUND).view(np.int32)), G, (0, 0, 0), BOUND)


def _keep(grid, ro, rd, z):
    words = grid.bits.cpu().numpy().view(np.uint32)
    return U.keep_mask(ro, rd, z, words, grid.G, np.array(grid.lo, F), F(grid.inv_cell), False)


def _by_hand(m, s, t, grid, ro, rd, z, Nf):
    """One object through engine.*: mark (keep_last False) -> gather -> mlp_fwd -> scatter -> composite."""
    from codenerf_amd import engine as E
    eng = m.engine()
    params = m.param_list()
    eng.ensure_packed(params, bwd=False)
    blob, _ = eng.latent_fwd(params, s, t)
    R = ro.shape[0]

    def sparse(zz, N):
        keep, count = E.sparse_mark(ro, rd, zz, R, N, grid.bits, grid.G, grid.lo, grid.inv_cell, False)
        incl = torch.cumsum(count, 0, dtype=torch.int32)
        Mk = int(incl[-1])
        off = incl - count
        xyz, vd = E.sparse_gather(ro, rd, zz, R, N, keep, off, Mk)
        sk, ck = eng.mlp_fwd(blob, Mk, xyz=xyz, viewdir=vd)
        return E.sparse_scatter(keep, off, R, N, sk, ck)

    Nc = z.shape[-1]
    sig_c, rgb_c = sparse(z, Nc)
    if not Nf:
        w = torch.empty(R, Nc, dtype=torch.float32, device=_dev())
        c, dpt = E.composite_fwd(sig_c, rgb_c, z, R, Nc, True, weights=w)
        return c, dpt, w.double().sum(-1).float(), None
    zf = E.sample_pdf(sig_c, z, R, Nc, torch.full((R, Nf), 0.5, device=_dev()))
    sig_f, rgb_f = sparse(zf, Nf)
    return E.composite_fine_fwd(sig_c, rgb_c, z, Nc, sig_f, rgb_f, zf, Nf, R, True, acc=True) + (zf,)


def _dense(m, s, t, grid, ro, rd, z, zf):
    """The definition: the dense forward in ray mode, zeroed by the verified keep mask."""
    from codenerf_amd import engine as E
    eng = m.engine()
    params = m.param_list()
    eng.ensure_packed(params, bwd=False)
    blob, _ = eng.latent_fwd(params, s, t)
    R, Nc = ro.shape[0], z.shape[-1]
    ron, rdn = ro.cpu().numpy(), rd.cpu().numpy()

    def zeroed(zz, N, stride):
        sig, rgb = eng.mlp_fwd(blob, R * N, rays_o=ro, rays_d=rd, z=zz, z_stride=stride, n_samples=N)
        k = _t(_keep(grid, ron, rdn, zz.cpu().numpy()).reshape(-1).astype(F))
        return sig[:R * N] * k, rgb[:R * N] * k[:, None]

    sig_c, rgb_c = zeroed(z, Nc, 0)
    if zf is None:
        return E.composite_fwd(sig_c, rgb_c, z, R, Nc, True)
    Nf = zf.shape[-1]
    sig_f, rgb_f = zeroed(zf, Nf, Nf)
    return E.composite_fine_fwd(sig_c, rgb_c, z, Nc, sig_f, rgb_f, zf, Nf, R, True)


def _close(tag, got, want, atol=1e-6):
    a, b = got.cpu().numpy(), want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    print(f"  {tag}: max|d| {np.abs(a - b).max():.2e}")
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=atol)


@pytest.mark.parametrize("Nf", [0, NF])
@pytest.mark.parametrize("kind", ["ball", "full"])
@pytest.mark.parametrize("plan", ["fp32", "bf16x3f"])
def test_render_scene_one_object_is_the_sparse_render(plan, kind, Nf):
    from codenerf_amd.render import ImageStep
    from codenerf_amd.scene import Scene, SceneObject
    m, g = _cached(("model", plan), lambda: _model(plan))
    s, t = _t(g["shape_table"][1]), _t(g["texture_table"][1])
    ro, rd = (_t(a) for a in U.rays(H))
    z = _t(U.midpoints(NC))
    grid = _grid(kind)
    R = H * H
    step = ImageStep(m)
    scene = Scene([SceneObject(s, t, grid)])
    out = step.render_scene(ro, rd, z, scene, n_fine=Nf)
    c, dpt, acc, zf = _by_hand(m, s, t, grid, ro, rd, z, Nf)
    assert _bits(out["rgb"], c) and _bits(out["depth"], dpt) and _bits(out["acc"], acc)
    assert out["obj_acc"].shape == (R, 1) and out["instance"].shape == (R,)
    assert set(out["instance"].cpu().numpy().tolist()) <= {-1, 0}
    if Nf:
        assert _bits(step.last_z_f, zf)
    # the kept counts, restated
    kc = int(_keep(grid, ro.cpu().numpy(), rd.cpu().numpy(), z.cpu().numpy()).sum())
    kf = int(_keep(grid, ro.cpu().numpy(), rd.cpu().numpy(), zf.cpu().numpy()).sum()) if Nf else 0
    assert step.last_sparse == (kc, kf, R * (NC + Nf)) and 0 < kc < R * NC
    # the dense definition
    cd, dd = _dense(m, s, t, grid, ro, rd, z, zf)
    _close(f"{plan} {kind} Nf {Nf} rgb", out["rgb"], cd)
    _close(f"{plan} {kind} Nf {Nf} depth", out["depth"], dd)
    # without the labels: the same bits
    o2 = step.render_scene(ro, rd, z, scene, n_fine=Nf, labels=False)
    assert o2["obj_acc"] is None and o2["instance"] is None
    assert all(_bits(o2[k], out[k]) for k in ("rgb", "depth", "acc"))


def _three_objects(g, dev=True):
    from codenerf_amd.scene import rotation_zyx
    st, tt = g["shape_table"], g["texture_table"]
    spec = [(0, 0, rotation_zyx(30, 20, -15), (0.25, -0.1, 0.05), 0.75, "ball"),
            (1, 1, rotation_zyx(-70, 10, 40), (-0.3, 0.2, -0.1), 1.0, "full"),
            (0, 1, rotation_zyx(115, -25, 5), (0.05, 0.3, 0.2), 1.5, "ball")]
    return [(st[i], tt[j], rot, np.array(tr), sc, kind) for i, j, rot, tr, sc, kind in spec]


@pytest.mark.parametrize("Nf", [0, NF])
def test_render_scene_three_objects_against_the_oracle(Nf):
    from codenerf_amd.render import ImageStep
    from codenerf_amd.scene import Scene, SceneObject
    m, g = _cached(("model", "fp32"), lambda: _model("fp32"))
    objs = _three_objects(g)
    K = len(objs)
    grids = [_grid(o[5]) for o in objs]
    scene = Scene([SceneObject(_t(o[0]), _t(o[1]), gr, o[2], o[3], o[4]) for o, gr in zip(objs, grids)])
    ro, rd = U.rays(H)
    z = U.midpoints(NC)
    R = H * H
    step = ImageStep(m)
    out = step.render_scene(_t(ro), _t(rd), _t(z), scene, n_fine=Nf)
    zf = step.last_z_f.cpu().numpy() if Nf else None
    # ---- the oracle: per object, ref_cpu's forward on the restated object rays
    p = ref_cpu.param_tensors(case_params(g), requires_grad=False)
    rows = np.array(scene.transforms(), dtype=F)
    assert S.same_bits(rows, np.stack([S.transform_row(o[2], o[3], o[4]) for o in objs]))
    ok, dk = S.scene_rays(ro, rd, rows)

    def planes(zz):
        sig, rgb, kept = [], [], 0
        for k, o in enumerate(objs):
            zk = zz if rows[k, 12] == 1 else zz * rows[k, 12]
            x = torch.tensor(U.points(ok[k], dk[k], zk))
            vd = torch.tensor(dk[k])[:, None, :].expand_as(x)
            with torch.no_grad():
                sg, cl = ref_cpu.codenerf_forward(p, x, vd, torch.tensor(o[0]), torch.tensor(o[1]))
            keep = _keep(grids[k], ok[k], dk[k], zk)
            kept += int(keep.sum())
            sig.append(sg[..., 0].double().numpy() * keep * float(rows[k, 12]))
            rgb.append(cl.double().numpy() * keep[..., None])
        a = np.stack(sig)
        tot = a.sum(0)
        f = np.divide(a, tot, out=np.zeros_like(a), where=tot > 0)
        return tot, (f[..., None] * np.stack(rgb)).sum(0), f, kept

    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    sig, rgb, f, kept_c = planes(z)
    zz = t64(z).expand(R, -1)
    kept_f = 0
    if Nf:
        sig_f, rgb_f, f_f, kept_f = planes(zf)
        pairs = [(t64(sig), t64(sig_f)), (t64(rgb), t64(rgb_f))] + [(t64(f[k]), t64(f_f[k])) for k in range(K)]
        zz, sig, rgb, *f = ref_cpu.merge_samples(zz, t64(zf), *pairs)
        f = np.stack([x.numpy() for x in f])
    want_rgb, want_depth = ref_cpu.volume_rendering(t64(sig), t64(rgb), zz, white_bg=True)
    w = ref_cpu.composite_weights(t64(sig), zz).numpy()
    obj_acc = np.stack([(w * f[k]).sum(-1) for k in range(K)], -1)
    inst, und = S.labels(obj_acc, w.sum(-1))
    print(f"three objects Nf {Nf}: kept {kept_c} + {kept_f} of {K * R * (NC + Nf)}, {int(und.sum())} pixels undecided, "
          f"labels {sorted(set(inst.tolist()))}")
    assert step.last_sparse == (kept_c, kept_f, K * R * (NC + Nf))
    _close("rgb", out["rgb"], want_rgb.numpy(), atol=K * 1e-6)
    _close("depth", out["depth"], want_depth.numpy(), atol=K * 1e-6)
    _close("acc", out["acc"], w.sum(-1), atol=K * 1e-6)
    assert und.sum() <= S.MAX_UNDECIDED * R
    assert np.array_equal(out["instance"].cpu().numpy()[~und], inst[~und])
    assert len(set(inst[~und].tolist()) - {-1}) >= 2         # the objects do occlude and share the picture
    np.testing.assert_allclose(out["obj_acc"].cpu().numpy(), obj_acc, rtol=1e-4, atol=K * 1e-6)


@pytest.mark.parametrize("Nf", [0, NF])
def test_an_object_no_ray_meets_changes_nothing(Nf):
    from codenerf_amd.render import ImageStep
    from codenerf_amd.scene import Scene, SceneObject, rotation_zyx
    m, g = _cached(("model", "fp32"), lambda: _model("fp32"))
    o = _three_objects(g)
    a = SceneObject(_t(o[0][0]), _t(o[0][1]), _grid("ball"), o[0][2], o[0][3], o[0][4])
    b = SceneObject(_t(o[1][0]), _t(o[1][1]), _grid("full"), o[1][2], o[1][3], o[1][4])
    far = SceneObject(_t(o[2][0]), _t(o[2][1]), _grid("full"), rotation_zyx(10, 20, 30), (6.0, -6.0, 6.0), 1.5)
    ro, rd, z = _t(U.rays(H)[0]), _t(U.rays(H)[1]), _t(U.midpoints(NC))
    step = ImageStep(m)
    two = step.render_scene(ro, rd, z, Scene([a, b]), n_fine=Nf)
    kept = step.last_sparse
    three = step.render_scene(ro, rd, z, Scene([a, b, far]), n_fine=Nf)
    assert step.last_sparse[:2] == kept[:2]
    assert all(_bits(two[k], three[k]) for k in ("rgb", "depth", "acc"))
    assert not three["obj_acc"][:, 2].any() and _bits(three["obj_acc"][:, :2], two["obj_acc"])
    assert torch.equal(two["instance"], three["instance"])


# ------------------------------------------------------------------ compose.py
def test_compose_py(tmp_path):
    import compose
    from oracle.params import make_codes
    from PIL import Image
    params = IU.net_params(3, sigma_shift=2.0)
    s, t = make_codes(5, 3)
    run = tmp_path / "exps" / "run"
    run.mkdir(parents=True)
    torch.save({"model_params": {k: torch.tensor(v) for k, v in params.items()},
                "shape_code_params": {"weight": torch.tensor(s)}, "texture_code_params": {"weight": torch.tensor(t)}},
               run / "models.pth")
    hp = {"net_hyperparams": dict(shape_blocks=3, texture_blocks=1, W=256, num_xyz_freq=10, num_dir_freq=4,
                                  latent_dim=256),
          "near": 0.8, "far": 1.8, "N_samples": 32, "N_importance": 8, "precision": "fp32"}
    (tmp_path / "hp.json").write_text(json.dumps(hp))
    desc = {"objects": [dict(shape=0, texture=1, translation=[0.25, 0.0, 0.0], rotation_deg=[30, 0, 0], scale=0.75,
                             bound=0.4, occ_grid=32, occ_tau=0.0, occ_dilate=0),
                        dict(shape=[1, 2, 0.5], texture=2, translation=[-0.25, 0.1, 0.0], rotation_deg=[-40, 10, 0],
                             scale=1.0, bound=0.4, occ_grid=32, occ_tau=0.0)]}
    (tmp_path / "scene.json").write_text(json.dumps(desc))
    out = tmp_path / "out"
    meta = compose.main(["--saved_dir", "run", "--jsonfile", str(tmp_path / "hp.json"), "--scene",
                         str(tmp_path / "scene.json"), "--frames", "2", "--azimuth", "0", "180", "--size", "16",
                         "--focal", "20", "--out", str(out)], exp_root=str(tmp_path / "exps"))
    stems = ("rgb", "instance", "alpha", "depth")
    assert sorted(os.listdir(out)) == sorted([f"{st}_{k:03d}.png" for st in stems for k in range(2)]
                                             + ["scene_frames.json"])
    assert json.load(open(out / "scene_frames.json")) == meta
    assert meta["scene"] == desc and len(meta["grid_fraction"]) == 2 and len(meta["frames"]) == 2
    assert [f["azimuth"] for f in meta["frames"]] == [0.0, 90.0]
    assert meta["n_samples"] == 32 and meta["n_importance"] == 8 and meta["near"] < meta["far"]
    seen = set()
    for k in range(2):
        with Image.open(out / f"instance_{k:03d}.png") as im:
            a = np.asarray(im)
        assert a.shape == (16, 16) and a.dtype == np.uint8 and set(a.reshape(-1).tolist()) <= {0, 1, 2}
        seen |= set(a.reshape(-1).tolist())
        with Image.open(out / f"rgb_{k:03d}.png") as im:
            assert np.asarray(im).shape == (16, 16, 3)
    assert seen - {0}                                      # some pixel belongs to an object
