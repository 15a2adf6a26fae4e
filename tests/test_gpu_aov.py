"""GPU: the geometry buffers -- cn_composite_aov, ImageStep.render_aov, render.py.

Yardsticks:
  * rgb / depth / acc: cn_composite_fwd's (acc = the sum of its weights output)
    and cn_composite_fine_fwd's, bit for bit; every output the same whichever
    optional pointers are NULL;
  * coarse normal: sum w u restated in numpy from the device's own weights
    (float32 u, float32 products, float64 sum), max |d| <= 2^-23: a float64
    sum of at most 256 terms is good to 3e-14 of sum |w u| <= 1, so the two
    differ only by the final float32 rounding of a value of at most 1;
  * merged normal: against the float64 restatement (aov_util.restate), with a
    measured bar: e_normal <= 2 max(e_rgb, 2^-23), e_rgb the error of
    cn_composite_fine_fwd's rgb (black background, |rgb| <= 1) against the same
    restatement on the same inputs -- the same weighted sum of bounded vectors;
    the factor 2 covers the square root and the division per u;
  * depth_med: the restatement's z_m bit for bit on every ray it decides (no
    C_k within 1e-5 of 0.5; at most 2 % of a shape's rays may be undecided);
  * render_aov: rgb and depth are render's / render_fine's bit for bit; the
    normal image within inputgrad_util.MARGIN x err_emu of the float64 autograd
    of ref_cpu.codenerf_forward composited in float64 (rel-L2 over the image).
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import aov_util as A
import inputgrad_util as U
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ kernel
COARSE = [(n, 0) for n in (2, 5, 64, 65, 256)]
MERGED = [(5, 3), (64, 64), (96, 160)]


def _case(Nc, Nf, per_ray_z):
    def make():
        d = A.inputs(Nc, Nf, per_ray_z)
        ref = {wb: A.restate_inputs(d, wb) for wb in (False, True)}
        bad = A.undecided(ref[False]["C"])
        print(f"({Nc}, {Nf}) per-ray z {per_ray_z}: {int(bad.sum())} of {A.R_MAX} rays undecided for depth_med")
        assert bad.sum() <= 0.02 * A.R_MAX
        return d, ref, bad
    return _cached(("case", Nc, Nf, per_ray_z), make)


def _row_sets(R):
    """One ray per launch cannot hold the four special rays at once: each goes alone."""
    return [slice(k, k + 1) for k in range(4)] if R == 1 else [slice(0, R)]


def _launch(d, rows, Nc, Nf, per_ray_z, white_bg, **kw):
    """engine.composite_aov on the rows of the inputs; kw: normals, acc, depth_median."""
    from codenerf_amd.engine import composite_aov
    dv = _dev()
    n = rows.stop - rows.start
    t = lambda x: x[rows].contiguous().to(dv)
    z_c = t(d["zc"]) if per_ray_z else d["zc"].to(dv)
    normals = kw.pop("normals", True)
    args = dict(kw)
    if Nf:
        args.update(sigma_f=t(d["sf"]), rgb_f=t(d["rf"]), z_f=t(d["zf"]), Nf=Nf)
    if normals:
        args.update(grad_c=t(d["gc"]).reshape(-1, 3))
        if Nf:
            args.update(grad_f=t(d["gf"]).reshape(-1, 3))
    out = composite_aov(t(d["sc"]), t(d["rc"]), z_c, Nc, n, white_bg, **args)
    return out, (t(d["sc"]), t(d["rc"]), z_c)


@pytest.mark.parametrize("white_bg", [True, False])
@pytest.mark.parametrize("per_ray_z", [False, True])
@pytest.mark.parametrize("Nc,Nf", COARSE + MERGED)
@pytest.mark.parametrize("R", [1, 5, 257])
def test_composite_aov(R, Nc, Nf, per_ray_z, white_bg):
    from codenerf_amd.engine import composite_fine_fwd, composite_fwd
    d, ref, bad = _case(Nc, Nf, per_ray_z)
    r = ref[white_bg]
    dv = _dev()
    for rows in _row_sets(R):
        n = rows.stop - rows.start
        out, (sc, rc, z_c) = _launch(d, rows, Nc, Nf, per_ray_z, white_bg)
        t = lambda x: x[rows].contiguous().to(dv)
        # ---- rgb, depth, acc: the existing kernels' bits
        if Nf:
            fine = (sc, rc, z_c, Nc, t(d["sf"]), t(d["rf"]), t(d["zf"]), Nf, n)
            rgb, depth, acc = composite_fine_fwd(*fine, white_bg=white_bg, acc=True)
        else:
            w = torch.empty(n, Nc, dtype=torch.float32, device=dv)
            rgb, depth = composite_fwd(sc, rc, z_c, n, Nc, white_bg, weights=w)
            acc = w.double().sum(-1).float()
        torch.cuda.synchronize()
        assert _bits(out["rgb"], rgb) and _bits(out["depth"], depth)
        assert _bits(out["acc"], acc)          # coarse: both are the float64 sum of the weights, rounded once
        # ---- the same whichever optional pointers are NULL
        for kw in (dict(normals=False), dict(acc=False), dict(depth_median=False),
                   dict(normals=False, acc=False, depth_median=False)):
            o2, _ = _launch(d, rows, Nc, Nf, per_ray_z, white_bg, **kw)
            for k, v in o2.items():
                if k == "normal" and not kw.get("normals", True) or not kw.get(k, True):
                    assert v is None
                else:
                    assert _bits(v, out[k]), (k, kw)
        # ---- normal
        nrm = out["normal"].cpu().numpy().astype(np.float64)
        assert out["normal"].shape == (n, 3)
        if Nf:
            rgb0 = composite_fine_fwd(*fine, white_bg=False)[0].cpu().numpy().astype(np.float64)
            e_rgb = np.abs(rgb0 - ref[False]["rgb"][rows]).max()
            e_nrm = np.abs(nrm - r["normal"][rows]).max()
            print(f"R {R} ({Nc}, {Nf}) rows {rows.start}: e_normal {e_nrm:.3e} e_rgb {e_rgb:.3e}")
            assert e_nrm <= 2 * max(e_rgb, EPS)
        else:
            u = A.unit_normals_f32(d["gc"][rows].numpy())
            prod = w.cpu().numpy()[..., None] * u
            assert prod.dtype == np.float32
            e_nrm = np.abs(nrm - prod.astype(np.float64).sum(1)).max()
            print(f"R {R} N {Nc} rows {rows.start}: normal max|d| {e_nrm:.3e} against the device's weights")
            assert e_nrm <= EPS
        assert (np.linalg.norm(nrm, axis=-1) <= out["acc"].cpu().numpy() + 1e-6).all()
        # ---- median depth: bitwise on every ray the restatement decides
        keep = ~bad[rows]
        med = out["depth_median"].cpu().numpy()
        assert np.array_equal(med[keep], r["depth_med"][rows][keep].astype(np.float32))
        # the special rays
        for k in range(rows.start, min(rows.stop, 4)):
            i = k - rows.start
            if k == 1:
                assert out["acc"][i] == 0 and not out["normal"][i].any()
                last = max(float(d["zc"][k, -1] if per_ray_z else d["zc"][-1]), float(d["zf"][k, -1]) if Nf else 0.0)
                assert med[i] == np.float32(last)
            if k == 2:
                assert out["acc"][i] > 0.99


def test_composite_aov_zero_gradient_and_nan():
    """A zero gradient contributes nothing and a NaN gradient counts as zero:
    the normal is the sum over the other samples, from the device's own weights."""
    from codenerf_amd.engine import composite_aov, composite_fwd
    d, _, _ = _case(64, 0, True)
    dv = _dev()
    rows = slice(0, 5)
    g = d["gc"][rows].clone()
    g[4, 10] = float("nan")
    g[4, 11] = 0.0
    sc, rc, zc = (d[k][rows].contiguous().to(dv) for k in ("sc", "rc", "zc"))
    out = composite_aov(sc, rc, zc, 64, 5, True, grad_c=g.reshape(-1, 3).to(dv))
    w = torch.empty(5, 64, dtype=torch.float32, device=dv)
    composite_fwd(sc, rc, zc, 5, 64, True, weights=w)
    u = A.unit_normals_f32(g.numpy())
    assert not u[4, 10].any() and not u[4, 11].any()
    want = (w.cpu().numpy()[..., None] * u).astype(np.float64).sum(1)
    assert np.isfinite(out["normal"].cpu().numpy()).all()
    assert np.abs(out["normal"].cpu().numpy() - want).max() <= EPS


# ------------------------------------------------------------------ render_aov
H = W = 8
NETS = [(3, p) for p in U.PLANS] + [(2, "fp32")]        # the srncar net on every plan, the default net at fp32


def _scene(Nf):
    """8 x 8 rays; 32 coarse samples, or 16 + 16 with fine samples computed once
    on the CPU (the fp32 oracle's sample_pdf at u = (j + 0.5) / 16)."""
    ro, vd, _ = U.camera_rays(H, W)
    return ro, vd, torch.linspace(0.8, 1.8, 16 if Nf else 32)


def _oracle_normal(sb, Nf, dtype, plan=None):
    """(normal (R, 3), z_f or None): autograd of codenerf_forward's sigma with
    respect to the sample points, composited over the (merged) samples in
    ``dtype``; float64, or fp32 under a plan's emulation."""
    params = U.net_params(sb, sigma_shift=2.0)
    ro, vd, z = _scene(Nf)
    s, t, obj = U.codes()
    p = U.tparams(params, dtype)
    sc, tc = torch.tensor(s[obj:obj + 1], dtype=dtype), torch.tensor(t[obj:obj + 1], dtype=dtype)
    ro, vd = ro.to(dtype), vd.to(dtype)

    def field(zz):
        xyz = (ro[:, None, :] + vd[:, None, :] * zz[..., None]).detach().requires_grad_()
        sig, _ = ref_cpu.codenerf_forward(p, xyz, vd[:, None, :].expand(-1, zz.shape[-1], -1), sc, tc,
                                          shape_blocks=sb, texture_blocks=1)
        sig[..., 0].sum().backward()
        return sig[..., 0].detach(), xyz.grad

    z_f = None
    if Nf:
        z_f = _cached(("zf", sb), lambda: ref_cpu.sample_pdf(_oracle_sigma32(sb), z, torch.full((H * W, Nf), 0.5)))
    with (U.emu_context(plan) if plan else contextlib.nullcontext()):
        zc = z.to(dtype).expand(H * W, -1)
        sig, g = field(zc)
        zm = zc
        if Nf:
            sig_f, g_f = field(z_f.to(dtype))
            zm, sig, g = ref_cpu.merge_samples(zc, z_f.to(dtype), (sig, sig_f), (g, g_f))
    w = ref_cpu.composite_weights(sig, zm)
    n = g.norm(dim=-1, keepdim=True)
    u = torch.where(n > 0, -g / n, torch.zeros_like(g))
    return (w[..., None] * u).sum(1).numpy(), z_f


def _oracle_sigma32(sb):
    params = U.net_params(sb, sigma_shift=2.0)
    ro, vd, z = _scene(16)
    s, t, obj = U.codes()
    p = U.tparams(params, torch.float32)
    with torch.no_grad():
        xyz = ro[:, None, :] + vd[:, None, :] * z[None, :, None]
        sig, _ = ref_cpu.codenerf_forward(p, xyz, vd[:, None, :].expand(-1, 16, -1), torch.tensor(s[obj:obj + 1]),
                                          torch.tensor(t[obj:obj + 1]), shape_blocks=sb, texture_blocks=1)
    return sig[..., 0]


def _step(sb, plan, **kw):
    from codenerf_amd.render import ImageStep
    m = U.model(U.net_params(sb, sigma_shift=2.0), sb, precision=plan)
    s, t, obj = U.codes()
    return ImageStep(m, **kw), torch.tensor(s[obj], device=_dev()), torch.tensor(t[obj], device=_dev())


@pytest.mark.parametrize("Nf", [0, 16])
@pytest.mark.parametrize("sb,plan", NETS)
def test_render_aov(sb, plan, Nf):
    step, s, t = _step(sb, plan)
    ro, vd, z = (x.to(_dev()) for x in _scene(Nf))
    exact, z_f = _cached(("n64", sb, Nf), lambda: _oracle_normal(sb, Nf, torch.float64))
    emu, _ = _cached(("nemu", sb, plan, Nf), lambda: _oracle_normal(sb, Nf, torch.float32, plan))
    kw = dict(z_f=z_f.to(_dev())) if Nf else {}
    if Nf:
        rgb, depth = step.render_fine(ro, vd, z, Nf, s, t, **kw)
    else:
        rgb, depth = step.render(ro, vd, z, s, t)
    out = step.render_aov(ro, vd, z, s, t, n_fine=Nf, **kw)
    torch.cuda.synchronize()
    assert _bits(out["rgb"], rgb) and _bits(out["depth"], depth)
    assert out["acc"].shape == out["depth_median"].shape == (H * W,) and out["normal"].shape == (H * W, 3)
    # no backward, and nothing else changes, without the normals
    eng = step.model.engine()
    calls = []
    bwd = eng.mlp_bwd
    eng.mlp_bwd = lambda *a, **k: calls.append(1) or bwd(*a, **k)
    try:
        plain = step.render_aov(ro, vd, z, s, t, n_fine=Nf, normals=False, **kw)
        assert not calls
        step.render_aov(ro, vd, z, s, t, n_fine=Nf, **kw)
        assert calls
    finally:
        del eng.mlp_bwd
    assert plain["normal"] is None
    for k in ("rgb", "depth", "acc", "depth_median"):
        assert _bits(plain[k], out[k]), k
    # ray parts (a 512-sample workspace: 8 of the 64 rays per part): the same bits
    parts = type(step)(step.model, act_budget=eng.act_bytes_per_sample() * 512)
    small = parts.render_aov(ro, vd, z, s, t, n_fine=Nf, **kw)
    for k in out:
        assert _bits(small[k], out[k]), k
    # the normal image against the float64 oracle
    e_gpu, e_emu = U.rel_l2(out["normal"].cpu().numpy(), exact), U.rel_l2(emu, exact)
    print(f"normal {plan} ({sb},1) Nf {Nf}: err_gpu {e_gpu:.3e} err_emu {e_emu:.3e} ratio {e_gpu / max(e_emu, 1e-300):.2f}")
    assert np.linalg.norm(exact) > 0.1
    assert e_gpu <= U.MARGIN * e_emu, (e_gpu, e_emu)


@pytest.mark.parametrize("rays,N", [(64, 32), (25, 16), (7, 48)])
@pytest.mark.parametrize("sb,plan", NETS)
def test_codes_forward_is_the_inference_forward(sb, plan, rays, N):
    """cn_mlp_fwd_codes (ray mode, into a workspace, at row 0 and at a later
    row) gives the sigma and rgb of cn_mlp_fwd without one, bit for bit: whole
    tiles (64 x 32), padded (25 x 16 = 400, 7 x 48 = 336: a ray across slabs)."""
    step, s, t = _step(sb, plan)
    eng, params = step.model.engine(), step.model.param_list()
    ro, vd, _ = U.camera_rays(H, W)
    ro, vd = ro[:rays].contiguous().to(_dev()), vd[:rays].contiguous().to(_dev())
    z = torch.linspace(0.8, 1.8, N, device=_dev())
    eng.ensure_packed(params, bwd=True)
    blob, _ = eng.latent_fwd(params, s, t)
    M = rays * N
    ray = dict(rays_o=ro, rays_d=vd, z=z, z_stride=0, n_samples=N)
    sig, rgb = eng.mlp_fwd(blob, M, **ray)
    for row0 in (0, 512):
        act = eng.new_act(row0 + M)
        sig_c, rgb_c = eng.mlp_fwd(blob, M, act=act, act_M=row0 + M, act_row0=row0, codes=True, **ray)
        torch.cuda.synchronize()
        assert _bits(sig_c[:M], sig[:M]) and _bits(rgb_c[:M], rgb[:M]), (plan, row0)


@pytest.mark.parametrize("Nf", [0, 16])
@pytest.mark.parametrize("sb,plan", NETS)
def test_a_texture_swap_leaves_the_geometry_buffers_alone(sb, plan, Nf):
    """sigma is taken before the texture code enters (src/model.py:36-53)."""
    step, s, t = _step(sb, plan)
    ro, vd, z = (x.to(_dev()) for x in _scene(Nf))
    t2 = torch.tensor(U.codes()[1][0], device=_dev())
    assert not torch.equal(t, t2)
    a = step.render_aov(ro, vd, z, s, t, n_fine=Nf)
    zf = step.last_z_f
    b = step.render_aov(ro, vd, z, s, t2, n_fine=Nf)
    torch.cuda.synchronize()
    for k in ("depth", "acc", "depth_median", "normal"):
        assert _bits(a[k], b[k]), k
    assert not torch.equal(a["rgb"], b["rgb"])
    if Nf:
        assert _bits(zf, step.last_z_f)
    # and a shape swap moves them
    c = step.render_aov(ro, vd, z, torch.tensor(U.codes()[0][0], device=_dev()), t, n_fine=Nf)
    assert not torch.equal(a["depth"], c["depth"]) and not torch.equal(a["normal"], c["normal"])


# ------------------------------------------------------------------ render.py
def _checkpoint(tmp_path):
    from oracle.params import make_codes
    params = U.net_params(3, sigma_shift=2.0)
    s, t = make_codes(5, 3)
    run = tmp_path / "exps" / "run"
    run.mkdir(parents=True)
    torch.save({"model_params": {k: torch.tensor(v) for k, v in params.items()},
                "shape_code_params": {"weight": torch.tensor(s)}, "texture_code_params": {"weight": torch.tensor(t)}},
               run / "models.pth")
    hp = {"net_hyperparams": dict(shape_blocks=3, texture_blocks=1, W=256, num_xyz_freq=10, num_dir_freq=4,
                                  latent_dim=256),
          "near": 0.8, "far": 1.8, "N_samples": 32, "N_importance": 0, "precision": "fp32"}
    (tmp_path / "hp.json").write_text(json.dumps(hp))
    return params, torch.tensor(s), torch.tensor(t)


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


@pytest.mark.parametrize("n_fine", [0, 8])
def test_render_py(tmp_path, n_fine):
    import render
    from codenerf_amd.edit import rgb_to_uint8
    from codenerf_amd.render import ImageStep
    from codenerf_amd.utils import get_rays
    params, s, t = _checkpoint(tmp_path)
    base = ["--saved_dir", "run", "--jsonfile", str(tmp_path / "hp.json"), "--size", "16", "--focal", "20",
            "--n_importance", str(n_fine)]
    step = ImageStep(U.model(params, 3))
    z = torch.linspace(0.8, 1.8, 32, device=_dev())

    def want(frame, si, ti):
        ro, vd = get_rays(16, 16, 20.0, torch.tensor(frame["pose"], device=_dev()))
        sc, tc = s[si].to(_dev()), t[ti].to(_dev())
        rgb = step.render_fine(ro, vd, z, n_fine, sc, tc)[0] if n_fine else step.render(ro, vd, z, sc, tc)[0]
        return rgb_to_uint8(rgb.reshape(16, 16, 3).cpu().numpy())

    # a turntable of the shape of object 0 with the texture blended from 1 to 2, with its four maps
    out = tmp_path / "turn"
    meta = render.main(base + ["--shape", "0", "--texture", "1", "2", "--frames", "3", "--azimuth", "0", "360",
                               "--aov", "True", "--out", str(out)], exp_root=str(tmp_path / "exps"))
    names = sorted(os.listdir(out))
    assert names == sorted([f"{stem}_{k:03d}.png" for stem in ("rgb", "depth", "depthmed", "normal", "alpha")
                            for k in range(3)] + ["frames.json"])
    assert json.load(open(out / "frames.json")) == meta
    fr = meta["frames"]
    assert [f["t_texture"] for f in fr] == [0.0, 0.5, 1.0] and [f["t_shape"] for f in fr] == [0.0] * 3
    assert [f["azimuth"] for f in fr] == [0.0, 120.0, 240.0]
    assert all(f["shape"] == [0] and f["texture"] == [1, 2] for f in fr)
    assert np.array_equal(_png(out / "rgb_000.png"), want(fr[0], 0, 1))
    assert np.array_equal(_png(out / "rgb_002.png"), want(fr[2], 0, 2))
    assert _png(out / "normal_000.png").shape == (16, 16, 3) and _png(out / "depth_000.png").shape == (16, 16)
    # the four maps of a frame are render_aov's at its pose and codes, encoded by aov_to_uint8
    from codenerf_amd.edit import AOV_NAMES, aov_to_uint8, blend
    ro, vd = get_rays(16, 16, 20.0, torch.tensor(fr[1]["pose"], device=_dev()))
    aov = step.render_aov(ro, vd, z, s[0].to(_dev()), blend(t[1], t[2], 0.5).to(_dev()), n_fine=n_fine)
    for name, stem in AOV_NAMES.items():
        a = aov[name].reshape(16, 16, -1).squeeze(-1).cpu().numpy()
        assert np.array_equal(_png(out / f"{stem}_001.png"), aov_to_uint8(name, a, 0.8, 1.8)), stem
    # a two-frame blend of both codes at a fixed camera: the last frame is object J's render
    out2 = tmp_path / "blend"
    meta2 = render.main(base + ["--shape", "0", "2", "--texture", "0", "2", "--frames", "2", "--azimuth", "40",
                                "--out", str(out2)], exp_root=str(tmp_path / "exps"))
    assert sorted(os.listdir(out2)) == ["frames.json", "rgb_000.png", "rgb_001.png"]
    f0, f1 = meta2["frames"]
    assert (f0["t_shape"], f0["t_texture"], f1["t_shape"], f1["t_texture"]) == (0.0, 0.0, 1.0, 1.0)
    assert f0["pose"] == f1["pose"] and f0["azimuth"] == f1["azimuth"] == 40.0
    assert np.array_equal(_png(out2 / "rgb_000.png"), want(f0, 0, 0))
    assert np.array_equal(_png(out2 / "rgb_001.png"), want(f1, 2, 2))
