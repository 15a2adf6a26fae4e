"""GPU: the masked image loss -- cn_render_loss_masked, cn_render_loss_fine_masked,
ImageStep's ray_weight / acc_target / sil_coef, and Optimizer(mask=...).

Per loss chunk of nb rays, with a weight m_r per ray, an opacity target a_r,
the coefficient sil_coef and acc_r the ray's weight sum:

    loss = sum_r [ m_r sum_c (col_rc - gt_rc)^2 + 3 sil_coef (acc_r - a_r)^2 ] / (3 nb)

The reference has neither weights nor a silhouette term, and oracle/ has no
masked loss: the expected values are the restatement below (``_chunk_losses``,
``_masked_image_step``) on top of oracle.ref_cpu's composite_weights,
volume_rendering, merge_samples and codenerf_forward, differentiated by torch
autograd on the CPU.

Bars, each the existing bar of the same arithmetic:
  * kernels (test_gpu_fine.py's render_loss_fine bars): rgb and acc rtol 1e-5 /
    atol 1e-6, chunk losses rtol 1e-5, dsig rtol 1e-4 / atol 1e-7, drgb rtol
    1e-4 / atol 1e-8; the fine kernel's coarse gradients as increments over a
    small gradient already present;
  * steps (test_fine_train_step_fp32_matches_oracle's): rgb / losses rtol 1e-4,
    parameter and code gradients rtol 2e-3, atol 2e-6 max(1, max|g|);
  * the identity, no-information and Optimizer checks have no tolerance
    (torch.equal).
"""
import os

import numpy as np
import pytest
import torch

from golden_util import case_params, load
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

SIL = 0.1
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ restatement
def _chunk_losses(out, acc, gt, chunk, m, a, lam):
    """The loss of every chunk (tensors) and their sum: mean over the chunk of
    m diff^2 + lam x mean over the chunk's rays of (acc - a)^2."""
    R = out.shape[0]
    losses, tot = [], 0.0
    for s in range(0, R, chunk):
        e = slice(s, min(s + chunk, R))
        nb = e.stop - e.start
        se = ((out[e] - gt[e]) ** 2).sum(-1)
        l = ((se if m is None else m[e] * se)).sum() / (3 * nb)
        if lam and a is not None:
            l = l + lam * ((acc[e] - a[e]) ** 2).sum() / nb
        losses.append(l)
        tot = tot + l
    return losses, tot


def _composite(sig, rgb, z):
    """-> (rgb (R,3) on the white background, acc (R,))."""
    if sig.shape[-1] == 1:
        # one sample: its interval is the closing 1e10 one and T = 1 (ref_cpu
        # takes the closing interval's shape from the first gap, of which a
        # single sample has none)
        w = 1 - torch.exp(-sig * 1e10)
        return (w[..., None] * rgb).sum(-2) + 1 - w.sum(-1)[..., None], w.sum(-1)
    out, _ = ref_cpu.volume_rendering(sig, rgb, z)
    return out, ref_cpu.composite_weights(sig, z).sum(-1)


# ------------------------------------------------------------------ kernel inputs
# Conditioning of the inputs.  A ray whose opacity is below 1 has sigma = 0 at
# its last sample (the closing interval is 1e10: any density there saturates
# the ray), and d loss / d sigma of that sample is 1e10 T d w with
#   d w = sum_c g_c (c_c - 1) + g_acc,
# four terms that cancel at random when colours and targets are random: at a
# cancellation of 1 in 1000 the fp32 restatement itself is 1e-4 off its own
# float64 version, and 1e10 puts that far above any absolute floor.  The rays
# that exercise the silhouette gradient ("open" rays: the even ones, opacity
# spread over about (0.2, 1), and ray 1, which has no density at all) are
# therefore background-like pixels, for which every term has one sign: sample
# colours in [0, 0.9), a target in [1.25, 1.75) -- brighter than anything the
# ray can render (col <= 1), so g_c < 0 and the squared error is no small
# difference either -- and opacity target 0 (g_acc >= 0).  On those of them
# whose weight is 0 the gradient is the silhouette term alone.  The open rays
# are thinned by no less than 0.2: alpha = 1 - exp(-sigma delta) carries an
# absolute 6e-8 per sample however small it is, which over 256 samples of an
# almost transparent ray is the whole 1e-6 floor of the rgb / acc bar.  The odd
# rays keep random colours, targets and opacity targets; they are saturated
# (density up to the last sample), where d sigma of the last sample is 0 and
# the rest has the scale the bars were set for.
def _mask_inputs(R, chunk, g):
    """Weights: 0, 1 and fractional values mixed, the second chunk (when there
    is one) entirely 0; targets in {0, 1} (0 on the open rays and on ray 1)."""
    kind = torch.randint(0, 3, (R,), generator=g)
    m = torch.where(kind == 0, torch.zeros(R), torch.where(kind == 1, torch.ones(R), torch.rand(R, generator=g)))
    if R > chunk:
        m[chunk:2 * chunk] = 0.0
    a = (torch.rand(R, generator=g) < 0.5).float()
    a[::2] = 0.0
    a[1:2] = 0.0
    return m.contiguous(), a.contiguous()


def _open_rays(sig, z, R):
    """The even rays end in empty space (sigma 0 from z = 1.6 on) and are
    thinned, so their opacities cover (0.2, 1) instead of sitting at 1."""
    zz = z.expand(R, -1) if z.dim() == 1 else z
    thin = torch.linspace(0.2, 1.0, R)[:, None]
    open_ = (torch.arange(R) % 2 == 0)[:, None]
    return torch.where(open_, torch.where(zz >= 1.6, torch.zeros_like(sig), sig * thin), sig)


def _background_like(gt, g, *colours):
    """Colours in [0, 0.9) and a target in [1.25, 1.75) on the open rays and on ray 1."""
    for c in colours:
        c[::2] = torch.rand(c[::2].shape, generator=g) * 0.9
        c[1:2] = torch.rand(c[1:2].shape, generator=g) * 0.9
    gt[::2] = 1.25 + 0.5 * torch.rand(gt[::2].shape, generator=g)
    gt[1:2] = 1.25 + 0.5 * torch.rand(gt[1:2].shape, generator=g)


def _coarse_inputs(R, N):
    g = torch.Generator().manual_seed(1000 + 7 * N + R)
    z = torch.linspace(0.8, 1.8, N) if N > 1 else torch.tensor([1.3])
    sig = _open_rays(torch.rand(R, N, generator=g) * 6, z, R)
    if R > 2:
        sig[1] = 0.0                                  # acc = 0
        sig[2, N // 2] = 1e4                          # an opaque wall: acc ~ 1
    rgb = torch.randn(R, N, 3, generator=g)
    gt = torch.rand(R, 3, generator=g)
    _background_like(gt, g, rgb)
    return z, sig, rgb, gt, g


def _fine_inputs(Nc, Nf):
    """As test_gpu_fine.py / test_gpu_fine_opt.py build them: ray 0 holds a
    coarse / fine tie, ray 1 no density, ray 2 an opaque wall."""
    R = 257
    g = torch.Generator().manual_seed(2000 + Nc + Nf)
    zc = torch.linspace(0.8, 1.8, Nc)
    zf = torch.sort(0.8 + torch.rand(R, Nf, generator=g), -1).values
    zf[0, :4] = zc[3]
    zf[0] = torch.sort(zf[0]).values
    sc = _open_rays(torch.rand(R, Nc, generator=g) * 6, zc, R)
    sf = _open_rays(torch.rand(R, Nf, generator=g) * 6, zf, R)
    sc[1], sf[1] = 0.0, 0.0
    sc[2, Nc // 2] = 1e4
    rc = torch.randn(R, Nc, 3, generator=g)
    rf = torch.randn(R, Nf, 3, generator=g)
    gt = torch.rand(R, 3, generator=g)
    _background_like(gt, g, rc, rf)
    return zc, zf, sc, sf, rc, rf, gt, g


def _report(tag, got, ref, rtol, atol, ref64=None):
    """Print the worst error beside its bar (and, given the float64
    restatement, the fp32 restatement's own error against it, in units of the
    same bar), then assert the bar."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bar = np.maximum(atol + rtol * np.abs(ref), 1e-300)
    err = np.abs(got - ref)
    worst = float((err / bar).max()) if err.size else 0.0
    own = ""
    if ref64 is not None:
        e64 = np.abs(ref - np.asarray(ref64, dtype=np.float64))
        own = (f"; restatement fp32 vs float64 {float((e64 / bar).max()):.3f}, "
               f"kernel vs float64 {float((np.abs(got - np.asarray(ref64, dtype=np.float64)) / bar).max()):.3f}")
    print(f"  {tag}: max|d| {float(err.max()) if err.size else 0.0:.3e}, worst error / bar {worst:.3f} "
          f"(rtol {rtol:g}, atol {atol:g}){own}")
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=tag)


# ------------------------------------------------------------------ 1: plain-case identity
def test_plain_case_is_the_plain_kernels_bits():
    """weight None or all ones, sil_coef 0: rgb, chunk losses, dsig, drgb of
    the masked entries equal the plain entries', coarse and fine."""
    from codenerf_amd.engine import render_loss, render_loss_fine, render_loss_fine_masked, render_loss_masked
    R, Nc, Nf, chunk = 257, 64, 64, 100
    zc, zf, sc, sf, rc, rf, gt, g = _cached(("fine_in", Nc, Nf), lambda: _fine_inputs(Nc, Nf))
    dv = _dev()
    t = lambda x: x.contiguous().to(dv)
    a = (torch.rand(R, generator=torch.Generator().manual_seed(3)) < 0.5).float().to(dv)
    ones = torch.ones(R, device=dv)
    plain = render_loss(t(sc), t(rc), t(zc), R, Nc, t(gt), chunk)
    for kw in (dict(), dict(ray_weight=ones), dict(ray_weight=ones, acc_target=a), dict(acc_target=a)):
        got = render_loss_masked(t(sc), t(rc), t(zc), R, Nc, t(gt), chunk, sil_coef=0.0, **kw)
        for x, y, name in zip(got[:4], plain, ("rgb", "losses", "dsig", "drgb")):
            assert torch.equal(x, y), (name, sorted(kw))
    g0 = torch.Generator().manual_seed(4)
    dsc0, drc0 = torch.randn(R * Nc, generator=g0), torch.randn(R * Nc, 3, generator=g0)

    def fine(fn, **kw):
        dsc, drc = t(dsc0.clone()), t(drc0.clone())
        dsf, drf = torch.empty(R * Nf, device=dv), torch.empty(R * Nf, 3, device=dv)
        out = fn(t(sc), t(rc), t(zc), Nc, t(sf), t(rf), t(zf), Nf, R, t(gt), chunk, dsc, drc, dsf, drf, **kw)
        return (out[0], out[1], dsc, drc, dsf, drf), out

    plain_f, _ = fine(render_loss_fine)
    for kw in (dict(), dict(ray_weight=ones), dict(ray_weight=ones, acc_target=a)):
        got, out = fine(render_loss_fine_masked, sil_coef=0.0, **kw)
        for x, y, name in zip(got, plain_f, ("rgb", "losses", "dsig_c", "drgb_c", "dsig_f", "drgb_f")):
            assert torch.equal(x, y), (name, sorted(kw))
        assert out[2].shape == (R,)


# ------------------------------------------------------------------ 2: kernels vs restatement
COARSE_SHAPES = [(257, 64, 2048), (257, 32, 100), (257, 96, 77),         # the fine test's coarse halves
                 (257, 1, 100), (257, 65, 100), (257, 256, 100), (1, 64, 100), (5, 64, 2)]


@pytest.mark.parametrize("lam", [0.0, SIL])
@pytest.mark.parametrize("R,N,chunk", COARSE_SHAPES)
def test_render_loss_masked_matches_restatement(R, N, chunk, lam):
    from codenerf_amd.engine import render_loss_masked
    z, sig, rgb, gt, g = _cached(("coarse_in", R, N), lambda: _coarse_inputs(R, N))
    m, a = _cached(("mask_in", R, N, chunk), lambda: _mask_inputs(R, chunk, torch.Generator().manual_seed(R + N)))
    if R == 1:
        m = torch.tensor([0.625])

    def restate(dt):
        s_, r_ = sig.clone().to(dt).requires_grad_(), rgb.clone().to(dt).requires_grad_()
        out, acc = _composite(s_, r_, z.to(dt))
        losses, tot = _chunk_losses(out, acc, gt.to(dt), chunk, m.to(dt), a.to(dt), lam)
        tot.backward()
        return out.detach(), acc.detach(), torch.stack(losses).detach(), s_.grad, r_.grad

    out, acc, losses, ds_r, dr_r = restate(torch.float32)
    r64 = restate(torch.float64)
    dv = _dev()
    t = lambda x: x.contiguous().to(dv)
    got_rgb, got_l, dsig, drgb, got_acc = render_loss_masked(t(sig), t(rgb), t(z), R, N, t(gt), chunk, ray_weight=t(m),
                                                             acc_target=t(a), sil_coef=lam)
    torch.cuda.synchronize()
    print(f"coarse R {R} N {N} chunk {chunk} sil_coef {lam}")
    _report("rgb", got_rgb.cpu(), out, 1e-5, 1e-6, r64[0])
    _report("acc", got_acc.cpu(), acc, 1e-5, 1e-6, r64[1])
    _report("losses", got_l.cpu(), losses, 1e-5, 0.0, r64[2])
    _report("dsig", dsig.cpu().reshape(R, N), ds_r, 1e-4, 1e-7, r64[3])
    _report("drgb", drgb.cpu().reshape(R, N, 3), dr_r, 1e-4, 1e-8, r64[4])
    if R > chunk and lam == 0.0:
        assert float(got_l[1]) == 0.0 and not bool(dsig.reshape(R, N)[chunk:2 * chunk].any())   # the weight-0 chunk
    # a NULL weight pointer is m = 1
    if lam:
        ref1, _ = _chunk_losses(out, acc, gt, chunk, None, a, lam)
        l1 = render_loss_masked(t(sig), t(rgb), t(z), R, N, t(gt), chunk, acc_target=t(a), sil_coef=lam)[1]
        _report("losses (no weights)", l1.cpu(), torch.stack(ref1), 1e-5, 0.0)


@pytest.mark.parametrize("lam", [0.0, SIL])
@pytest.mark.parametrize("Nc,Nf,chunk", [(64, 64, 2048), (32, 32, 100), (96, 160, 77)])
def test_render_loss_fine_masked_matches_restatement(Nc, Nf, chunk, lam):
    from codenerf_amd.engine import render_loss_fine_masked
    R = 257
    zc, zf, sc, sf, rc, rf, gt, g = _cached(("fine_in", Nc, Nf), lambda: _fine_inputs(Nc, Nf))
    m, a = _cached(("mask_in", R, Nc + Nf, chunk),
                   lambda: _mask_inputs(R, chunk, torch.Generator().manual_seed(R + Nc + Nf)))

    def restate(dt):
        leaves = [x.clone().to(dt).requires_grad_() for x in (sc, rc, sf, rf)]
        z_m, s_m, r_m = ref_cpu.merge_samples(zc.to(dt), zf.to(dt), (leaves[0], leaves[2]), (leaves[1], leaves[3]))
        out, acc = _composite(s_m, r_m, z_m)
        losses, tot = _chunk_losses(out, acc, gt.to(dt), chunk, m.to(dt), a.to(dt), lam)
        tot.backward()
        return [out.detach(), acc.detach(), torch.stack(losses).detach()] + [x.grad for x in leaves]

    ref, r64 = restate(torch.float32), restate(torch.float64)
    # an already-present coarse gradient, small so (d0 + grad) - d0 keeps grad's bits
    g0 = torch.Generator().manual_seed(9)
    dsc0, drc0 = torch.randn(R * Nc, generator=g0) * 1e-9, torch.randn(R * Nc, 3, generator=g0) * 1e-9
    dv = _dev()
    t = lambda x: x.contiguous().to(dv)
    dsc, drc = t(dsc0.clone()), t(drc0.clone())
    dsf, drf = torch.empty(R * Nf, device=dv), torch.empty(R * Nf, 3, device=dv)
    got_rgb, got_l, got_acc = render_loss_fine_masked(t(sc), t(rc), t(zc), Nc, t(sf), t(rf), t(zf), Nf, R, t(gt), chunk,
                                                      dsc, drc, dsf, drf, ray_weight=t(m), acc_target=t(a),
                                                      sil_coef=lam)
    torch.cuda.synchronize()
    print(f"fine Nc {Nc} Nf {Nf} chunk {chunk} sil_coef {lam}")
    _report("rgb", got_rgb.cpu(), ref[0], 1e-5, 1e-6, r64[0])
    _report("acc", got_acc.cpu(), ref[1], 1e-5, 1e-6, r64[1])
    _report("losses", got_l.cpu(), ref[2], 1e-5, 0.0, r64[2])
    _report("dsig_c", (dsc.cpu() - dsc0).reshape(R, Nc), ref[3], 1e-4, 1e-7, r64[3])
    _report("drgb_c", (drc.cpu() - drc0).reshape(R, Nc, 3), ref[4], 1e-4, 1e-8, r64[4])
    _report("dsig_f", dsf.cpu().reshape(R, Nf), ref[5], 1e-4, 1e-7, r64[5])
    _report("drgb_f", drf.cpu().reshape(R, Nf, 3), ref[6], 1e-4, 1e-8, r64[6])


def test_sil_coef_without_a_target_is_refused():
    from codenerf_amd import _lib
    from codenerf_amd.engine import render_loss_masked
    dv = _dev()
    x = torch.zeros(4 * 8, device=dv)
    with pytest.raises(ValueError):
        render_loss_masked(x, torch.zeros(32, 3, device=dv), torch.linspace(1, 2, 8).to(dv), 4, 8,
                           torch.zeros(4, 3, device=dv), 4, sil_coef=0.5)
    L = _lib.lib()
    assert L.cn_render_loss_masked(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 0, 4, 8, 1, _lib.ptr(x), 4, _lib.ptr(x),
                                   _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), None, None, 0.5, None,
                                   None) == -1
    assert b"cn_render_loss_masked" in L.cn_last_error()


# ------------------------------------------------------------------ steps
def _image_masks(H, W):
    """Weights: a checkerboard of 1 and 0.5 with a zero block (the top
    quarter of the rows); targets: a disc."""
    i, j = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = torch.where((i + j) % 2 == 0, torch.ones(H, W), torch.full((H, W), 0.5))
    m[:H // 4] = 0.0
    a = (((i - H / 2) ** 2 + (j - W / 2) ** 2) < (H / 3) ** 2).float()
    return m.reshape(-1).contiguous(), a.reshape(-1).contiguous()


def _model(g, precision):
    from codenerf_amd.model import CodeNeRF
    m = CodeNeRF(3, 1, precision=precision)
    m.load_state_dict({k: torch.tensor(v) for k, v in case_params(g).items()})
    return m.to(_dev())


def _gpu_step(g, precision, Nf, gt=None, rnd=None, z_f=None, **kw):
    """One ImageStep step on a golden case -> (model, shape table, texture
    table, coarse losses, fine losses or None, rgb, step)."""
    from codenerf_amd.render import ImageStep
    m = _model(g, precision)
    st = torch.nn.Parameter(torch.tensor(g["shape_table"], device=_dev()))
    tt = torch.nn.Parameter(torch.tensor(g["texture_table"], device=_dev()))
    step = ImageStep(m, chunk=int(g["chunk"]), reg_coef=1e-4)
    t = lambda k: torch.tensor(g[k], device=_dev())
    gt = t("gt") if gt is None else gt.to(_dev())
    if Nf:
        lc, lf, rgb, _ = step.forward_backward_fine(t("rays_o"), t("viewdir"), t("z_vals"), rnd.to(_dev()), gt, st, tt,
                                                    int(g["obj_idx"]), z_f=z_f, **kw)
    else:
        lc, rgb, _ = step.forward_backward(t("rays_o"), t("viewdir"), t("z_vals"), gt, st, tt, int(g["obj_idx"]), **kw)
        lf = None
    torch.cuda.synchronize()
    return m, st, tt, lc, lf, rgb, step


# ------------------------------------------------------------------ 3: masked pixels carry no information
@pytest.mark.parametrize("plan", ["fp32", "bf16x3f"])
def test_masked_pixels_carry_no_information(plan):
    g = load("n64_16x16")
    H, W, Nf = int(g["H"]), int(g["W"]), 64
    R = H * W
    m, a = _image_masks(H, W)
    gt1 = torch.tensor(g["gt"])
    gt2 = gt1.clone()
    noise = torch.rand(R, 3, generator=torch.Generator().manual_seed(21))
    gt2[m == 0] = noise[m == 0]                       # the targets differ exactly where the weight is 0
    assert int((m == 0).sum()) > 0 and not torch.equal(gt1, gt2) and torch.equal(gt1[m > 0], gt2[m > 0])
    rnd = torch.rand(R, Nf, generator=torch.Generator().manual_seed(22))

    def run(gt, weight):
        _, st, tt, lc, lf, rgb, step = _gpu_step(g, plan, Nf, gt=gt, rnd=rnd, weight_grads=False, input_grads=True,
                                                 ray_weight=weight.to(_dev()), acc_target=a.to(_dev()), sil_coef=SIL)
        return [lc, lf, st.grad, tt.grad, step.last_ray_grads[0], step.last_ray_grads[1], rgb, step.last_acc]

    one, two = run(gt1, m), run(gt2, m)
    for x, y, name in zip(one, two, ("coarse losses", "fine losses", "d shape", "d texture", "d rays_o", "d viewdirs",
                                     "rgb", "acc")):
        assert torch.equal(x, y), name
    assert bool(one[2].any()) and bool(one[4].any())                 # and they are not trivially zero
    ones = torch.ones(R)
    u1, u2 = run(gt1, ones), run(gt2, ones)
    for k, name in ((0, "coarse losses"), (1, "fine losses"), (2, "d shape"), (3, "d texture"), (4, "d rays_o")):
        assert not torch.equal(u1[k], u2[k]), name


# ------------------------------------------------------------------ 4: step vs restatement, fp32
def _masked_image_step(p, st, tt, oi, ro, vd, z_c, z_f, gt, chunk, m, a, lam, reg_coef=1e-4):
    """oracle.ref_cpu's image_step / fine_image_step (z_f None: coarse only)
    with the masked loss in place of the chunk-mean MSE; backward per chunk.
    -> (coarse losses, fine losses, rgb of the last loss)."""
    Nc = z_c.shape[-1]
    R = ro.shape[0]
    lc_all, lf_all, outs = [], [], []
    for s0 in range(0, R, chunk):
        e = slice(s0, min(s0 + chunk, R))
        s, t = st[oi][None], tt[oi][None]
        xyz = ro[e, None, :] + vd[e, None, :] * z_c[..., None]
        sig_c, rgb_c = ref_cpu.codenerf_forward(p, xyz, vd[e, None, :].expand(-1, Nc, -1), s, t)
        out, acc = _composite(sig_c[..., 0], rgb_c, z_c)
        (lc,), loss = _chunk_losses(out, acc, gt[e], chunk, m[e], a[e], lam)
        lc_all.append(lc.item())
        if z_f is not None:
            zf = z_f[e]
            xyz_f = ro[e, None, :] + vd[e, None, :] * zf[..., None]
            sig_f, rgb_f = ref_cpu.codenerf_forward(p, xyz_f, vd[e, None, :].expand(-1, zf.shape[-1], -1), s, t)
            z_m, s_m, r_m = ref_cpu.merge_samples(z_c, zf, (sig_c[..., 0], sig_f[..., 0]), (rgb_c, rgb_f))
            out, acc = _composite(s_m, r_m, z_m)
            (lf,), tot_f = _chunk_losses(out, acc, gt[e], chunk, m[e], a[e], lam)
            lf_all.append(lf.item())
            loss = loss + tot_f
        if s0 == 0:
            loss = loss + reg_coef * torch.mean(torch.norm(s, dim=-1) + torch.norm(t, dim=-1))
        loss.backward()
        outs.append((out.detach(), acc.detach()))
    return lc_all, lf_all, torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


@pytest.mark.parametrize("case,Nf", [("ragged_48x48_n16", 0), ("ragged_48x48_n16", 40), ("n64_16x16", 64)])
def test_masked_step_fp32_matches_restatement(case, Nf):
    g = load(case)
    H, W = int(g["H"]), int(g["W"])
    R = H * W
    m, a = _image_masks(H, W)
    rnd = torch.rand(R, Nf, generator=torch.Generator().manual_seed(5)) if Nf else None
    kw = dict(ray_weight=m.to(_dev()), acc_target=a.to(_dev()), sil_coef=SIL)
    mod, st, tt, lc, lf, rgb, step = _gpu_step(g, "fp32", Nf, rnd=rnd, weight_grads=True, **kw)
    zf = step.last_z_f if Nf else None
    p = ref_cpu.param_tensors(case_params(g))
    st_r = torch.tensor(g["shape_table"], requires_grad=True)
    tt_r = torch.tensor(g["texture_table"], requires_grad=True)
    ro, vd, z = torch.tensor(g["rays_o"]), torch.tensor(g["viewdir"]), torch.tensor(g["z_vals"])
    lc_r, lf_r, rgb_r, acc_r = _masked_image_step(p, st_r, tt_r, int(g["obj_idx"]), ro, vd, z,
                                                  zf.cpu() if Nf else None, torch.tensor(g["gt"]), int(g["chunk"]),
                                                  m, a, SIL)
    print(f"step {case} Nf {Nf}")
    _report("rgb", rgb.cpu(), rgb_r, 1e-4, 1e-6)
    _report("acc", step.last_acc.cpu(), acc_r, 1e-4, 1e-6)
    _report("coarse losses", lc.cpu(), np.array(lc_r), 1e-4, 0.0)
    if Nf:
        _report("fine losses", lf.cpu(), np.array(lf_r), 1e-4, 0.0)
    bar = lambda b: 2e-6 * max(1.0, float(np.abs(b).max()))
    worst = 0.0
    for k, prm in mod.named_parameters():
        x, y = prm.grad.cpu().numpy(), p[k].grad.numpy()
        worst = max(worst, float((np.abs(x - y) / (bar(y) + 2e-3 * np.abs(y))).max()))
        np.testing.assert_allclose(x, y, rtol=2e-3, atol=bar(y), err_msg=k)
    print(f"  parameter gradients: worst error / bar {worst:.3f} (rtol 2e-3, atol 2e-6 max(1, max|g|))")
    _report("d shape table", st.grad.cpu(), st_r.grad, 2e-3, bar(st_r.grad.numpy()))
    _report("d texture table", tt.grad.cpu(), tt_r.grad, 2e-3, bar(tt_r.grad.numpy()))
    # the codes-only path: the same losses, the same code gradients, no weight gradients
    mod2, st2, tt2, lc2, lf2, rgb2, step2 = _gpu_step(g, "fp32", Nf, rnd=rnd, z_f=zf, weight_grads=False, **kw)
    _report("codes-only coarse losses", lc2.cpu(), np.array(lc_r), 1e-4, 0.0)
    if Nf:
        _report("codes-only fine losses", lf2.cpu(), np.array(lf_r), 1e-4, 0.0)
    _report("codes-only d shape table", st2.grad.cpu(), st_r.grad, 2e-3, bar(st_r.grad.numpy()))
    _report("codes-only d texture table", tt2.grad.cpu(), tt_r.grad, 2e-3, bar(tt_r.grad.numpy()))
    _report("codes-only against training, d shape", st2.grad.cpu(), st.grad.cpu(), 2e-3, bar(st.grad.cpu().numpy()))
    _report("codes-only against training, d texture", tt2.grad.cpu(), tt.grad.cpu(), 2e-3,
            bar(tt.grad.cpu().numpy()))
    for k, prm in mod2.named_parameters():
        assert prm.grad is None or not bool(prm.grad.any()), k


def test_default_step_leaves_no_opacity_and_checks_sizes():
    g = load("n64_16x16")
    _, _, _, _, _, _, step = _gpu_step(g, "fp32", 0, weight_grads=False)
    assert step.last_acc is None
    with pytest.raises(ValueError):
        _gpu_step(g, "fp32", 0, weight_grads=False, ray_weight=torch.ones(7, device=_dev()))


# ------------------------------------------------------------------ 5: Optimizer
NET = {"shape_blocks": 3, "texture_blocks": 1, "W": 256, "num_xyz_freq": 10, "num_dir_freq": 4, "latent_dim": 256}


def _hpams(root, **extra):
    hp = {"net_hyperparams": dict(NET),
          "data": {"cat": "srn_cars", "splits": "cars_train", "data_dir": root, "n_train_views": 3, "n_test_views": 3},
          "N_samples": 16, "near": 0.8, "far": 1.8, "loss_reg_coef": 1e-4, "precision": "fp32", "N_importance": 8}
    hp.update(extra)
    return hp


@pytest.fixture(scope="module")
def painted(tmp_path_factory):
    """One synthetic object, 3 views at 32 x 32 with masks, twice: a 16 x 16
    square (a quarter of the view) of target view 0 painted black in one copy
    and red in the other, and cleared in both copies' mask file; and a
    randomly initialised checkpoint."""
    from PIL import Image
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.model import CodeNeRF
    base = tmp_path_factory.mktemp("masked_opt")
    roots = {}
    for colour, value in (("black", (0, 0, 0)), ("red", (255, 0, 0))):
        root = str(base / colour)
        split = make_synthetic_srn(root, "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4,
                                   masks=True)
        obj = os.path.join(split, sorted(os.listdir(split))[0])
        img = np.array(Image.open(os.path.join(obj, "rgb", "000000.png")).convert("RGB"))
        msk = np.array(Image.open(os.path.join(obj, "mask", "000000.png")))
        assert msk[8:24, 8:24].any(), "the square must cover part of the object"
        img[8:24, 8:24] = value
        msk[8:24, 8:24] = 0
        Image.fromarray(img).save(os.path.join(obj, "rgb", "000000.png"))
        Image.fromarray(msk).save(os.path.join(obj, "mask", "000000.png"))
        roots[colour] = root
    exps = str(base / "exps")
    os.makedirs(os.path.join(exps, "t"))
    torch.manual_seed(11)
    net = CodeNeRF(**NET)
    torch.save({"model_params": net.state_dict(),
                "shape_code_params": {"weight": torch.randn(4, 256) * 0.1},
                "texture_code_params": {"weight": torch.randn(4, 256) * 0.1}}, os.path.join(exps, "t", "models.pth"))
    return roots, exps


def _optimize(painted, colour, **kw):
    from codenerf_amd.optimizer import Optimizer
    roots, exps = painted
    torch.manual_seed(0)
    opt = Optimizer("t", 0, [0], "test", hpams=_hpams(roots[colour]), batch_size=512, num_opts=3, exp_root=exps, **kw)
    opt.optimize_objs([0], lr=1e-2, lr_half_interval=2, save_img=False)
    return opt


def _codes(opt):
    return opt.optimized_shapecodes.clone(), opt.optimized_texturecodes.clone()


def _same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


def test_optimizer_ignores_what_the_mask_excludes(painted):
    """The painted square is outside the mask.  With bg_weight 0 (rays outside
    the mask weigh nothing) its colour cannot reach the codes; without a mask
    it does.  (ray_weight = fg + bg_weight (1 - fg): at bg_weight 1 every ray
    weighs 1 and the square counts again -- then the run is the unmasked one,
    bit for bit, which is checked as well.)"""
    black = _codes(_optimize(painted, "black", mask="files", bg_weight=0.0))
    red = _codes(_optimize(painted, "red", mask="files", bg_weight=0.0))
    assert torch.isfinite(black[0]).all() and _same(black, red)
    plain_black = _codes(_optimize(painted, "black", mask=None))
    plain_red = _codes(_optimize(painted, "red", mask=None))
    assert not _same(plain_black, plain_red)
    assert not _same(black, plain_black)
    # mask=None is the loop of an Optimizer built without the new arguments
    assert _same(plain_black, _codes(_optimize(painted, "black")))
    # all-ones weights and no silhouette term: the masked kernels give the plain kernels' bits
    assert _same(plain_red, _codes(_optimize(painted, "red", mask="files", bg_weight=1.0)))


def test_optimizer_white_mask_with_the_silhouette_term(painted):
    opt = _optimize(painted, "black", mask="white", sil_coef=SIL)
    out = torch.load(os.path.join(opt.save_dir, "codes.pth"), map_location="cpu", weights_only=True)
    assert set(out) == {"ids", "num_obj", "optimized_shapecodes", "optimized_texturecodes", "psnr_eval", "ssim_eval"}
    assert len(opt.psnr_opt[0]) == 3 and np.isfinite(opt.psnr_opt[0]).all()
    assert len(out["psnr_eval"][0]) == 2 and np.isfinite(out["psnr_eval"][0]).all()
    assert torch.isfinite(out["optimized_shapecodes"]).all() and torch.isfinite(out["optimized_texturecodes"]).all()
    assert opt.step_impl.last_acc.shape == (32 * 32,)
    # psnr_opt logs the masked loss's value: the silhouette term is part of it
    assert opt.psnr_opt[0] != _optimize(painted, "black", mask="white").psnr_opt[0]


def test_optimizer_files_mask_needs_the_directory(painted, tmp_path):
    from codenerf_amd.data import make_synthetic_srn
    from codenerf_amd.optimizer import Optimizer
    _, exps = painted
    make_synthetic_srn(str(tmp_path), "srn_cars", "cars_test", n_obj=1, n_views=3, H=32, W=32, focal=32.8, seed=4)
    opt = Optimizer("t", 0, [0], "test", hpams=_hpams(str(tmp_path)), batch_size=512, num_opts=1, exp_root=exps,
                    mask="files")
    with pytest.raises(FileNotFoundError, match="mask/"):
        opt.optimize_objs([0], save_img=False)
    with pytest.raises(ValueError):
        Optimizer("t", 0, [0], "test", hpams=_hpams(str(tmp_path)), batch_size=512, num_opts=1, exp_root=exps,
                  mask="alpha")
