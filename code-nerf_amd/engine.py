"""Thin host wrapper of the C ABI: one ``Engine`` = one plan (network
configuration + precision) on one device.

It owns the packed weight blobs (repacked only when a parameter changed), the
device pointer tables, and hands torch tensors to the ``cn_*`` entry points
on torch's current stream.  All arithmetic happens in the HIP library.
"""
import ctypes
import os

import torch
from torch.autograd.graph import increment_version

from . import _lib
from ._lib import check, ptr

PRECISIONS = {"fp32": _lib.CN_FP32, "bf16": _lib.CN_BF16, "bf16x3": _lib.CN_BF16X3, "bf16x3f": _lib.CN_BF16X3F}
# Training-workspace budget per call (bytes): larger images are rendered in
# ray parts that fit it (render.ImageStep, model.CodeNeRF.forward).  At the
# srncar net one training sample holds ~8.2 KB (bf16) / ~16 KB (fp32) of
# activation planes, so 48 GiB is ~6.2 M / ~3.1 M samples per part.
ACT_BUDGET = int(os.environ.get("CODENERF_ACT_BUDGET", str(48 << 30)))


class Engine:
    def __init__(self, shape_blocks=3, texture_blocks=1, W=256, num_xyz_freq=10, num_dir_freq=4,
                 latent_dim=256, precision="fp32", device=None):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        self.L = _lib.lib()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.precision = precision
        self.net = dict(shape_blocks=shape_blocks, texture_blocks=texture_blocks, W=W,
                        num_xyz_freq=num_xyz_freq, num_dir_freq=num_dir_freq, latent_dim=latent_dim)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.cn_plan_create(shape_blocks, texture_blocks, W, num_xyz_freq, num_dir_freq, latent_dim,
                                        PRECISIONS[precision], ctypes.byref(h)), "cn_plan_create")
        self._plan = h
        self.n_params = self.L.cn_plan_num_params(h)
        self.n_inject = self.L.cn_plan_num_inject(h)
        self.blob_floats = self.L.cn_blob_floats(h)
        self.pack_fwd = torch.empty(self.L.cn_packed_bytes(h, 0), dtype=torch.uint8, device=self.device)
        self.pack_bwd = torch.empty(self.L.cn_packed_bytes(h, 1), dtype=torch.uint8, device=self.device)
        self._packed_key = None
        self._param_tab = None
        self._tables = {}

    def __del__(self):
        try:
            if getattr(self, "_plan", None) is not None and self._plan.value:
                self.L.cn_plan_destroy(self._plan)
        except Exception:
            pass

    # ------------------------------------------------------------ helpers
    @property
    def stream(self):
        return _lib.stream_ptr(self.device)

    def pad(self, M):
        return self.L.cn_pad_samples(self._plan, M)

    def act_bytes(self, M):
        return self.L.cn_act_bytes(self._plan, M)

    def dw_ws_bytes(self, M):
        return self.L.cn_dw_ws_bytes(self._plan, M)

    def act_bytes_per_sample(self):
        return self.L.cn_act_bytes_per_sample(self._plan)

    def max_act_samples(self, budget=None):
        """Most training samples one workspace of ``budget`` bytes holds
        (a multiple of the 256-sample tile, at most CN_MAX_SAMPLES)."""
        b = ACT_BUDGET if budget is None else int(budget)
        n = (b // self.act_bytes_per_sample()) // 256 * 256
        return max(256, min(n, self.L.cn_max_samples() // 256 * 256))

    def table(self, tensors):
        """Device array of the tensors' data pointers (cached)."""
        key = tuple(t.data_ptr() for t in tensors)
        tab = self._tables.get(key)
        if tab is None:
            if len(self._tables) > 64:
                self._tables.clear()
            tab = torch.tensor(list(key), dtype=torch.int64, device=self.device)
            self._tables[key] = tab
        return tab

    def _check_params(self, params):
        if len(params) != self.n_params:
            raise ValueError(f"expected {self.n_params} parameter tensors, got {len(params)}")
        for p in params:
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("parameters must be contiguous float32 tensors on the engine's device")

    # ------------------------------------------------------------ weights
    def ensure_packed(self, params, bwd=True):
        key = (tuple((p.data_ptr(), p._version) for p in params), bwd)
        if key == self._packed_key:
            return
        self._check_params(params)
        tab = self.table(params)
        check(self.L.cn_pack_weights(self._plan, ptr(tab), ptr(self.pack_fwd),
                                     ptr(self.pack_bwd) if bwd else None, self.stream), "cn_pack_weights")
        self._packed_key = key
        self._param_tab = tab       # the weights the packs came from (mlp_dw's fold reads them)

    def latent_fwd(self, params, shape_code, texture_code):
        blob = torch.empty(self.blob_floats, dtype=torch.float32, device=self.device)
        zvec = torch.empty(self.n_inject, 256, dtype=torch.float32, device=self.device)
        check(self.L.cn_latent_fwd(self._plan, ptr(self.table(params)), ptr(shape_code), ptr(texture_code),
                                   ptr(blob), ptr(zvec), self.stream), "cn_latent_fwd")
        return blob, zvec

    # ------------------------------------------------------------ MLP
    def mlp_fwd(self, blob, M, xyz=None, viewdir=None, rays_o=None, rays_d=None, z=None, z_stride=0,
                n_samples=0, act=None, act_M=0, act_row0=0, sigma=None, rgb=None, codes=False):
        """act_M / act_row0: the workspace is sized for act_M samples and this
        pass fills rows [act_row0, act_row0 + pad(M)) (coarse + fine passes).
        codes: codes-only optimisation -- store only what mlp_bwd(codes=True)
        needs (cn_mlp_fwd_codes)."""
        Mp = self.pad(M)
        if sigma is None:
            sigma = torch.empty(Mp, dtype=torch.float32, device=self.device)
        if rgb is None:
            rgb = torch.empty(Mp, 3, dtype=torch.float32, device=self.device)
        assert sigma.numel() >= Mp and rgb.numel() >= 3 * Mp
        fn = self.L.cn_mlp_fwd_codes if codes else self.L.cn_mlp_fwd
        check(fn(self._plan, ptr(self.pack_fwd), ptr(blob), M, ptr(xyz), ptr(viewdir),
                 ptr(rays_o), ptr(rays_d), ptr(z), z_stride, n_samples, ptr(sigma), ptr(rgb),
                 ptr(act), int(act_M), int(act_row0), self.stream), "cn_mlp_fwd")
        return sigma, rgb

    def new_act(self, M):
        return torch.empty(self.act_bytes(M), dtype=torch.uint8, device=self.device)

    def mlp_bwd(self, blob, M, dsigma, drgb, act, codes=False, act_M=0, row0=0, pose=False):
        """dX chain over rows [row0, row0 + pad(M)) of an act_M-sample workspace
        (act_M 0: M); dsigma / drgb hold the range's rows.  codes: the
        codes-only variant (stores only the planes mlp_dbias reads).  pose:
        the codes-only variant that also stores the two input-side gradient
        planes mlp_input_grad reads (cn_mlp_bwd_pose)."""
        fn = self.L.cn_mlp_bwd_pose if pose else self.L.cn_mlp_bwd_codes if codes else self.L.cn_mlp_bwd_rows
        check(fn(self._plan, ptr(self.pack_bwd), ptr(blob), M, ptr(dsigma), ptr(drgb), ptr(act), int(act_M),
                 int(row0), self.stream), "cn_mlp_bwd")

    def mlp_input_grad(self, act, M, xyz=None, viewdir=None, rays_o=None, rays_d=None, z=None, z_stride=0,
                       n_samples=0, act_M=0, row0=0, params=None, per_ray=True):
        """Gradient with respect to the network inputs over rows [row0, row0 +
        pad(M)), after mlp_bwd(pose=True) or the training backward over the
        same rows; the inputs are the forward's (points or rays x z).
        -> (d_xyz [Mp,3], d_viewdir [Mp,3]) and, in ray mode with per_ray,
        (d_rays_o [R,3], d_rays_d [R,3]); ``params``: tensors or a table,
        default the parameters of the last ensure_packed."""
        ptab = self._param_tab if params is None else (
            params if isinstance(params, torch.Tensor) else self.table(params))
        if ptab is None:
            raise RuntimeError("mlp_input_grad: no packed weights (call ensure_packed before the forward)")
        Mp = self.pad(M)
        dxyz = torch.empty(Mp, 3, dtype=torch.float32, device=self.device)
        dvd = torch.empty(Mp, 3, dtype=torch.float32, device=self.device)
        dro = drd = None
        if xyz is None and per_ray:
            R = M // max(1, int(n_samples))
            dro = torch.empty(R, 3, dtype=torch.float32, device=self.device)
            drd = torch.empty(R, 3, dtype=torch.float32, device=self.device)
        check(self.L.cn_mlp_input_grad(self._plan, ptr(ptab), ptr(act), int(act_M), int(row0), M, ptr(xyz),
                                       ptr(viewdir), ptr(rays_o), ptr(rays_d), ptr(z), int(z_stride),
                                       int(n_samples), ptr(dxyz), ptr(dvd), ptr(dro), ptr(drd), self.stream),
              "cn_mlp_input_grad")
        return dxyz, dvd, dro, drd

    def mlp_dw(self, act, M, zvec, grads, dbuf, ws=None, act_M=0, row0=0, db_accum=False, nwg=0, params=None):
        """Weight gradients over rows [row0, row0 + pad(M)) (grads accumulate;
        dbuf is overwritten, or accumulated with db_accum).  ``grads``: the
        list of gradient tensors or a pointer table from ``table()``;
        nwg: persistent workgroups (0 = one per CU).  The encoding_shape fold
        reads the forward's weights: ``params`` (tensors or a table), default
        the parameters of the last ensure_packed."""
        ptab = self._param_tab if params is None else (
            params if isinstance(params, torch.Tensor) else self.table(params))
        if ptab is None:
            raise RuntimeError("mlp_dw: no packed weights (call ensure_packed before the forward)")
        if ws is None:
            ws = torch.empty(self.dw_ws_bytes(M), dtype=torch.uint8, device=self.device)
        tab = grads if isinstance(grads, torch.Tensor) else self.table(grads)
        # the tables may be used on a stream other than the one they were made on
        cur = torch.cuda.current_stream(self.device)
        tab.record_stream(cur)
        ptab.record_stream(cur)
        check(self.L.cn_mlp_dw_rows(self._plan, ptr(act), int(act_M), int(row0), M, ptr(zvec),
                                    ptr(ptab), ptr(tab), ptr(dbuf), int(bool(db_accum)), int(nwg), ptr(ws),
                                    self.stream), "cn_mlp_dw_rows")

    def mlp_dbias(self, act, M, dbuf, ws=None, act_M=0):
        if ws is None:
            ws = torch.empty(self.dw_ws_bytes(M), dtype=torch.uint8, device=self.device)
        check(self.L.cn_mlp_dbias(self._plan, ptr(act), int(act_M), M, ptr(dbuf), ptr(ws), self.stream),
              "cn_mlp_dbias")

    def latent_bwd(self, params, grads, shape_code, texture_code, zvec, dbuf, d_shape, d_tex, reg_coef=0.0,
                   reg_out=None):
        scratch = torch.empty(self.n_inject, 256, dtype=torch.float32, device=self.device)
        check(self.L.cn_latent_bwd(self._plan, ptr(self.table(params)), ptr(self.table(grads)), ptr(shape_code),
                                   ptr(texture_code), ptr(zvec), ptr(dbuf), ptr(scratch), ptr(d_shape), ptr(d_tex),
                                   float(reg_coef), ptr(reg_out), self.stream), "cn_latent_bwd")


# ---------------------------------------------------------------- rendering
def _dev_stream(t):
    return _lib.stream_ptr(t.device)


def composite_fwd(sigma, rgb, z, R, N, white_bg=True, weights=None):
    L = _lib.lib()
    z_stride = 0 if z.numel() == N else N
    out_rgb = torch.empty(R, 3, dtype=torch.float32, device=sigma.device)
    depth = torch.empty(R, dtype=torch.float32, device=sigma.device)
    check(L.cn_composite_fwd(ptr(sigma), ptr(rgb), ptr(z), z_stride, R, N, int(white_bg), ptr(out_rgb), ptr(depth),
                             ptr(weights), _dev_stream(sigma)), "cn_composite_fwd")
    return out_rgb, depth


def composite_bwd(sigma, rgb, z, R, N, grad_rgb, grad_depth=None, white_bg=True):
    L = _lib.lib()
    z_stride = 0 if z.numel() == N else N
    dsig = torch.empty(R * N, dtype=torch.float32, device=sigma.device)
    drgb = torch.empty(R * N, 3, dtype=torch.float32, device=sigma.device)
    check(L.cn_composite_bwd(ptr(sigma), ptr(rgb), ptr(z), z_stride, R, N, int(white_bg), ptr(grad_rgb),
                             ptr(grad_depth), ptr(dsig), ptr(drgb), _dev_stream(sigma)), "cn_composite_bwd")
    return dsig, drgb


def _loss_outputs(R, chunk, dev, acc=False):
    """What a loss entry writes next to the gradients: rgb (R, 3), the per-ray
    errors (R,), the chunk losses and, for a masked entry, the opacity (R,)."""
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    return new(R, 3), new(R), new((R + chunk - 1) // chunk), new(R) if acc else None


def render_loss(sigma, rgb, z, R, N, gt, chunk, white_bg=True, dsig=None, drgb=None):
    L = _lib.lib()
    dev = sigma.device
    z_stride = 0 if z.numel() == N else N
    out_rgb, ray_se, chunk_loss, _ = _loss_outputs(R, chunk, dev)
    if dsig is None:
        dsig = torch.empty(R * N, dtype=torch.float32, device=dev)
    if drgb is None:
        drgb = torch.empty(R * N, 3, dtype=torch.float32, device=dev)
    check(L.cn_render_loss(ptr(sigma), ptr(rgb), ptr(z), z_stride, R, N, int(white_bg), ptr(gt), chunk,
                           ptr(out_rgb), ptr(ray_se), ptr(chunk_loss), ptr(dsig), ptr(drgb), _dev_stream(sigma)),
          "cn_render_loss")
    return out_rgb, chunk_loss, dsig, drgb


def _mask_args(ray_weight, acc_target, sil_coef, who):
    """Arguments of the masked loss entries: None / None / 0 is the plain loss."""
    sil_coef = float(sil_coef)
    if sil_coef > 0 and acc_target is None:
        raise ValueError(f"{who}: sil_coef > 0 needs acc_target")
    for t in (ray_weight, acc_target):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError(f"{who}: ray_weight / acc_target must be contiguous float32 tensors")
    return sil_coef


def render_loss_masked(sigma, rgb, z, R, N, gt, chunk, white_bg=True, dsig=None, drgb=None, ray_weight=None,
                       acc_target=None, sil_coef=0.0):
    """render_loss with per-ray weights m (R,) and the silhouette term: per
    chunk of nb rays, sum_r [m_r se_r + 3 sil_coef (acc_r - acc_target_r)^2]
    / (3 nb), acc = the ray's weight sum.  ray_weight None: m = 1; sil_coef 0
    or acc_target None: no silhouette term.
    -> (rgb, chunk losses, dsig, drgb, acc (R,))."""
    L = _lib.lib()
    dev = sigma.device
    sil_coef = _mask_args(ray_weight, acc_target, sil_coef, "render_loss_masked")
    z_stride = 0 if z.numel() == N else N
    out_rgb, ray_se, chunk_loss, acc = _loss_outputs(R, chunk, dev, acc=True)
    if dsig is None:
        dsig = torch.empty(R * N, dtype=torch.float32, device=dev)
    if drgb is None:
        drgb = torch.empty(R * N, 3, dtype=torch.float32, device=dev)
    check(L.cn_render_loss_masked(ptr(sigma), ptr(rgb), ptr(z), z_stride, R, N, int(white_bg), ptr(gt), chunk,
                                  ptr(out_rgb), ptr(ray_se), ptr(chunk_loss), ptr(dsig), ptr(drgb),
                                  ptr(ray_weight), ptr(acc_target), sil_coef, ptr(acc), _dev_stream(sigma)),
          "cn_render_loss_masked")
    return out_rgb, chunk_loss, dsig, drgb, acc


def sample_pdf(sigma_c, z_c, R, Nc, rand):
    """Fine z (R, Nf) from the coarse densities; rand (R, Nf) in [0, 1)."""
    L = _lib.lib()
    Nf = rand.shape[-1]
    zc_stride = 0 if z_c.numel() == Nc else Nc
    z_f = torch.empty(R, Nf, dtype=torch.float32, device=sigma_c.device)
    check(L.cn_sample_pdf(ptr(sigma_c), ptr(z_c), zc_stride, R, Nc, ptr(rand), Nf, ptr(z_f),
                          _dev_stream(sigma_c)), "cn_sample_pdf")
    return z_f


def render_loss_fine(sigma_c, rgb_c, z_c, Nc, sigma_f, rgb_f, z_f, Nf, R, gt, chunk, dsig_c, drgb_c,
                     dsig_f, drgb_f, white_bg=True):
    """Fine composite + MSE over the merged samples; accumulates into
    dsig_c / drgb_c, writes dsig_f / drgb_f.  -> (rgb (R,3), chunk losses)."""
    L = _lib.lib()
    dev = sigma_c.device
    zc_stride = 0 if z_c.numel() == Nc else Nc
    out_rgb, ray_se, chunk_loss, _ = _loss_outputs(R, chunk, dev)
    check(L.cn_render_loss_fine(ptr(sigma_c), ptr(rgb_c), ptr(z_c), zc_stride, Nc, ptr(sigma_f), ptr(rgb_f),
                                ptr(z_f), Nf, R, int(white_bg), ptr(gt), chunk, ptr(out_rgb), ptr(ray_se),
                                ptr(chunk_loss), ptr(dsig_c), ptr(drgb_c), ptr(dsig_f), ptr(drgb_f),
                                _dev_stream(sigma_c)), "cn_render_loss_fine")
    return out_rgb, chunk_loss


def render_loss_fine_masked(sigma_c, rgb_c, z_c, Nc, sigma_f, rgb_f, z_f, Nf, R, gt, chunk, dsig_c, drgb_c,
                            dsig_f, drgb_f, white_bg=True, ray_weight=None, acc_target=None, sil_coef=0.0):
    """render_loss_fine with the weights and the silhouette term of
    render_loss_masked (acc over the merged samples).
    -> (rgb (R,3), chunk losses, acc (R,))."""
    L = _lib.lib()
    dev = sigma_c.device
    sil_coef = _mask_args(ray_weight, acc_target, sil_coef, "render_loss_fine_masked")
    zc_stride = 0 if z_c.numel() == Nc else Nc
    out_rgb, ray_se, chunk_loss, acc = _loss_outputs(R, chunk, dev, acc=True)
    check(L.cn_render_loss_fine_masked(ptr(sigma_c), ptr(rgb_c), ptr(z_c), zc_stride, Nc, ptr(sigma_f), ptr(rgb_f),
                                       ptr(z_f), Nf, R, int(white_bg), ptr(gt), chunk, ptr(out_rgb), ptr(ray_se),
                                       ptr(chunk_loss), ptr(dsig_c), ptr(drgb_c), ptr(dsig_f), ptr(drgb_f),
                                       ptr(ray_weight), ptr(acc_target), sil_coef, ptr(acc),
                                       _dev_stream(sigma_c)), "cn_render_loss_fine_masked")
    return out_rgb, chunk_loss, acc


def composite_fine_fwd(sigma_c, rgb_c, z_c, Nc, sigma_f, rgb_f, z_f, Nf, R, white_bg=True, acc=False):
    """Forward-only composite over the merged coarse + fine samples (the
    forward half of render_loss_fine).  -> (rgb (R,3), depth (R,)[, acc (R,)])."""
    L = _lib.lib()
    dev = sigma_c.device
    zc_stride = 0 if z_c.numel() == Nc else Nc
    out_rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    out_acc = torch.empty(R, dtype=torch.float32, device=dev) if acc else None
    check(L.cn_composite_fine_fwd(ptr(sigma_c), ptr(rgb_c), ptr(z_c), zc_stride, Nc, ptr(sigma_f), ptr(rgb_f),
                                  ptr(z_f), Nf, R, int(white_bg), ptr(out_rgb), ptr(depth), ptr(out_acc),
                                  _dev_stream(sigma_c)), "cn_composite_fine_fwd")
    return (out_rgb, depth, out_acc) if acc else (out_rgb, depth)


def composite_aov(sigma_c, rgb_c, z_c, Nc, R, white_bg=True, grad_c=None, sigma_f=None, rgb_f=None, z_f=None, Nf=0,
                  grad_f=None, acc=True, depth_median=True):
    """composite_fwd (Nf 0) or composite_fine_fwd with the geometry buffers
    (cn_composite_aov): -> dict(rgb (R,3), depth (R,), acc (R,) or None,
    depth_median (R,) or None, normal (R,3) or None).  grad_c (R*Nc, 3) and,
    with Nf > 0, grad_f (R*Nf, 3) = d sigma / d xyz per sample ask for the
    normal sum_k w_k u_k (not normalised)."""
    L = _lib.lib()
    dev = sigma_c.device
    zc_stride = 0 if z_c.numel() == Nc else Nc
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(rgb=new(R, 3), depth=new(R), acc=new(R) if acc else None,
               depth_median=new(R) if depth_median else None,
               normal=new(R, 3) if grad_c is not None or grad_f is not None else None)
    check(L.cn_composite_aov(ptr(sigma_c), ptr(rgb_c), ptr(z_c), zc_stride, int(Nc), ptr(grad_c), ptr(sigma_f),
                             ptr(rgb_f), ptr(z_f), int(Nf), ptr(grad_f), int(R), int(white_bg), ptr(out["rgb"]),
                             ptr(out["depth"]), ptr(out["acc"]), ptr(out["depth_median"]), ptr(out["normal"]),
                             _dev_stream(sigma_c)), "cn_composite_aov")
    return out


def occupancy_build(sigma, G, tau, dilate=0):
    """Grid bits (G^3 / 32 words, int32 storage) from the densities at the G^3
    cell centres: sigma >= tau (NaN occupied), dilated by `dilate` cells
    (cn_occupancy_build)."""
    L = _lib.lib()
    if sigma.numel() != G ** 3 or sigma.dtype != torch.float32 or not sigma.is_contiguous():
        raise ValueError(f"occupancy_build: sigma must hold G^3 = {G ** 3} contiguous float32 values")
    bits = torch.empty(G ** 3 // 32, dtype=torch.int32, device=sigma.device)
    check(L.cn_occupancy_build(ptr(sigma), int(G), float(tau), int(dilate), ptr(bits), _dev_stream(sigma)),
          "cn_occupancy_build")
    return bits


def sparse_mark(rays_o, rays_d, z, R, N, bits, G, lo, inv_cell, keep_last=True):
    """Which samples fall in a set cell of the grid (cn_sparse_mark)
    -> (keep (R, 8) int32 bit words, count (R,) int32)."""
    L = _lib.lib()
    if bits.numel() != G ** 3 // 32:
        raise ValueError(f"sparse_mark: a grid of {G}^3 cells has {G ** 3 // 32} words, got {bits.numel()}")
    z_stride = 0 if z.numel() == N else N
    keep = torch.empty(R, 8, dtype=torch.int32, device=rays_o.device)
    count = torch.empty(R, dtype=torch.int32, device=rays_o.device)
    check(L.cn_sparse_mark(ptr(rays_o), ptr(rays_d), ptr(z), z_stride, R, N, ptr(bits), int(G), float(lo[0]),
                           float(lo[1]), float(lo[2]), float(inv_cell), int(bool(keep_last)), ptr(keep), ptr(count),
                           _dev_stream(rays_o)), "cn_sparse_mark")
    return keep, count


def sparse_gather(rays_o, rays_d, z, R, N, keep, offset, Mk):
    """Points and view directions of the Mk kept samples, ray-major
    (cn_sparse_gather); offset (R,) int32 = the exclusive prefix sum of
    sparse_mark's counts, Mk their sum.  -> (xyz (Mk, 3), viewdir (Mk, 3))."""
    L = _lib.lib()
    z_stride = 0 if z.numel() == N else N
    xyz = torch.empty(Mk, 3, dtype=torch.float32, device=rays_o.device)
    vd = torch.empty(Mk, 3, dtype=torch.float32, device=rays_o.device)
    check(L.cn_sparse_gather(ptr(rays_o), ptr(rays_d), ptr(z), z_stride, R, N, ptr(keep), ptr(offset), ptr(xyz),
                             ptr(vd), _dev_stream(rays_o)), "cn_sparse_gather")
    return xyz, vd


def sparse_scatter(keep, offset, R, N, sigma_k, rgb_k, sigma=None, rgb=None):
    """Dense sigma (R*N,) and rgb (R*N, 3) from the compact rows: 0 at every
    sample that is not kept (cn_sparse_scatter)."""
    L = _lib.lib()
    if sigma is None:
        sigma = torch.empty(R * N, dtype=torch.float32, device=keep.device)
    if rgb is None:
        rgb = torch.empty(R * N, 3, dtype=torch.float32, device=keep.device)
    check(L.cn_sparse_scatter(ptr(keep), ptr(offset), R, N, ptr(sigma_k), ptr(rgb_k), ptr(sigma), ptr(rgb),
                              _dev_stream(keep)), "cn_sparse_scatter")
    return sigma, rgb


def _host_floats(vals):
    """A host float array for an h_* argument -> (keep-alive, pointer)."""
    a = (ctypes.c_float * len(vals))(*[float(v) for v in vals])
    return a, ctypes.cast(a, ctypes.c_void_p)


def scene_rays(rays_o, rays_d, transforms):
    """World rays in each object's frame (cn_scene_rays).  transforms: K rows of
    13 floats, the object -> world rotation row-major, the translation and
    1 / scale.  -> (origins (K, R, 3), directions (K, R, 3))."""
    L = _lib.lib()
    K, R = len(transforms), rays_o.shape[0]
    flat = [v for row in transforms for v in row]
    if len(flat) != 13 * K:
        raise ValueError("scene_rays: a transform is 13 floats (rotation 9, translation 3, 1 / scale)")
    out_o = torch.empty(K, R, 3, dtype=torch.float32, device=rays_o.device)
    out_d = torch.empty(K, R, 3, dtype=torch.float32, device=rays_o.device)
    keep, h = _host_floats(flat)
    check(L.cn_scene_rays(ptr(rays_o), ptr(rays_d), R, h, K, ptr(out_o), ptr(out_d), _dev_stream(rays_o)),
          "cn_scene_rays")
    return out_o, out_d


def scene_combine(sigma_k, rgb_k, inv_s, sigma=None, rgb=None):
    """The K object planes sigma_k (K, M) and rgb_k (K, M, 3) as one
    (cn_scene_combine); inv_s: K host floats 1 / scale.  -> (sigma (M,), rgb (M, 3))."""
    L = _lib.lib()
    K, M = len(inv_s), sigma_k.numel() // max(1, len(inv_s))
    if sigma_k.numel() != K * M or rgb_k.numel() != 3 * K * M:
        raise ValueError("scene_combine: sigma_k must hold K * M and rgb_k 3 * K * M values")
    if sigma is None:
        sigma = torch.empty(M, dtype=torch.float32, device=sigma_k.device)
    if rgb is None:
        rgb = torch.empty(M, 3, dtype=torch.float32, device=sigma_k.device)
    keep, h = _host_floats(inv_s)
    check(L.cn_scene_combine(ptr(sigma_k), ptr(rgb_k), h, K, M, ptr(sigma), ptr(rgb), _dev_stream(sigma_k)),
          "cn_scene_combine")
    return sigma, rgb


def scene_composite(sigma_c, rgb_c, z_c, Nc, R, inv_s, white_bg=True, sigma_f=None, rgb_f=None, z_f=None, Nf=0,
                    obj_c=None, obj_f=None, labels=True, acc_min=0.5):
    """composite_fwd (Nf 0) or composite_fine_fwd on a scene's combined planes,
    with the weights split back onto the K objects (cn_scene_composite): obj_c
    (K, R*Nc) and obj_f (K, R*Nf) are the object density planes that went into
    scene_combine.  -> dict(rgb (R,3), depth (R,), acc (R,), obj_acc (R, K) and
    instance (R,) int32, both None without labels)."""
    L = _lib.lib()
    dev = sigma_c.device
    K = len(inv_s)
    zc_stride = 0 if z_c.numel() == Nc else Nc
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    out = dict(rgb=new(R, 3), depth=new(R), acc=new(R), obj_acc=new(R, K) if labels else None,
               instance=torch.empty(R, dtype=torch.int32, device=dev) if labels else None)
    keep, h = _host_floats(inv_s)
    check(L.cn_scene_composite(ptr(sigma_c), ptr(rgb_c), ptr(z_c), zc_stride, int(Nc), ptr(sigma_f), ptr(rgb_f),
                               ptr(z_f), int(Nf), ptr(obj_c), ptr(obj_f), h, K, int(R), int(white_bg), float(acc_min),
                               ptr(out["rgb"]), ptr(out["depth"]), ptr(out["acc"]), ptr(out["obj_acc"]),
                               ptr(out["instance"]), _dev_stream(sigma_c)), "cn_scene_composite")
    return out


def _mesh_field(field, dims, who):
    nx, ny, nz = (int(n) for n in dims)
    if field.dtype != torch.float32 or not field.is_contiguous() or field.numel() != nx * ny * nz:
        raise ValueError(f"{who}: field must hold nx * ny * nz = {nx * ny * nz} contiguous float32 values")
    return nx, ny, nz


def mesh_count(field, dims, iso):
    """Crossing edges and triangles per lattice point (cn_mesh_count)
    -> (vflags uint8 [P], vcount int32 [P], tcount int32 [P])."""
    L = _lib.lib()
    nx, ny, nz = _mesh_field(field, dims, "mesh_count")
    P = nx * ny * nz
    vflags = torch.empty(P, dtype=torch.uint8, device=field.device)
    vcount = torch.empty(P, dtype=torch.int32, device=field.device)
    tcount = torch.empty(P, dtype=torch.int32, device=field.device)
    check(L.cn_mesh_count(ptr(field), nx, ny, nz, float(iso), ptr(vflags), ptr(vcount), ptr(tcount),
                          _dev_stream(field)), "cn_mesh_count")
    return vflags, vcount, tcount


def mesh_emit(field, dims, iso, lo, spacing, vflags, voff, toff, Nv, Nt, vert=None, tri=None):
    """Vertices and triangles of the iso-surface (cn_mesh_emit); voff / toff
    (P,) int32 = the exclusive prefix sums of mesh_count's counts, Nv / Nt their
    sums.  -> (vert (Nv, 3) float32, tri (Nt, 3) int32); rows past Nv / Nt of
    larger buffers handed in are left alone."""
    L = _lib.lib()
    nx, ny, nz = _mesh_field(field, dims, "mesh_emit")
    for t, dt in ((vflags, torch.uint8), (voff, torch.int32), (toff, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != nx * ny * nz:
            raise ValueError("mesh_emit: vflags (uint8), voff and toff (int32) must hold one contiguous value per point")
    if vert is None:
        vert = torch.empty(Nv, 3, dtype=torch.float32, device=field.device)
    if tri is None:
        tri = torch.empty(Nt, 3, dtype=torch.int32, device=field.device)
    if vert.numel() < 3 * Nv or tri.numel() < 3 * Nt:
        raise ValueError("mesh_emit: vert / tri hold fewer than Nv / Nt rows")
    check(L.cn_mesh_emit(ptr(field), nx, ny, nz, float(iso), float(lo[0]), float(lo[1]), float(lo[2]),
                         float(spacing[0]), float(spacing[1]), float(spacing[2]), ptr(vflags), ptr(voff), ptr(toff),
                         ptr(vert), ptr(tri), _dev_stream(field)), "cn_mesh_emit")
    return vert, tri


def get_rays_dev(H, W, focal, focal_is_f64, c2w):
    L = _lib.lib()
    dev = c2w.device
    ro = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    vd = torch.empty(H * W, 3, dtype=torch.float32, device=dev)
    check(L.cn_get_rays(H, W, float(focal), int(focal_is_f64), ptr(c2w), ptr(ro), ptr(vd), _dev_stream(c2w)),
          "cn_get_rays")
    return ro, vd


def get_rays_bwd(H, W, focal, focal_is_f64, c2w, d_rays_o, d_viewdirs):
    """Gradient of get_rays_dev's outputs with respect to c2w -> (3, 4)."""
    L = _lib.lib()
    dev = c2w.device
    out = torch.empty(3, 4, dtype=torch.float32, device=dev)
    ws = torch.empty(L.cn_get_rays_bwd_ws_bytes(H, W), dtype=torch.uint8, device=dev)
    check(L.cn_get_rays_bwd(H, W, float(focal), int(focal_is_f64), ptr(c2w), ptr(d_rays_o), ptr(d_viewdirs),
                            ptr(out), ptr(ws), _dev_stream(c2w)), "cn_get_rays_bwd")
    return out


def sample_points(ro, vd, z, R, N):
    L = _lib.lib()
    z_stride = 0 if z.numel() == N else N
    xyz = torch.empty(R, N, 3, dtype=torch.float32, device=ro.device)
    vrep = torch.empty(R, N, 3, dtype=torch.float32, device=ro.device)
    check(L.cn_sample_points(ptr(ro), ptr(vd), ptr(z), z_stride, R, N, ptr(xyz), ptr(vrep), _dev_stream(ro)),
          "cn_sample_points")
    return xyz, vrep


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, lrs, weight_decay, beta1, beta2, eps, step, zero_grad=False):
    """zero_grad: the kernel also sets every gradient to 0 after reading it."""
    L = _lib.lib()
    n = len(params)
    P = ctypes.c_void_p * n
    keep = []

    def arr(vals, ctype):
        a = (ctype * n)(*vals)
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    ptrs = lambda ts: arr([t.data_ptr() for t in ts], ctypes.c_void_p)
    counts = arr([t.numel() for t in params], ctypes.c_int)
    lr = arr([float(x) for x in lrs], ctypes.c_double)
    fn = L.cn_adamw_step_zero_grad if zero_grad else L.cn_adamw_step
    check(fn(n, ptrs(params), ptrs(grads), ptrs(exp_avgs), ptrs(exp_avg_sqs), counts, lr,
             float(weight_decay), float(beta1), float(beta2), float(eps), int(step),
             _dev_stream(params[0])), "cn_adamw_step")
    # the kernel wrote the tensors behind torch's back: bump their version
    # counters so version-keyed caches (the packed weights) see the update
    increment_version(list(params))
    increment_version(list(exp_avgs) + list(exp_avg_sqs))
