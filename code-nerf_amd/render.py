"""Fused training / rendering steps over whole images.

``ImageStep`` replaces the per-image body of the reference training loop
(src/trainer.py:65-84, and its twin src/optimizer.py:75-94): rays -> samples
-> CodeNeRF -> compositing -> chunk-mean MSE (+ code regulariser on chunk 0)
-> backward into ``.grad`` of the model parameters and the code rows.  The
reference processes 2048-ray chunks with a host sync per chunk; here an image
is rendered in as few launches as the activation budget allows, with the
chunk semantics of the loss (gradient = sum of chunk-mean gradients,
regulariser counted once) kept exactly.  Samples are generated inside the MLP
kernel from (ray, z); xyz is never materialised.

Large images (C5: 256^2 rays x 256 samples in fp32) are split into ray parts
of whole loss chunks whose training workspace fits ``engine.ACT_BUDGET``;
their gradients accumulate before the caller's optimiser step.

One host schedule serves every step: ``forward_backward`` (coarse only) and
``forward_backward_fine`` (coarse + fine) are the same ray-part loop
(``_step``) over the same part function (``_part``), the coarse-only step
being the case "no fine samples"; with fine samples the part adds sample_pdf,
the fine forward and its loss, the optional recompute forwards and a second
input-gradient reduction.  ``render`` and ``render_fine`` share their loop
(``_render``) the same way.

Backward schedule: the rows of a part (coarse rows, then fine rows) are cut
into ``bwd_ranges`` row ranges; the dX chain of range i runs on the current
stream while the weight-gradient pass of range i-1 runs on a side stream
(the dX chain is MFMA-bound, dW streams its operand planes from HBM).
"""
import ctypes

import torch

from . import _lib
from . import dp as _dp
from . import engine as _eng
from ._lib import check


class ImageStep:
    def __init__(self, model, chunk=2048, reg_coef=1e-4, white_bg=True, timers=None, overlap_dw=True,
                 bwd_ranges=2, dw_side_wgs=0, act_budget=None, max_rays=None):
        self.model = model
        self.timers = timers
        self.chunk = int(chunk)
        self.reg_coef = float(reg_coef)
        self.white_bg = bool(white_bg)
        # dX / dW pipelining (see module docstring); overlap_dw False: one dX
        # launch then one dW launch per part, on the current stream
        self.overlap_dw = bool(overlap_dw)
        self.bwd_ranges = max(1, int(bwd_ranges))
        self.dw_side_wgs = int(dw_side_wgs)      # workgroups of the overlapped dW launches (0: one per CU)
        self.act_budget = act_budget
        self.max_rays = max_rays                 # explicit cap on rays per part (tests)
        # store-vs-recompute A/B (fine step only): the loss forwards store no
        # dW operand planes; a second forward writes them before the backward
        self.recompute = False
        self.last_ray_grads = None               # forward_backward[_fine](input_grads=True)
        self.last_z_f = None                     # fine z of the last forward_backward_fine / render_fine
        self.last_acc = None                     # per-ray opacity of the last masked loss (ray_weight / acc_target)
        self.last_sparse = None                  # (kept coarse, kept fine, total) samples of the last render through a grid
        self._ws = {}                            # device -> grow-only workspace
        self._aov_ws = {}                        # device -> grow-only workspace of render_aov's normals
        self._side = {}                          # device -> side stream
        # called whenever a step starts writing .grad (dp.GradExchange's
        # mark_dirty: a fused zero-grad AdamW step must not mask them)
        self.grad_listeners = []

    # ------------------------------------------------------------ resources
    def _workspace(self, eng, M):
        """Activation workspace for at least M samples (grow-only, per device:
        every call passes its capacity as act_M, so one workspace serves every
        part size)."""
        ws = self._ws.get(eng.device)
        if ws is None or ws["cap"] < M:
            cap = eng.pad(M)
            if ws is not None:
                self._ws.pop(eng.device)
                del ws
            dev = eng.device
            ws = dict(cap=cap, act=eng.new_act(cap),
                      dw=torch.empty(eng.dw_ws_bytes(cap), dtype=torch.uint8, device=dev),
                      dbuf=torch.empty(eng.n_inject, 256, dtype=torch.float32, device=dev),
                      sig=torch.empty(cap, dtype=torch.float32, device=dev),
                      rgb=torch.empty(cap, 3, dtype=torch.float32, device=dev),
                      dsig=torch.empty(cap, dtype=torch.float32, device=dev),
                      drgb=torch.empty(cap, 3, dtype=torch.float32, device=dev))
            self._ws[eng.device] = ws
        return ws

    @staticmethod
    def _zero_pad_rows(ws, layout, ranges):
        """Upstream-gradient rows no loss kernel writes (the padding between
        and after the coarse and fine row ranges) must be 0 for the dX chain.
        They are zeroed when the row layout changes, not every step: nothing
        else writes them."""
        if ws.get("pad_layout") == layout:
            return
        for a, b in ranges:
            if b > a:
                ws["dsig"][a:b].zero_()
                ws["drgb"][a:b].zero_()
        ws["pad_layout"] = layout

    def side_stream(self, device):
        s = self._side.get(device)
        if s is None:
            s = torch.cuda.Stream(device)
            self._side[device] = s
        return s

    def ray_parts(self, eng, R, n_per_ray):
        """Contiguous ray ranges [(a, b)] of whole loss chunks whose training
        workspace (pad(rays x coarse) + rays x fine samples) fits the budget."""
        cap = eng.max_act_samples(self.act_budget)
        per = (cap - 256) // n_per_ray
        if self.max_rays:
            per = min(per, int(self.max_rays))
        per = per // self.chunk * self.chunk
        if per <= 0:
            raise ValueError(f"a loss chunk of {self.chunk} rays x {n_per_ray} samples does not fit the "
                             f"activation budget ({cap} samples): lower the chunk or raise CODENERF_ACT_BUDGET")
        return [(a, min(a + per, R)) for a in range(0, R, per)]

    @staticmethod
    def ensure_grads(tensors):
        for p in tensors:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return [p.grad for p in tensors]

    def _writing_grads(self):
        for f in self.grad_listeners:
            f()

    # ------------------------------------------------------------ backward
    def _bwd_dw(self, eng, blob, ws, zvec, gtab, M):
        """dX chain + weight gradients over rows [0, M) of the workspace
        (dsig / drgb rows already hold the upstream gradients, padding rows 0),
        pipelined over row ranges on two streams when overlap_dw is set."""
        tm = self.timers
        cap, act = ws["cap"], ws["act"]
        dsig, drgb = ws["dsig"], ws["drgb"]
        Mp = eng.pad(M)
        k = self.bwd_ranges if self.overlap_dw else 1
        k = max(1, min(k, Mp // 256))
        cuts = [(Mp // 256) * i // k * 256 for i in range(k)] + [M]
        ranges = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(k)]

        # timers: `contended` marks launches that share the chip with a launch
        # on the other stream (the bench reports kernel rooflines from the
        # uncontended ones)
        def bwd(r0, n, ov=False):
            ev = tm.mark("bwd") if tm else None
            eng.mlp_bwd(blob, n, dsig[r0:], drgb[r0:], act, act_M=cap, row0=r0)
            if tm:
                tm.done("bwd", ev, n=n, contended=ov)

        def dw(r0, n, i, nwg, ov=False):
            ev = tm.mark("dw") if tm else None
            eng.mlp_dw(act, n, zvec, gtab, ws["dbuf"], ws["dw"], act_M=cap, row0=r0, db_accum=i > 0, nwg=nwg)
            if tm:
                tm.done("dw", ev, n=n, contended=ov)

        if k == 1:
            bwd(0, M)
            dw(0, M, 0, 0)
            return
        main = torch.cuda.current_stream(eng.device)
        side = self.side_stream(eng.device)
        L = _lib.lib()

        def wait(waiter, signaller):
            # fence-less stream dependency (cn_stream_wait): a torch event's
            # record does a system-scope release -- an L2 write-back of the
            # planes the last kernel wrote, ~15 us of idle GPU per fork / join
            check(L.cn_stream_wait(ctypes.c_void_p(waiter.cuda_stream), ctypes.c_void_p(signaller.cuda_stream)),
                  "cn_stream_wait")

        bwd(*ranges[0])
        for i in range(1, k):
            wait(side, main)
            with torch.cuda.stream(side):
                dw(*ranges[i - 1], i - 1, self.dw_side_wgs, ov=True)
            bwd(*ranges[i], ov=True)
        # the last range's dW runs alone (every CU) on the main stream, right
        # behind its dX chain: the side stream's dW (which shares the partial
        # workspace) finished during that chain, so the join is free, where
        # handing the last dW to the side stream and joining after it added a
        # second cross-stream dependency per step
        wait(main, side)
        dw(*ranges[k - 1], k - 1, 0)

    # ------------------------------------------------------------ steps
    def forward_backward(self, rays_o, viewdirs, z_vals, gt, shape_table, texture_table, obj_idx,
                         reg=True, weight_grads=True, input_grads=False, ray_weight=None, acc_target=None,
                         sil_coef=0.0):
        """One image: returns (chunk losses [ceil(R/chunk)], rendered rgb [R,3],
        reg loss [1]).  Gradients are accumulated into .grad.  weight_grads
        False (codes-only optimisation, src/optimizer.py): the weight-gradient
        pass is replaced by the bias sums the code gradients need.
        input_grads (pose refinement; no reference counterpart): the gradient
        of the summed chunk losses with respect to every ray is left in
        ``self.last_ray_grads = (d_rays_o [R,3], d_viewdirs [R,3])`` (the
        codes path then runs the backward that also stores the two input-side
        gradient planes); the return value is unchanged.
        ray_weight (R,), acc_target (R,), sil_coef (no reference counterpart in
        code; the paper's real-image experiments mask the loss): any of them
        given, the loss of a chunk of nb rays is sum_r [m_r se_r + 3 sil_coef
        (acc_r - acc_target_r)^2] / (3 nb) with m = ray_weight (None: 1) and
        acc_r the ray's accumulated opacity (engine.render_loss_masked), on
        every path alike; nothing after the loss kernel changes.  The opacity
        of every ray is then left in ``self.last_acc``.  With the defaults the
        step is the plain one, call for call."""
        losses, _, rgb, reg_out = self._step(rays_o, viewdirs, z_vals, None, None, gt, shape_table, texture_table,
                                             obj_idx, reg, weight_grads, input_grads,
                                             self._mask(ray_weight, acc_target, sil_coef, rays_o))
        return losses, rgb, reg_out

    def forward_backward_fine(self, rays_o, viewdirs, z_c, rand_f, gt, shape_table, texture_table, obj_idx,
                              reg=True, z_f=None, weight_grads=True, input_grads=False, ray_weight=None,
                              acc_target=None, sil_coef=0.0):
        """Coarse + fine image step (the BASELINE configs' "64 + 64"; no
        reference counterpart -- NeRF hierarchical sampling through the one
        CodeNeRF MLP, oracle/ref_cpu.py:fine_image_step).  Loss = coarse
        chunk-mean MSE + fine chunk-mean MSE (+ code regulariser once).  The
        coarse pass fills activation rows [0, pad(R*Nc)), the fine pass the
        rows after, so one backward schedule covers both.
        z_f (R, Nf), optional: fine samples to use instead of sample_pdf's
        (tests replaying one sampling under two precisions); rand_f is then
        only read for Nf.
        weight_grads False (codes-only optimisation at test time): both
        forwards store only what the codes backward reads, one codes backward
        runs over the coarse and fine rows, and the bias sums replace the
        weight-gradient pass; the model's .grad tensors are not written.
        input_grads (pose refinement), on either path: the gradient of both
        losses with respect to every ray is left in ``self.last_ray_grads``
        as in forward_backward; z_f is a constant of it (no gradient through
        sample_pdf, as in NeRF and oracle/ref_cpu.py:fine_image_step).
        ray_weight, acc_target, sil_coef: as in forward_backward, applied to
        the coarse and to the fine loss alike (the fine opacity runs over the
        merged samples); ``self.last_acc`` is the fine loss's.
        Returns (coarse chunk losses, fine chunk losses, fine rgb (R,3), reg)."""
        return self._step(rays_o, viewdirs, z_c, rand_f, z_f, gt, shape_table, texture_table, obj_idx, reg,
                          weight_grads, input_grads, self._mask(ray_weight, acc_target, sil_coef, rays_o))

    @staticmethod
    def _mask(ray_weight, acc_target, sil_coef, rays_o):
        """(ray_weight, acc_target, sil_coef) of a masked step on the rays'
        device, or None for the plain loss."""
        if ray_weight is None and acc_target is None and not sil_coef:
            return None
        R = rays_o.shape[0]
        out = []
        for name, t in (("ray_weight", ray_weight), ("acc_target", acc_target)):
            if t is not None:
                t = t.reshape(-1).to(rays_o.device, torch.float32).contiguous()
                if t.numel() != R:
                    raise ValueError(f"{name} must hold one value per ray ({R}), got {t.numel()}")
            out.append(t)
        return out[0], out[1], float(sil_coef)

    @staticmethod
    def _cat(parts):
        """A single ray part hands back its own tensor: no cat, no copy."""
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def _step(self, rays_o, viewdirs, z_c, rand_f, z_f, gt, shape_table, texture_table, obj_idx, reg, weight_grads,
              input_grads, mask=None):
        """The ray-part loop of both steps (rand_f None: no fine samples) ->
        (coarse losses, fine losses or None, rgb, reg of part 0)."""
        Nf = 0 if rand_f is None else rand_f.shape[-1]
        if self.recompute and Nf and not weight_grads:
            raise ValueError("recompute rebuilds the weight-gradient operands: it has no codes-only form "
                             "(weight_grads=False)")
        eng = self.model.engine()
        z_c = z_c.contiguous().to(eng.device, torch.float32)
        outs = []
        for k, (a, b) in enumerate(self.ray_parts(eng, rays_o.shape[0], z_c.shape[-1] + Nf)):
            outs.append(self._part(eng, rays_o[a:b], viewdirs[a:b], z_c if z_c.dim() == 1 else z_c[a:b],
                                   rand_f[a:b] if Nf else None, None if z_f is None else z_f[a:b].contiguous(),
                                   gt[a:b], shape_table, texture_table, obj_idx, reg and k == 0, weight_grads,
                                   input_grads,
                                   mask and tuple(None if t is None else t[a:b] for t in mask[:2]) + mask[2:]))
        loss_c, loss_f, rgb, regs, z_fs, ray_grads, accs = zip(*outs)
        if mask:
            self.last_acc = self._cat(accs)
        if input_grads:
            self.last_ray_grads = (self._cat([g[0] for g in ray_grads]), self._cat([g[1] for g in ray_grads]))
        if Nf:
            self.last_z_f = self._cat(z_fs)
        return self._cat(loss_c), self._cat(loss_f) if Nf else None, self._cat(rgb), regs[0]

    def _part(self, eng, rays_o, viewdirs, z_c, rand_f, z_f, gt, shape_table, texture_table, obj_idx, reg,
              weight_grads, input_grads, mask=None):
        """One ray part of a step -> (coarse losses, fine losses, rgb, reg,
        fine z, ray gradients, opacity): the fine entries None without fine
        samples (rand_f None; rgb is then the coarse one), the ray gradients
        None without input_grads, the opacity None without mask = (ray
        weights, opacity targets, silhouette coefficient) of the part's rays."""
        params = self.model.param_list()
        grads = self.ensure_grads(params)
        self.ensure_grads([shape_table, texture_table])
        self._writing_grads()
        tm = self.timers
        R = rays_o.shape[0]
        Nc = z_c.shape[-1]
        Nf = 0 if rand_f is None else rand_f.shape[-1]
        Mc, Mf = R * Nc, R * Nf
        Mc_p = eng.pad(Mc)
        M = Mc_p + Mf if Nf else Mc              # rows of the backward: coarse, its padding, fine
        Mp = eng.pad(M)
        ws = self._workspace(eng, M)
        cap, act = ws["cap"], ws["act"]
        sig, rgb, dsig, drgb = ws["sig"], ws["rgb"], ws["dsig"], ws["drgb"]
        self._zero_pad_rows(ws, (Mc, Mf), [(Mc, Mc_p), (Mc_p + Mf, Mp)])
        eng.ensure_packed(params, bwd=True)
        s, t = shape_table.detach()[obj_idx], texture_table.detach()[obj_idx]
        blob, zvec = eng.latent_fwd(params, s, t)

        def timed(name, launch, **done):
            # mark arms the timer of the next hot launch: nothing goes between
            ev = tm.mark(name) if tm else None
            out = launch()
            if tm:
                tm.done(name, ev, **done)
            return out

        # a pass = (samples, z, z stride, samples per ray, first workspace row)
        def fwd(rows, out_sig, out_rgb, codes=False):
            n, z, stride, N, r0 = rows
            return eng.mlp_fwd(blob, n, rays_o=rays_o, rays_d=viewdirs, z=z, z_stride=stride, n_samples=N, act=act,
                               act_M=cap, act_row0=r0, sigma=out_sig[r0:r0 + eng.pad(n)],
                               rgb=out_rgb[r0:r0 + eng.pad(n)], codes=codes)

        def input_grad(rows):
            n, z, stride, N, r0 = rows
            return eng.mlp_input_grad(act, n, rays_o=rays_o, rays_d=viewdirs, z=z, z_stride=stride, n_samples=N,
                                      act_M=cap, row0=r0)[2:]

        # codes-only and recompute (a fine-step option) both store only the codes forward's planes
        rc = bool(self.recompute and Nf) or not weight_grads
        coarse = (Mc, z_c, 0 if z_c.dim() == 1 else Nc, Nc, 0)
        sig_c, rgb_c = timed("fwd", lambda: fwd(coarse, sig, rgb, rc), n=Mc)
        acc = None
        if mask:
            mw, ma, lam = mask
            out_rgb, loss_c, _, _, acc = _eng.render_loss_masked(sig_c, rgb_c, z_c, R, Nc, gt, self.chunk,
                                                                 self.white_bg, dsig=dsig[:Mc], drgb=drgb[:Mc],
                                                                 ray_weight=mw, acc_target=ma, sil_coef=lam)
        else:
            out_rgb, loss_c, _, _ = _eng.render_loss(sig_c, rgb_c, z_c, R, Nc, gt, self.chunk, self.white_bg,
                                                     dsig=dsig[:Mc], drgb=drgb[:Mc])
        loss_f = fine = None
        if Nf:
            if z_f is None:
                z_f = _eng.sample_pdf(sig_c, z_c, R, Nc, rand_f)
            else:
                z_f = z_f.to(eng.device, torch.float32)
            fine = (Mf, z_f, Nf, Nf, Mc_p)
            sig_f, rgb_f = timed("fwd", lambda: fwd(fine, sig, rgb, rc), n=Mf)
            if mask:
                out_rgb, loss_f, acc = _eng.render_loss_fine_masked(
                    sig_c, rgb_c, z_c, Nc, sig_f, rgb_f, z_f, Nf, R, gt, self.chunk, dsig[:Mc], drgb[:Mc],
                    dsig[Mc_p:Mc_p + Mf], drgb[Mc_p:Mc_p + Mf], self.white_bg, ray_weight=mw, acc_target=ma,
                    sil_coef=lam)
            else:
                out_rgb, loss_f = _eng.render_loss_fine(sig_c, rgb_c, z_c, Nc, sig_f, rgb_f, z_f, Nf, R, gt,
                                                        self.chunk, dsig[:Mc], drgb[:Mc], dsig[Mc_p:Mc_p + Mf],
                                                        drgb[Mc_p:Mc_p + Mf], self.white_bg)
            if self.recompute:
                # recompute A/B (hard part 2): the forward passes above
                # stored only ReLU masks + sigma pre-activations; the planes the dW
                # pass reads are produced here by a second training forward
                if ws.get("dsig_tmp") is None or ws["dsig_tmp"].numel() < cap:   # its (discarded) outputs
                    ws["dsig_tmp"] = torch.empty(cap, dtype=torch.float32, device=eng.device)
                    ws["drgb_tmp"] = torch.empty(cap, 3, dtype=torch.float32, device=eng.device)
                timed("fwd", lambda: (fwd(coarse, ws["dsig_tmp"], ws["drgb_tmp"]),
                                      fwd(fine, ws["dsig_tmp"], ws["drgb_tmp"])))
        if weight_grads:
            self._bwd_dw(eng, blob, ws, zvec, eng.table(grads), M)
        else:
            # one codes backward over the coarse rows, the (zero) padding and
            # the fine rows, then the bias sums the code gradients need
            timed("bwd", lambda: eng.mlp_bwd(blob, M, dsig, drgb, act, codes=True, act_M=cap, row0=0,
                                             pose=input_grads), n=M)
            timed("dw", lambda: eng.mlp_dbias(act, M, ws["dbuf"], ws["dw"], act_M=cap), n=M)
            grads = ws.setdefault("scratch_grads", [torch.zeros_like(p) for p in params])
        ray_grads = None
        if input_grads:
            # both backwards left dA of encoding_xyz and of encoding_viewdir in
            # the workspace (the ray direction is also the view direction): the
            # planes of the coarse rows and of the fine rows, each reduced over
            # its own samples; z_f is a constant
            ray_grads = input_grad(coarse)
            if fine:
                d_f = input_grad(fine)
                ray_grads = (ray_grads[0] + d_f[0], ray_grads[1] + d_f[1])
        reg_out = torch.empty(1, dtype=torch.float32, device=eng.device)     # written by cn_latent_bwd
        eng.latent_bwd(params, grads, s, t, zvec, ws["dbuf"], shape_table.grad[obj_idx],
                       texture_table.grad[obj_idx], self.reg_coef if reg else 0.0, reg_out)
        return loss_c, loss_f, out_rgb, reg_out, z_f if Nf else None, ray_grads, acc

    # ------------------------------------------------------------ inference
    @torch.no_grad()
    def render(self, rays_o, viewdirs, z_vals, shape_code, texture_code, occupancy=None):
        """Forward only (src/optimizer.py:108-124): -> rgb (R,3), depth (R,).
        No workspace; images beyond CN_MAX_SAMPLES samples go in ray parts.
        occupancy (an ``occupancy.OccupancyGrid`` built for this shape code; no
        reference counterpart): the MLP is evaluated only at the samples in
        set cells of the grid and at the last sample of every ray; the density
        and colour of every other sample are 0 and nothing else changes
        (DESIGN.md 8.4).  One host synchronisation per pass reads the kept
        count back.  ``self.last_sparse = (kept coarse, kept fine, total)``
        samples of the call.  None: the dense render, call for call."""
        return self._render(rays_o, viewdirs, z_vals, 0, shape_code, texture_code, occupancy=occupancy)

    @torch.no_grad()
    def render_fine(self, rays_o, viewdirs, z_c, n_fine, shape_code, texture_code, rand_f=None, z_f=None,
                    occupancy=None):
        """Forward only through the coarse + fine renderer the fine step
        trains (no reference counterpart): coarse pass -> sample_pdf -> fine
        pass -> composite over the merged samples -> rgb (R,3), depth (R,).
        rand_f None: the deterministic samples u_j = (j + 0.5) / n_fine
        (NeRF's test-time convention; nothing is drawn).  z_f (R, n_fine)
        given: those fine samples, sample_pdf skipped.  The fine z used are
        left in ``self.last_z_f``.  No workspace; ray parts as in render.
        occupancy: as in render, for the coarse pass (last sample kept) and
        the fine pass (grid cells only).  The last coarse sample is also the
        last of the merged ray, because sample_pdf's bins are midpoints of the
        coarse z; a caller-supplied z_f beyond it gives that guarantee up
        (a ray whose last merged sample is culled is not opaque)."""
        return self._render(rays_o, viewdirs, z_c, int(n_fine), shape_code, texture_code, rand_f, z_f, occupancy)

    def _sparse_fwd(self, eng, blob, rays_o, viewdirs, z, n, N, occ, keep_last, out_sig=None, out_rgb=None):
        """The MLP pass of one ray part through the grid: mark -> prefix sum ->
        gather -> MLP on the kept points -> scatter.  -> (sigma (n N,), rgb
        (n N, 3), kept samples); reading the kept count back synchronises.
        out_sig / out_rgb: the planes to scatter into (render_scene's slices)."""
        keep, count = _eng.sparse_mark(rays_o, viewdirs, z, n, N, occ.bits, occ.G, occ.lo, occ.inv_cell, keep_last)
        incl = torch.cumsum(count, 0, dtype=torch.int32)
        Mk = int(incl[-1])                       # cn_mlp_fwd takes its sample count on the host
        if Mk == 0:
            if out_sig is not None:
                return out_sig.zero_(), out_rgb.zero_(), 0
            dev = rays_o.device
            return (torch.zeros(n * N, dtype=torch.float32, device=dev),
                    torch.zeros(n * N, 3, dtype=torch.float32, device=dev), 0)
        off = incl - count
        xyz, vd = _eng.sparse_gather(rays_o, viewdirs, z, n, N, keep, off, Mk)
        sig_k, rgb_k = eng.mlp_fwd(blob, Mk, xyz=xyz, viewdir=vd)
        sig, rgb = _eng.sparse_scatter(keep, off, n, N, sig_k, rgb_k, out_sig, out_rgb)
        return sig, rgb, Mk

    def _render(self, rays_o, viewdirs, z_c, Nf, shape_code, texture_code, rand_f=None, z_f=None, occupancy=None):
        """The ray-part loop of both renderers (Nf 0: no fine pass)."""
        eng = self.model.engine()
        params = self.model.param_list()
        R = rays_o.shape[0]
        Nc = z_c.shape[-1]
        z = z_c.contiguous().to(eng.device, torch.float32)
        if z_f is not None:
            z_f = z_f.contiguous().to(eng.device, torch.float32)
        elif rand_f is not None:
            rand_f = rand_f.contiguous().to(eng.device, torch.float32)
        eng.ensure_packed(params, bwd=False)
        blob, _ = eng.latent_fwd(params, shape_code.reshape(-1).contiguous(), texture_code.reshape(-1).contiguous())
        per = max(1, (eng.L.cn_max_samples() - 256) // max(Nc, Nf))
        zc_stride = 0 if z.dim() == 1 else Nc
        rgbs, depths, zfs = [], [], []
        occ = occupancy
        kept_c = kept_f = 0
        if occ is not None:
            rays_o = rays_o.contiguous().to(eng.device, torch.float32)
            viewdirs = viewdirs.contiguous().to(eng.device, torch.float32)
        for a in range(0, R, per):
            b = min(a + per, R)
            n = b - a
            zp = z if z.dim() == 1 else z[a:b]
            if occ is not None:
                sig_c, rgb_c, k = self._sparse_fwd(eng, blob, rays_o[a:b], viewdirs[a:b], zp, n, Nc, occ, True)
                kept_c += k
            else:
                sig_c, rgb_c = eng.mlp_fwd(blob, n * Nc, rays_o=rays_o[a:b], rays_d=viewdirs[a:b], z=zp,
                                           z_stride=zc_stride, n_samples=Nc)
            if not Nf:
                c, d = _eng.composite_fwd(sig_c, rgb_c, zp, n, Nc, self.white_bg)
            else:
                if z_f is not None:
                    zf = z_f[a:b]
                else:
                    rnd = (torch.full((n, Nf), 0.5, dtype=torch.float32, device=eng.device) if rand_f is None
                           else rand_f[a:b])
                    zf = _eng.sample_pdf(sig_c, zp, n, Nc, rnd)
                if occ is not None:
                    sig_f, rgb_f, k = self._sparse_fwd(eng, blob, rays_o[a:b], viewdirs[a:b], zf, n, Nf, occ, False)
                    kept_f += k
                else:
                    sig_f, rgb_f = eng.mlp_fwd(blob, n * Nf, rays_o=rays_o[a:b], rays_d=viewdirs[a:b], z=zf,
                                               z_stride=Nf, n_samples=Nf)
                c, d = _eng.composite_fine_fwd(sig_c, rgb_c, zp, Nc, sig_f, rgb_f, zf, Nf, n, self.white_bg)
                zfs.append(zf)
            rgbs.append(c)
            depths.append(d)
        if Nf:
            self.last_z_f = self._cat(zfs)
        if occ is not None:
            self.last_sparse = (kept_c, kept_f, R * (Nc + Nf))
        return self._cat(rgbs), self._cat(depths)

    @torch.no_grad()
    def render_scene(self, rays_o, viewdirs, z_c, scene, n_fine=0, rand_f=None, labels=True, acc_min=0.5):
        """Several objects in one picture (``scene.Scene``; no reference
        counterpart) -> dict(rgb (R,3), depth (R,), acc (R,),
        obj_acc (R, K), instance (R,) int32; the last two None without labels).
        Object k sees the world ray from its own frame (engine.scene_rays) at
        the depths z / s_k and is evaluated only at the samples in set cells of
        its grid -- no sample is exempt, so it contributes nothing outside its
        box --; the K planes are combined per sample (engine.scene_combine) and
        the ray is composited as one object's: coarse only, or with n_fine
        samples of sample_pdf on the combined coarse density (rand_f None: the
        deterministic ones), merged.  obj_acc[k] = sum_i w_i f_k,i, the share of
        the ray's opacity that object k holds; instance = the lowest k with the
        largest share where acc >= acc_min, else -1.
        ``self.last_z_f`` and ``self.last_sparse`` as render_fine leaves them,
        the kept counts summed over the objects (total = K R (Nc + Nf)).  One
        host synchronisation per object and pass.  No gradients."""
        eng = self.model.engine()
        params = self.model.param_list()
        dev = eng.device
        objs = scene.objects
        K, R, Nc, Nf = len(objs), rays_o.shape[0], z_c.shape[-1], int(n_fine)
        z = z_c.contiguous().to(dev, torch.float32)
        if rand_f is not None:
            rand_f = rand_f.contiguous().to(dev, torch.float32)
        rays_o = rays_o.contiguous().to(dev, torch.float32)
        viewdirs = viewdirs.contiguous().to(dev, torch.float32)
        eng.ensure_packed(params, bwd=False)
        code = lambda c: c.detach().reshape(-1).to(dev, torch.float32).contiguous()
        blobs = [eng.latent_fwd(params, code(o.shape_code), code(o.texture_code))[0] for o in objs]
        xf, inv_s = scene.transforms(), scene.inv_s()
        per = max(1, (eng.L.cn_max_samples() - 256) // max(Nc, Nf))
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        parts, zfs = [], []
        kept_c = kept_f = 0

        def one_pass(ro_k, rd_k, zz, n, N):
            """The K objects over one set of depths -> (object densities (K, n N),
            combined sigma, combined rgb, kept samples)."""
            sig_k, rgb_k, kept = new(K, n * N), new(K, n * N, 3), 0
            for k, o in enumerate(objs):
                zk = zz if inv_s[k] == 1.0 else zz * inv_s[k]
                kept += self._sparse_fwd(eng, blobs[k], ro_k[k], rd_k[k], zk, n, N, o.grid, False, sig_k[k],
                                         rgb_k[k])[2]
            sig, rgb = _eng.scene_combine(sig_k, rgb_k, inv_s)
            return sig_k, sig, rgb, kept

        for a in range(0, R, per):
            b = min(a + per, R)
            n = b - a
            zp = z if z.dim() == 1 else z[a:b]
            ro_k, rd_k = _eng.scene_rays(rays_o[a:b], viewdirs[a:b], xf)
            obj_c, sig_c, rgb_c, k = one_pass(ro_k, rd_k, zp, n, Nc)
            kept_c += k
            fine = {}
            if Nf:
                rnd = (torch.full((n, Nf), 0.5, dtype=torch.float32, device=dev) if rand_f is None else rand_f[a:b])
                zf = _eng.sample_pdf(sig_c, zp, n, Nc, rnd)
                obj_f, sig_f, rgb_f, k = one_pass(ro_k, rd_k, zf, n, Nf)
                kept_f += k
                fine = dict(sigma_f=sig_f, rgb_f=rgb_f, z_f=zf, Nf=Nf, obj_f=obj_f if labels else None)
                zfs.append(zf)
            parts.append(_eng.scene_composite(sig_c, rgb_c, zp, Nc, n, inv_s, self.white_bg,
                                              obj_c=obj_c if labels else None, labels=labels, acc_min=acc_min,
                                              **fine))
        if Nf:
            self.last_z_f = self._cat(zfs)
        self.last_sparse = (kept_c, kept_f, K * R * (Nc + Nf))
        return {k: None if parts[0][k] is None else self._cat([p[k] for p in parts]) for k in parts[0]}

    def _aov_workspace(self, eng, M):
        """What the normals of render_aov need for M rows (grow-only, per
        device): the activation workspace, the network outputs and the constant
        upstream gradient d sigma = 1, d rgb = 0."""
        ws = self._aov_ws.get(eng.device)
        if ws is None or ws["cap"] < M:
            self._aov_ws.pop(eng.device, None)
            del ws
            cap, dev = eng.pad(M), eng.device
            ws = dict(cap=cap, act=eng.new_act(cap),
                      sig=torch.empty(cap, dtype=torch.float32, device=dev),
                      rgb=torch.empty(cap, 3, dtype=torch.float32, device=dev),
                      dsig=torch.ones(cap, dtype=torch.float32, device=dev),
                      drgb=torch.zeros(cap, 3, dtype=torch.float32, device=dev))
            self._aov_ws[eng.device] = ws
        return ws

    @torch.no_grad()
    def render_aov(self, rays_o, viewdirs, z_c, shape_code, texture_code, n_fine=0, normals=True, rand_f=None,
                   z_f=None):
        """render (n_fine 0) or render_fine with the geometry buffers (no
        reference counterpart) -> dict(rgb (R,3), depth (R,),
        acc (R,), depth_median (R,), normal (R,3) or None): rgb and depth are
        those calls' bit for bit; acc = sum w; depth_median = the z of the first
        sample at which the running weight sum reaches 0.5; normal = sum_k w_k
        u_k with u = -grad(sigma) / |grad(sigma)| per sample, not normalised
        (engine.composite_aov).  rand_f, z_f and ``self.last_z_f``: as in
        render_fine.
        normals: each ray part runs the codes-mode forward in ray mode into a
        workspace (coarse rows, then fine rows, as the steps lay them out) --
        its sigma and rgb are the inference forward's bit for bit
        (tests/test_gpu_aov.py), so it is the part's only forward --, the pose
        backward with d sigma = 1 and d rgb = 0, and the input gradient of the
        coarse and of the fine rows; the parts are then also sized to fit
        engine.ACT_BUDGET.  False: no workspace and no backward."""
        eng = self.model.engine()
        params = self.model.param_list()
        R, Nc, Nf = rays_o.shape[0], z_c.shape[-1], int(n_fine)
        z = z_c.contiguous().to(eng.device, torch.float32)
        if z_f is not None:
            z_f = z_f.contiguous().to(eng.device, torch.float32)
        elif rand_f is not None:
            rand_f = rand_f.contiguous().to(eng.device, torch.float32)
        eng.ensure_packed(params, bwd=bool(normals))
        blob, _ = eng.latent_fwd(params, shape_code.reshape(-1).contiguous(), texture_code.reshape(-1).contiguous())
        per = max(1, (eng.L.cn_max_samples() - 256) // max(Nc, Nf))
        if normals:
            cap = eng.max_act_samples(self.act_budget)
            if (cap - 256) // (Nc + Nf) < 1:
                raise ValueError(f"one ray of {Nc + Nf} samples does not fit the activation budget ({cap} samples): "
                                 "raise CODENERF_ACT_BUDGET")
            per = min(per, (cap - 256) // (Nc + Nf))
        zc_stride = 0 if z.dim() == 1 else Nc
        parts, zfs = [], []
        for a in range(0, R, per):
            b = min(a + per, R)
            n = b - a
            ro, vd = rays_o[a:b], viewdirs[a:b]
            zp = z if z.dim() == 1 else z[a:b]
            Mc, Mf = n * Nc, n * Nf
            Mc_p = eng.pad(Mc)
            ws = self._aov_workspace(eng, Mc_p + Mf if Nf else Mc) if normals else None

            def fwd(m, zz, stride, N, r0):
                if ws is None:
                    return eng.mlp_fwd(blob, m, rays_o=ro, rays_d=vd, z=zz, z_stride=stride, n_samples=N)
                rows = slice(r0, r0 + eng.pad(m))
                return eng.mlp_fwd(blob, m, rays_o=ro, rays_d=vd, z=zz, z_stride=stride, n_samples=N, act=ws["act"],
                                   act_M=ws["cap"], act_row0=r0, sigma=ws["sig"][rows], rgb=ws["rgb"][rows],
                                   codes=True)

            def grad(m, zz, stride, N, r0):
                return eng.mlp_input_grad(ws["act"], m, rays_o=ro, rays_d=vd, z=zz, z_stride=stride, n_samples=N,
                                          act_M=ws["cap"], row0=r0, per_ray=False)[0]

            sig_c, rgb_c = fwd(Mc, zp, zc_stride, Nc, 0)
            fine = {}
            if Nf:
                if z_f is not None:
                    zf = z_f[a:b]
                else:
                    rnd = (torch.full((n, Nf), 0.5, dtype=torch.float32, device=eng.device) if rand_f is None
                           else rand_f[a:b])
                    zf = _eng.sample_pdf(sig_c, zp, n, Nc, rnd)
                sig_f, rgb_f = fwd(Mf, zf, Nf, Nf, Mc_p)
                fine = dict(sigma_f=sig_f, rgb_f=rgb_f, z_f=zf, Nf=Nf)
                zfs.append(zf)
            if normals:
                # one pose backward over the coarse rows, the padding and the fine rows
                eng.mlp_bwd(blob, Mc_p + Mf if Nf else Mc, ws["dsig"], ws["drgb"], ws["act"], act_M=ws["cap"],
                            row0=0, pose=True)
                fine.update(grad_c=grad(Mc, zp, zc_stride, Nc, 0))
                if Nf:
                    fine.update(grad_f=grad(Mf, zf, Nf, Nf, Mc_p))
            parts.append(_eng.composite_aov(sig_c, rgb_c, zp, Nc, n, self.white_bg, **fine))
        if Nf:
            self.last_z_f = self._cat(zfs)
        return {k: None if parts[0][k] is None else self._cat([p[k] for p in parts]) for k in parts[0]}

    @torch.no_grad()
    def render_sharded(self, rays_o, viewdirs, z_vals, shape_code, texture_code, dist=None, group=None):
        """One image rendered by all ranks (C5 inference):
        rank r renders the contiguous ray block dp.ray_block(R, r) and the
        blocks are all-gathered -> rgb (R,3), depth (R,) on every rank."""
        R = rays_o.shape[0]
        a, b = _dp.ray_block(R, dist, group)
        z = z_vals if z_vals.dim() == 1 else z_vals[a:b]
        if b > a:
            rgb, depth = self.render(rays_o[a:b], viewdirs[a:b], z, shape_code, texture_code)
        else:
            rgb = torch.empty(0, 3, dtype=torch.float32, device=rays_o.device)
            depth = torch.empty(0, dtype=torch.float32, device=rays_o.device)
        return _dp.gather_ray_blocks(rgb, R, dist, group), _dp.gather_ray_blocks(depth, R, dist, group)
