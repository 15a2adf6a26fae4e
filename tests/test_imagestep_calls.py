"""CPU: the host schedule of render.ImageStep, call by call.

ImageStep is run end to end on CPU tensors against a recording fake of
``engine.Engine`` and of the module-level ``engine.*`` launchers it calls (the
loss, sampling and compositing kernels).  Every call is logged with its name,
its integer / float / bool arguments and, for a tensor argument, which buffer
it is a view of (a workspace buffer of ``step._ws`` or a named input), its
element offset and its length; a fake ``timers`` logs ``mark`` / ``done`` into
the same list, so where a timer is armed relative to the launches is part of
the record.  ``overlap_dw`` is off: the two-stream schedule of ``_bwd_dw``
needs a device.

The traces are compared, exactly (they hold counts and offsets), with
tests/golden/imagestep_calls.json, which ``python tests/test_imagestep_calls.py``
records.  The fixture is recorded at the commit *before* a change to the
schedule and kept while that change is made: it is what lets a restructuring
of the step be checked without a device.

Shapes: R = 8 rays, Nc = 8, Nf = 4, loss chunk 4 -- 64 coarse rows padded to
256, 32 fine rows behind them, 512 rows in all; two ray parts through
max_rays = 4 (training) or a small CN_MAX_SAMPLES (inference).
"""
import contextlib
import inspect
import itertools
import json
import os
import sys
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":          # under pytest conftest.py has done this
    sys.path.insert(0, REPO)

from codenerf_amd import engine as E  # noqa: E402
from codenerf_amd.render import ImageStep  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "imagestep_calls.json")
R, NC, NF, CHUNK = 8, 8, 4, 4
OBJ = 1
WS_KEYS = ("act", "dw", "dbuf", "sig", "rgb", "dsig", "drgb", "dsig_tmp", "drgb_tmp")
MODULE_FAKES = ("render_loss", "render_loss_fine", "sample_pdf", "composite_fwd", "composite_fine_fwd")


def _pad(M):
    return (M + 255) // 256 * 256


class Table:
    """What the fake Engine.table returns: remembers which tensors it lists."""

    def __init__(self, kind):
        self.kind = kind


class Recorder:
    def __init__(self):
        self.log = []            # the trace
        self.outs = []           # (call name, what the fake returned), in call order
        self.named = {}          # storage pointer -> name of an input buffer
        self.params = []
        self.step = None
        self._n = 0

    def name(self, label, t):
        self.named[t.untyped_storage().data_ptr()] = label
        return t

    def fresh(self, *shape):
        """A new output tensor; every one holds a value of its own."""
        self._n += 1
        return torch.full(shape, float(self._n), dtype=torch.float32)

    def _buffers(self):
        bufs = dict(self.named)
        for ws in self.step._ws.values():
            for k in WS_KEYS:
                if ws.get(k) is not None:
                    bufs[ws[k].untyped_storage().data_ptr()] = k
        return bufs

    def _list_kind(self, v):
        if len(v) == len(self.params):
            if all(a is p for a, p in zip(v, self.params)):
                return "params"
            if all(a is p.grad for a, p in zip(v, self.params)):
                return "model_grads"
        if any(v is ws.get("scratch_grads") for ws in self.step._ws.values()):
            return "scratch_grads"
        return None

    def desc(self, v, bufs):
        if v is None or isinstance(v, (bool, int, float)):
            return v
        if isinstance(v, torch.Tensor):
            label = bufs.get(v.untyped_storage().data_ptr())
            return [label, v.storage_offset(), v.numel()] if label else ["new", list(v.shape)]
        if isinstance(v, Table):
            return ["table", v.kind]
        if isinstance(v, (list, tuple)):
            return self._list_kind(v) or [self.desc(x, bufs) for x in v]
        raise TypeError(f"unexpected argument {v!r}")

    def outputs(self, name):
        return [o for n, o in self.outs if n == name]


def recorded(fn):
    """Log a fake's call (arguments bound to the real signature, defaults
    applied, so positional / keyword / omitted-default spellings agree)."""
    sig = inspect.signature(fn)

    def wrap(self, *a, **k):
        b = sig.bind(self, *a, **k)
        b.apply_defaults()
        rec = self.rec
        bufs = rec._buffers()
        rec.log.append([fn.__name__, {n: rec.desc(v, bufs) for n, v in list(b.arguments.items())[1:]}])
        out = fn(self, *a, **k)
        rec.outs.append((fn.__name__, out))
        return out
    return wrap


class FakeEngine:
    """engine.Engine's launch methods with its signatures; nothing computes."""
    device = torch.device("cpu")
    n_inject = 2

    def __init__(self, rec, max_samples):
        self.rec = rec
        self.L = types.SimpleNamespace(cn_max_samples=lambda: max_samples)

    def pad(self, M):
        return _pad(M)

    def new_act(self, M):
        return torch.empty(4 * M, dtype=torch.uint8)

    def dw_ws_bytes(self, M):
        return 64

    def max_act_samples(self, budget=None):
        return 1 << 20

    def table(self, tensors):
        return Table(self.rec._list_kind(tensors))

    @recorded
    def ensure_packed(self, params, bwd=True):
        pass

    @recorded
    def latent_fwd(self, params, shape_code, texture_code):
        return self.rec.fresh(4), self.rec.fresh(self.n_inject, 256)

    @recorded
    def mlp_fwd(self, blob, M, xyz=None, viewdir=None, rays_o=None, rays_d=None, z=None, z_stride=0,
                n_samples=0, act=None, act_M=0, act_row0=0, sigma=None, rgb=None, codes=False):
        Mp = _pad(M)
        sigma = self.rec.fresh(Mp) if sigma is None else sigma
        rgb = self.rec.fresh(Mp, 3) if rgb is None else rgb
        assert sigma.numel() >= Mp and rgb.numel() >= 3 * Mp
        return sigma, rgb

    @recorded
    def mlp_bwd(self, blob, M, dsigma, drgb, act, codes=False, act_M=0, row0=0, pose=False):
        pass

    @recorded
    def mlp_input_grad(self, act, M, xyz=None, viewdir=None, rays_o=None, rays_d=None, z=None, z_stride=0,
                       n_samples=0, act_M=0, row0=0, params=None, per_ray=True):
        Mp, n = _pad(M), M // max(1, int(n_samples))
        return self.rec.fresh(Mp, 3), self.rec.fresh(Mp, 3), self.rec.fresh(n, 3), self.rec.fresh(n, 3)

    @recorded
    def mlp_dw(self, act, M, zvec, grads, dbuf, ws=None, act_M=0, row0=0, db_accum=False, nwg=0, params=None):
        pass

    @recorded
    def mlp_dbias(self, act, M, dbuf, ws=None, act_M=0):
        pass

    @recorded
    def latent_bwd(self, params, grads, shape_code, texture_code, zvec, dbuf, d_shape, d_tex, reg_coef=0.0,
                   reg_out=None):
        pass


class FakeKernels:
    """The module-level launchers of engine.py; the loss kernels write nothing."""

    def __init__(self, rec):
        self.rec = rec

    @recorded
    def render_loss(self, sigma, rgb, z, R, N, gt, chunk, white_bg=True, dsig=None, drgb=None):
        return self.rec.fresh(R, 3), self.rec.fresh((R + chunk - 1) // chunk), dsig, drgb

    @recorded
    def sample_pdf(self, sigma_c, z_c, R, Nc, rand):
        return self.rec.fresh(R, rand.shape[-1])

    @recorded
    def render_loss_fine(self, sigma_c, rgb_c, z_c, Nc, sigma_f, rgb_f, z_f, Nf, R, gt, chunk, dsig_c, drgb_c,
                         dsig_f, drgb_f, white_bg=True):
        return self.rec.fresh(R, 3), self.rec.fresh((R + chunk - 1) // chunk)

    @recorded
    def composite_fwd(self, sigma, rgb, z, R, N, white_bg=True, weights=None):
        return self.rec.fresh(R, 3), self.rec.fresh(R)

    @recorded
    def composite_fine_fwd(self, sigma_c, rgb_c, z_c, Nc, sigma_f, rgb_f, z_f, Nf, R, white_bg=True, acc=False):
        return self.rec.fresh(R, 3), self.rec.fresh(R)


class FakeTimers:
    def __init__(self, rec):
        self.rec = rec

    def mark(self, name):
        self.rec.log.append(["mark", name])
        return len(self.rec.log) - 1

    def done(self, name, s, n=0, contended=False):
        assert self.rec.log[s] == ["mark", name]
        self.rec.log.append(["done", name, {"mark": s, "n": n, "contended": contended}])


@contextlib.contextmanager
def patched(fk):
    old = {n: getattr(E, n) for n in MODULE_FAKES}
    try:
        for n in MODULE_FAKES:
            setattr(E, n, getattr(fk, n))
        yield
    finally:
        for n, f in old.items():
            setattr(E, n, f)


class Rig:
    """One ImageStep over the fakes, with named inputs."""

    def __init__(self, parts=1, timers=True, max_samples=1 << 20):
        rec = self.rec = Recorder()
        rec.params = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(5))]
        for i, p in enumerate(rec.params):
            rec.name(f"p{i}", p)
            p.grad = rec.name(f"p{i}.grad", torch.zeros_like(p))
        self.eng = FakeEngine(rec, max_samples)
        model = types.SimpleNamespace(engine=lambda: self.eng, param_list=lambda: rec.params)
        self.step = rec.step = ImageStep(model, chunk=CHUNK, timers=FakeTimers(rec) if timers else None,
                                         overlap_dw=False, max_rays=4 if parts == 2 else None)
        self.kernels = FakeKernels(rec)
        self.ro = rec.name("rays_o", torch.zeros(R, 3))
        self.vd = rec.name("viewdirs", torch.zeros(R, 3))
        self.gt = rec.name("gt", torch.zeros(R, 3))
        self.rand_f = rec.name("rand_f", torch.zeros(R, NF))
        self.z_f = rec.name("z_f", torch.zeros(R, NF))
        self.z = {1: rec.name("z1", torch.zeros(NC)), 2: rec.name("z2", torch.zeros(R, NC))}
        self.tables = []
        for n in ("shape", "texture"):
            t = rec.name(n, torch.nn.Parameter(torch.zeros(3, 4)))
            t.grad = rec.name(n + ".grad", torch.zeros(3, 4))
            self.tables.append(t)

    def train(self, fine, wg=True, ig=False, zdim=1, zf=False):
        with patched(self.kernels):
            if fine:
                return self.step.forward_backward_fine(self.ro, self.vd, self.z[zdim], self.rand_f, self.gt,
                                                       *self.tables, OBJ, z_f=self.z_f if zf else None,
                                                       weight_grads=wg, input_grads=ig)
            return self.step.forward_backward(self.ro, self.vd, self.z[zdim], self.gt, *self.tables, OBJ,
                                              weight_grads=wg, input_grads=ig)

    def render(self, fine, zdim=1, fine_in=None):
        s, t = self.tables[0].detach()[OBJ], self.tables[1].detach()[OBJ]
        with patched(self.kernels):
            if fine:
                return self.step.render_fine(self.ro, self.vd, self.z[zdim], NF, s, t,
                                             rand_f=self.rand_f if fine_in == "rand" else None,
                                             z_f=self.z_f if fine_in == "zf" else None)
            return self.step.render(self.ro, self.vd, self.z[zdim], s, t)


# ------------------------------------------------------------------ cases
def _train_cases():
    cases = {}
    for fine, wg, ig, parts, zdim in itertools.product((False, True), (True, False), (False, True), (1, 2), (1, 2)):
        cases[f"{'fine' if fine else 'coarse'}-wg{int(wg)}-ig{int(ig)}-p{parts}-z{zdim}"] = dict(
            fine=fine, wg=wg, ig=ig, parts=parts, zdim=zdim)
    for parts, zdim in itertools.product((1, 2), (1, 2)):
        cases[f"fine-zf-p{parts}-z{zdim}"] = dict(fine=True, wg=True, ig=True, parts=parts, zdim=zdim, zf=True)
    for ig, parts in itertools.product((False, True), (1, 2)):
        cases[f"fine-recompute-ig{int(ig)}-p{parts}"] = dict(fine=True, wg=True, ig=ig, parts=parts, zdim=1,
                                                             recompute=True)
    return cases


def _render_cases():
    cases = {}
    for parts, zdim in itertools.product((1, 2), (1, 2)):
        cases[f"render-p{parts}-z{zdim}"] = dict(fine=False, parts=parts, zdim=zdim)
        for fine_in in (None, "rand", "zf"):
            cases[f"render_fine-{fine_in or 'det'}-p{parts}-z{zdim}"] = dict(fine=True, parts=parts, zdim=zdim,
                                                                             fine_in=fine_in)
    return cases


TRAIN, RENDER = _train_cases(), _render_cases()


def run_train(c, timers=True):
    rig = Rig(c["parts"], timers)
    rig.step.recompute = c.get("recompute", False)
    out = rig.train(c["fine"], c["wg"], c["ig"], c["zdim"], c.get("zf", False))
    return rig, out


def run_render(c):
    # 8 samples per ray: a CN_MAX_SAMPLES of 256 + 4 x 8 makes two parts of 4 rays
    rig = Rig(max_samples=(256 + 4 * NC) if c["parts"] == 2 else 1 << 20)
    out = rig.render(c["fine"], c["zdim"], c.get("fine_in"))
    return rig, out


def record():
    traces = {k: run_train(c)[0].rec.log for k, c in TRAIN.items()}
    traces.update({k: run_render(c)[0].rec.log for k, c in RENDER.items()})
    return traces


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _plain(trace):
    return json.loads(json.dumps(trace))


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", list(TRAIN))
def test_training_step_calls(name, golden):
    c = TRAIN[name]
    rig, out = run_train(c)
    rec, step = rig.rec, rig.step
    assert _plain(rec.log) == golden[name]

    # without timers: the same launches
    quiet, _ = run_train(c, timers=False)
    assert quiet.rec.log == [e for e in rec.log if e[0] not in ("mark", "done")]

    fine, parts = c["fine"], c["parts"]
    nchunk = R // CHUNK
    assert len(out) == (4 if fine else 3)
    losses = out[:2] if fine else out[:1]
    rgb, reg = out[-2], out[-1]
    assert all(tuple(l.shape) == (nchunk,) for l in losses)
    assert tuple(rgb.shape) == (R, 3) and tuple(reg.shape) == (1,)

    lc = [o[1] for o in rec.outputs("render_loss")]
    rgb_parts = [o[0] for o in rec.outputs("render_loss_fine" if fine else "render_loss")]
    lf = [o[1] for o in rec.outputs("render_loss_fine")]
    zf_parts = [o for o in rec.outputs("sample_pdf")]
    assert len(lc) == parts
    if parts == 1:
        # the part's own tensors: no cat, no copy
        assert losses[0] is lc[0] and rgb is rgb_parts[0]
        if fine:
            assert losses[1] is lf[0]
    else:
        assert torch.equal(losses[0], torch.cat(lc)) and torch.equal(rgb, torch.cat(rgb_parts))
        if fine:
            assert torch.equal(losses[1], torch.cat(lf))

    if not fine:
        assert step.last_z_f is None
    else:
        assert tuple(step.last_z_f.shape) == (R, NF)
        if c.get("zf"):
            assert not zf_parts and torch.equal(step.last_z_f, rig.z_f)
            if parts == 1:
                assert step.last_z_f.data_ptr() == rig.z_f.data_ptr()
        elif parts == 1:
            assert step.last_z_f is zf_parts[0]
        else:
            assert torch.equal(step.last_z_f, torch.cat(zf_parts))

    if not c["ig"]:
        assert step.last_ray_grads is None
    else:
        d_ro, d_rd = step.last_ray_grads
        assert tuple(d_ro.shape) == (R, 3) and tuple(d_rd.shape) == (R, 3)
        ig = rec.outputs("mlp_input_grad")
        if fine:                                # per part: the coarse rows' plus the fine rows'
            assert len(ig) == 2 * parts
            ig = [(None, None, c_[2] + f_[2], c_[3] + f_[3]) for c_, f_ in zip(ig[0::2], ig[1::2])]
        elif parts == 1:
            assert d_ro is ig[0][2] and d_rd is ig[0][3]
        assert len(ig) == parts
        assert torch.equal(d_ro, torch.cat([g[2] for g in ig])) and torch.equal(d_rd, torch.cat([g[3] for g in ig]))

    # weight_grads False: the model's .grad tensors are not handed to any launch
    grads_seen = {e[1]["grads"] if e[0] == "latent_bwd" else e[1]["grads"][1]
                  for e in rec.log if e[0] in ("latent_bwd", "mlp_dw")}
    assert grads_seen == ({"model_grads"} if c["wg"] else {"scratch_grads"})


@pytest.mark.parametrize("parts", [1, 2])
def test_coarse_step_ignores_recompute(parts, golden):
    c = dict(TRAIN[f"coarse-wg1-ig0-p{parts}-z1"], recompute=True)
    assert _plain(run_train(c)[0].rec.log) == golden[f"coarse-wg1-ig0-p{parts}-z1"]
    c = dict(TRAIN[f"coarse-wg0-ig1-p{parts}-z1"], recompute=True)
    assert _plain(run_train(c)[0].rec.log) == golden[f"coarse-wg0-ig1-p{parts}-z1"]


@pytest.mark.parametrize("parts", [1, 2])
def test_fine_recompute_has_no_codes_only_form(parts):
    rig = Rig(parts)
    rig.step.recompute = True
    with pytest.raises(ValueError):
        rig.train(True, wg=False)
    assert rig.rec.log == []                    # raised before anything was launched


@pytest.mark.parametrize("name", list(RENDER))
def test_render_calls(name, golden):
    c = RENDER[name]
    rig, (rgb, depth) = run_render(c)
    rec, step = rig.rec, rig.step
    assert _plain(rec.log) == golden[name]
    assert tuple(rgb.shape) == (R, 3) and tuple(depth.shape) == (R,)
    outs = rec.outputs("composite_fine_fwd" if c["fine"] else "composite_fwd")
    assert len(outs) == c["parts"]
    if c["parts"] == 1:
        assert rgb is outs[0][0] and depth is outs[0][1]
    else:
        assert torch.equal(rgb, torch.cat([o[0] for o in outs]))
        assert torch.equal(depth, torch.cat([o[1] for o in outs]))
    if not c["fine"]:
        assert step.last_z_f is None
        return
    assert tuple(step.last_z_f.shape) == (R, NF)
    zfs = rec.outputs("sample_pdf")
    if c["fine_in"] == "zf":
        assert not zfs and torch.equal(step.last_z_f, rig.z_f)
    elif c["parts"] == 1:
        assert step.last_z_f is zfs[0]
    else:
        assert torch.equal(step.last_z_f, torch.cat(zfs))


def test_padding_rows_zeroed_when_the_layout_changes():
    """dsig / drgb rows [Mc, pad(Mc)) and [pad(Mc) + Mf, pad(M)) are zeroed on a
    change of row layout (a switch between the coarse and the fine step on one
    ImageStep included) and left alone otherwise."""
    rig = Rig()
    Mc, Mf = R * NC, R * NF
    Mc_p = _pad(Mc)
    cap = _pad(Mc_p + Mf)
    ws = rig.step._workspace(rig.eng, cap)      # the fine step's rows: never regrown below
    pads = {False: [(Mc, Mc_p)], True: [(Mc, Mc_p), (Mc_p + Mf, cap)]}

    def run(fine, zeroed):
        ws["dsig"].fill_(float("nan"))
        ws["drgb"].fill_(float("nan"))
        rig.train(fine)
        assert rig.step._ws[rig.eng.device] is ws
        want = torch.zeros(cap, dtype=torch.bool)
        for a, b in zeroed:
            want[a:b] = True
        for buf in (ws["dsig"], ws["drgb"].reshape(cap, 3)[:, 0], ws["drgb"].reshape(cap, 3)[:, 2]):
            assert torch.equal(buf == 0, want)
            assert torch.equal(torch.isnan(buf), ~want)

    for fine in (False, True, False):
        run(fine, pads[fine])
    run(False, [])                              # unchanged layout: nothing re-zeroed
    run(True, pads[True])
    run(True, [])


if __name__ == "__main__":
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: it is recorded before a change to the schedule and kept; "
                 "remove it to record the current schedule")
    rows = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in record().items())
    with open(FIXTURE, "w") as f:
        f.write("{\n" + rows + "\n}\n")
    print(f"wrote {FIXTURE}")
