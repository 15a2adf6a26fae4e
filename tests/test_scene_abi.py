"""CPU: the C ABI of the scene entries (cn_scene_rays, cn_scene_combine,
cn_scene_composite): exported, bound with the documented signatures, additive
to ABI 4, and every host check refuses with -1 and a message that starts with
the entry's name before anything is launched.  The device pointers below are
never dereferenced; the host arrays (h_xf, h_inv_s) are real, as the entries
read them at the call."""
import ctypes
import os

import pytest

D = ctypes.c_void_p(256)
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGS = {
    "cn_scene_rays": [P, P, I, P, I, P, P, P],
    "cn_scene_combine": [P, P, P, I, I, P, P, P],
    "cn_scene_composite": [P, P, P, I, I, P, P, P, I, P, P, P, I, I, I, F, P, P, P, P, P, P],
}
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]
BAD_INV_S = (0.0, -1.0, float("inf"), float("nan"))


def _lib():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load_library()


def _host(vals):
    a = (ctypes.c_float * len(vals))(*vals)
    return a, ctypes.cast(a, ctypes.c_void_p)


def test_the_symbols_are_exported_and_bound():
    L, lib = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "codenerf.h")).read()
    from codenerf_amd import engine
    for name, want in SIGS.items():
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == L._SIGS[name][1] == want
        assert f"int {name}(" in header
        assert callable(getattr(engine, name[3:]))
    assert L.ABI_VERSION == 4 and lib.cn_abi_version() == 4
    assert "#define CN_ABI_VERSION 4" in header


def _refused(lib, entry, rc, what):
    assert rc == -1, what
    err = lib.cn_last_error()
    assert err.startswith(entry.encode() + b":") and what in err, (what, err)


# ------------------------------------------------------------------ rays
def _rays(lib, ro=D, rd=D, R=4, xf=IDENTITY, K=1, out_o=D, out_d=D, null_xf=False):
    keep, h = _host(list(xf))
    return lib.cn_scene_rays(ro, rd, R, None if null_xf else h, K, out_o, out_d, None)


def test_rays_refusals():
    _, lib = _lib()
    e = "cn_scene_rays"
    for k in ("ro", "rd", "out_o", "out_d"):
        _refused(lib, e, _rays(lib, **{k: None}), b"NULL argument")
    _refused(lib, e, _rays(lib, null_xf=True), b"NULL argument")
    for K in (0, -1, 9):
        _refused(lib, e, _rays(lib, K=K, xf=IDENTITY * 9), b"K must be in [1, 8]")
    for R in (0, -5):
        _refused(lib, e, _rays(lib, R=R), b"R must be at least 1")
    _refused(lib, e, _rays(lib, R=lib.cn_max_samples() + 1), b"exceed CN_MAX_SAMPLES")
    for bad in BAD_INV_S:
        _refused(lib, e, _rays(lib, xf=IDENTITY[:12] + [bad]), b"1/s must be finite and positive")
        _refused(lib, e, _rays(lib, K=3, xf=IDENTITY * 2 + IDENTITY[:12] + [bad]), b"1/s must be finite and positive")
    for i in (0, 8, 9, 11):
        xf = list(IDENTITY)
        xf[i] = float("nan")
        _refused(lib, e, _rays(lib, xf=xf), b"must be finite")


# ------------------------------------------------------------------ combine
def _combine(lib, sig_k=D, rgb_k=D, inv_s=(1.0,), K=1, M=64, sig=D, rgb=D, null_inv_s=False):
    keep, h = _host(list(inv_s))
    return lib.cn_scene_combine(sig_k, rgb_k, None if null_inv_s else h, K, M, sig, rgb, None)


def test_combine_refusals():
    _, lib = _lib()
    e = "cn_scene_combine"
    for k in ("sig_k", "rgb_k", "sig", "rgb"):
        _refused(lib, e, _combine(lib, **{k: None}), b"NULL argument")
    _refused(lib, e, _combine(lib, null_inv_s=True), b"NULL argument")
    for K in (0, -1, 9):
        _refused(lib, e, _combine(lib, K=K, inv_s=[1.0] * 9), b"K must be in [1, 8]")
    for M in (0, -1):
        _refused(lib, e, _combine(lib, M=M), b"M must be positive")
    _refused(lib, e, _combine(lib, M=lib.cn_max_samples() + 1), b"exceed CN_MAX_SAMPLES")
    for bad in BAD_INV_S:
        _refused(lib, e, _combine(lib, inv_s=[bad]), b"1/s must be finite and positive")
        _refused(lib, e, _combine(lib, K=8, inv_s=[1.0] * 7 + [bad]), b"1/s must be finite and positive")


# ------------------------------------------------------------------ composite
def _composite(lib, sig_c=D, rgb_c=D, z_c=D, zc_stride=0, Nc=64, sig_f=None, rgb_f=None, z_f=None, Nf=0, obj_c=D,
               obj_f=None, inv_s=(1.0, 0.5), K=2, R=4, acc_min=0.5, out_rgb=D, out_depth=D, out_acc=D, obj_acc=D,
               instance=D, null_inv_s=False):
    keep, h = _host(list(inv_s))
    return lib.cn_scene_composite(sig_c, rgb_c, z_c, zc_stride, Nc, sig_f, rgb_f, z_f, Nf, obj_c, obj_f,
                                  None if null_inv_s else h, K, R, 1, acc_min, out_rgb, out_depth, out_acc, obj_acc,
                                  instance, None)


FINE = dict(sig_f=D, rgb_f=D, z_f=D, obj_f=D, Nf=64)
E = "cn_scene_composite"


def test_composite_null_required_pointers():
    _, lib = _lib()
    for k in ("sig_c", "rgb_c", "z_c", "out_rgb", "out_depth", "out_acc"):
        _refused(lib, E, _composite(lib, **{k: None}), b"NULL argument")
        _refused(lib, E, _composite(lib, **{k: None}, **FINE), b"NULL argument")
    _refused(lib, E, _composite(lib, null_inv_s=True), b"NULL argument")


def test_composite_counts():
    _, lib = _lib()
    for K in (0, -1, 9):
        _refused(lib, E, _composite(lib, K=K, inv_s=[1.0] * 9), b"K must be in [1, 8]")
    for Nc in (0, -1):
        _refused(lib, E, _composite(lib, Nc=Nc), b"Nc must be at least 1 and Nf at least 0")
    _refused(lib, E, _composite(lib, Nf=-1), b"Nc must be at least 1 and Nf at least 0")
    _refused(lib, E, _composite(lib, Nc=257), b"at most 256 samples per ray")
    _refused(lib, E, _composite(lib, **dict(FINE, Nc=129, Nf=128)), b"at most 256 samples per ray")
    _refused(lib, E, _composite(lib, **dict(FINE, Nc=2 ** 31 - 1, Nf=2 ** 31 - 1)), b"at most 256 samples per ray")
    for stride in (1, 63, 65, -64):
        _refused(lib, E, _composite(lib, zc_stride=stride), b"zc_stride must be 0 or Nc")
        _refused(lib, E, _composite(lib, zc_stride=stride, **FINE), b"zc_stride must be 0 or Nc")
    for R in (0, -3):
        _refused(lib, E, _composite(lib, R=R), b"R and N must be positive")
    big = lib.cn_max_samples() // 64 + 1
    _refused(lib, E, _composite(lib, R=big), b"exceed CN_MAX_SAMPLES")
    _refused(lib, E, _composite(lib, **dict(FINE, Nc=32, Nf=32, R=big)), b"exceed CN_MAX_SAMPLES")


def test_composite_fine_pointers_go_with_nf():
    _, lib = _lib()
    for k in ("sig_f", "rgb_f", "z_f"):
        _refused(lib, E, _composite(lib, **dict(FINE, **{k: None})), b"Nf > 0 needs d_sigma_f, d_rgb_f and d_z_f")
        _refused(lib, E, _composite(lib, **{k: D}), b"Nf == 0 takes no fine pointer")
    _refused(lib, E, _composite(lib, obj_f=D), b"Nf == 0 takes no fine pointer")


def test_composite_labels_go_together_and_need_the_object_planes():
    _, lib = _lib()
    both = b"d_obj_acc and d_instance go together"
    for kw in (dict(obj_acc=None), dict(instance=None)):
        _refused(lib, E, _composite(lib, **kw), both)
        _refused(lib, E, _composite(lib, **kw, **FINE), both)
    need = b"the labels need d_obj_c (and d_obj_f when Nf > 0)"
    _refused(lib, E, _composite(lib, obj_c=None), need)
    _refused(lib, E, _composite(lib, **dict(FINE, obj_c=None)), need)
    _refused(lib, E, _composite(lib, **dict(FINE, obj_f=None)), need)


def test_composite_scales_and_threshold():
    _, lib = _lib()
    for bad in BAD_INV_S:
        _refused(lib, E, _composite(lib, inv_s=[1.0, bad]), b"1/s must be finite and positive")
        _refused(lib, E, _composite(lib, inv_s=[bad, 1.0], obj_acc=None, instance=None, obj_c=None),
                 b"1/s must be finite and positive")
    _refused(lib, E, _composite(lib, acc_min=float("nan")), b"acc_min is NaN")
