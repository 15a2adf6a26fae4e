"""CPU: the C ABI of the geometry buffers (cn_composite_aov): exported, bound
with the documented signature, additive to ABI 4, and every host check refuses
with -1 and a message that starts with the entry's name before anything is
launched (the pointers below are never dereferenced)."""
import ctypes
import os

import pytest

D = ctypes.c_void_p(256)
ENTRY = "cn_composite_aov"


def _lib():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load_library()


def test_the_symbol_is_exported_and_bound():
    L, lib = _lib()
    P, I = ctypes.c_void_p, ctypes.c_int
    want = [P, P, P, I, I, P, P, P, P, I, P, I, I, P, P, P, P, P, P]
    assert ENTRY in L.EXPORTED
    fn = getattr(lib, ENTRY)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == L._SIGS[ENTRY][1] == want
    assert L.ABI_VERSION == 4 and lib.cn_abi_version() == 4
    from codenerf_amd import engine
    assert callable(engine.composite_aov)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "codenerf.h")).read()
    assert "int cn_composite_aov(" in header


def _call(lib, sig_c=D, rgb_c=D, z_c=D, zc_stride=0, Nc=64, grad_c=None, sig_f=None, rgb_f=None, z_f=None, Nf=0,
          grad_f=None, R=4, out_rgb=D, out_depth=D, out_acc=D, out_med=D, out_normal=None):
    return lib.cn_composite_aov(sig_c, rgb_c, z_c, zc_stride, Nc, grad_c, sig_f, rgb_f, z_f, Nf, grad_f, R, 1,
                                out_rgb, out_depth, out_acc, out_med, out_normal, None)


FINE = dict(sig_f=D, rgb_f=D, z_f=D, Nf=64)


def _refused(lib, what, **kw):
    assert _call(lib, **kw) == -1, kw
    err = lib.cn_last_error()
    assert err.startswith(ENTRY.encode() + b":") and what in err, (kw, err)


def test_null_required_pointers():
    _, lib = _lib()
    for k in ("sig_c", "rgb_c", "z_c", "out_rgb", "out_depth"):
        _refused(lib, b"NULL argument", **{k: None})
        _refused(lib, b"NULL argument", **{k: None}, **FINE)


def test_sample_counts():
    _, lib = _lib()
    for Nc in (0, -1):
        _refused(lib, b"Nc must be at least 1 and Nf at least 0", Nc=Nc)
    _refused(lib, b"Nc must be at least 1 and Nf at least 0", Nf=-1)
    _refused(lib, b"at most 256 samples per ray", Nc=257)
    _refused(lib, b"at most 256 samples per ray", **dict(FINE, Nc=129, Nf=128))
    _refused(lib, b"at most 256 samples per ray", **dict(FINE, Nc=2 ** 31 - 1, Nf=2 ** 31 - 1))
    for stride in (1, 63, 65, -64):
        _refused(lib, b"zc_stride must be 0 or Nc", zc_stride=stride)
        _refused(lib, b"zc_stride must be 0 or Nc", zc_stride=stride, **FINE)


def test_fine_pointers_go_with_nf():
    _, lib = _lib()
    for k in ("sig_f", "rgb_f", "z_f"):
        _refused(lib, b"Nf > 0 needs d_sigma_f, d_rgb_f and d_z_f", **dict(FINE, **{k: None}))
        _refused(lib, b"Nf == 0 takes no fine pointer", **{k: D})
    _refused(lib, b"Nf == 0 takes no fine pointer", grad_f=D, grad_c=D, out_normal=D)


def test_normal_and_gradients_go_together():
    _, lib = _lib()
    need = b"d_out_normal needs d_grad_c (and d_grad_f when Nf > 0)"
    _refused(lib, need, out_normal=D)
    _refused(lib, need, out_normal=D, **FINE)
    _refused(lib, need, out_normal=D, grad_c=D, **FINE)
    _refused(lib, need, out_normal=D, grad_f=D, **FINE)
    alone = b"a gradient pointer needs d_out_normal"
    _refused(lib, alone, grad_c=D)
    _refused(lib, alone, grad_c=D, **FINE)
    _refused(lib, alone, grad_f=D, **FINE)
    _refused(lib, alone, grad_c=D, grad_f=D, **FINE)


def test_the_size_guard_of_check_rn():
    L, lib = _lib()
    for R in (0, -3):
        _refused(lib, b"R and N must be positive", R=R)
    big = lib.cn_max_samples() // 64 + 1
    _refused(lib, b"exceed CN_MAX_SAMPLES", R=big)
    _refused(lib, b"exceed CN_MAX_SAMPLES", **dict(FINE, Nc=32, Nf=32, R=big))
