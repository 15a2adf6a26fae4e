"""CPU: the C ABI of the masked image loss (cn_render_loss_masked,
cn_render_loss_fine_masked): exported, bound, additive to ABI 4, and every
host check refuses with -1 and a message naming the entry before anything is
launched (the pointers below are never dereferenced)."""
import ctypes
import os

import pytest

ENTRIES = ("cn_render_loss_masked", "cn_render_loss_fine_masked")


def _lib():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load_library()


def test_both_symbols_are_exported_and_bound():
    L, lib = _lib()
    for name in ENTRIES:
        assert name in L.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(L._SIGS[name][1])
    # the plain entry's arguments, then weight, target, coefficient, opacity output (before the stream)
    for plain, masked in (("cn_render_loss", ENTRIES[0]), ("cn_render_loss_fine", ENTRIES[1])):
        a, b = L._SIGS[plain][1], L._SIGS[masked][1]
        assert b[:len(a) - 1] == a[:-1]
        assert b[len(a) - 1:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert L.ABI_VERSION == 4 and lib.cn_abi_version() == 4


def _coarse(lib, N=64, chunk=100, z_stride=0, weight=True, target=True, sil=0.0, R=8):
    d = ctypes.c_void_p(256)
    return lib.cn_render_loss_masked(d, d, d, z_stride, R, N, 1, d, chunk, d, d, d, d, d, d if weight else None,
                                     d if target else None, sil, d, None)


def _fine(lib, N=64, chunk=100, z_stride=0, weight=True, target=True, sil=0.0, R=8):
    """N: the merged sample count (Nc = N - 64 when that is positive)."""
    d = ctypes.c_void_p(256)
    Nc = N - 64 if N > 64 else N // 2
    return lib.cn_render_loss_fine_masked(d, d, d, z_stride, Nc, d, d, d, N - Nc, R, 1, d, chunk, d, d, d, d, d, d, d,
                                          d if weight else None, d if target else None, sil, d, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_host_checks_refuse_before_any_launch(entry):
    _, lib = _lib()
    call = _coarse if entry == ENTRIES[0] else _fine
    who = entry.encode()

    def refused(what, **kw):
        assert call(lib, **kw) == -1, kw
        err = lib.cn_last_error()
        assert who + b":" in err and what in err, err

    refused(b"256 samples", N=257)
    refused(b"chunk must be positive", chunk=0)
    refused(b"sil_coef", sil=-1.0)
    refused(b"sil_coef", sil=float("nan"))
    refused(b"sil_coef", sil=float("inf"))
    refused(b"d_acc_target", sil=0.5, target=False)
    refused(b"stride", z_stride=7)
    refused(b"R and N must be positive", R=0)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_required_argument_is_refused(entry):
    _, lib = _lib()
    d = ctypes.c_void_p(256)
    if entry == ENTRIES[0]:
        rc = lib.cn_render_loss_masked(d, d, d, 0, 8, 64, 1, None, 100, d, d, d, d, d, d, d, 0.0, d, None)
    else:
        rc = lib.cn_render_loss_fine_masked(d, d, d, 0, 32, d, d, d, 32, 8, 1, None, 100, d, d, d, d, d, d, d, d, d,
                                            0.0, d, None)
    assert rc == -1
    assert entry.encode() + b": NULL argument" in lib.cn_last_error()
