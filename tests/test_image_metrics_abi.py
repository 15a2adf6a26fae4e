"""CPU: the C ABI of the device evaluation metrics (cn_image_metrics,
cn_image_metrics_ws_bytes) and the --device_metrics flag; no device needed
(the refusals come before any device call, the pointers are never
dereferenced)."""
import ctypes

import pytest

import optimize
from codenerf_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


def test_both_symbols_are_exported(lib):
    assert "cn_image_metrics" in _lib.EXPORTED and "cn_image_metrics_ws_bytes" in _lib.EXPORTED
    assert hasattr(lib, "cn_image_metrics") and hasattr(lib, "cn_image_metrics_ws_bytes")
    assert _lib.ABI_VERSION == 4 and lib.cn_abi_version() == 4          # additive to ABI 4


@pytest.mark.parametrize("H,W,V,chunk,word", [(6, 7, 1, 1, b"at least 7"), (7, 6, 1, 1, b"at least 7"),
                                              (0, 0, 1, 1, b"at least 7"), (-3, 16, 1, 1, b"at least 7"),
                                              (16, 16, 0, 1, b"V must"), (16, 16, -1, 1, b"V must"),
                                              (16, 16, 1, 0, b"chunk must"), (16, 16, 1, -5, b"chunk must")])
def test_invalid_shapes_are_refused(lib, H, W, V, chunk, word):
    d = ctypes.c_void_p(256)
    assert lib.cn_image_metrics_ws_bytes(H, W, V, chunk) == 0
    assert lib.cn_image_metrics(d, d, H, W, V, chunk, d, None, d, None) == -1
    msg = lib.cn_last_error()
    assert b"cn_image_metrics" in msg and word in msg, msg


@pytest.mark.parametrize("null", ["d_img", "d_gt", "d_out", "d_ws"])
def test_null_pointers_are_refused(lib, null):
    d = ctypes.c_void_p(256)
    p = {k: (None if k == null else d) for k in ("d_img", "d_gt", "d_out", "d_ws")}
    assert lib.cn_image_metrics(p["d_img"], p["d_gt"], 16, 16, 1, 2048, p["d_out"], None, p["d_ws"], None) == -1
    assert b"cn_image_metrics: NULL argument" in lib.cn_last_error()


def test_workspace_size(lib):
    assert lib.cn_image_metrics_ws_bytes(7, 7, 1, 1) > 0
    one = lib.cn_image_metrics_ws_bytes(128, 128, 1, 2048)
    assert one > 0 and one % 8 == 0
    # every view has its own partials: the size is linear in V
    assert lib.cn_image_metrics_ws_bytes(128, 128, 249, 2048) == 249 * one
    # a chunk above H * W is one chunk, whatever its value
    assert lib.cn_image_metrics_ws_bytes(37, 70, 1, 37 * 70) == lib.cn_image_metrics_ws_bytes(37, 70, 1, 1 << 30)


def test_device_metrics_flag():
    ap = optimize.build_parser()
    assert ap.parse_args([]).device_metrics is False
    assert ap.parse_args(["--device_metrics", "True"]).device_metrics is True
    assert ap.parse_args(["--device_metrics", "False"]).device_metrics is False
    assert "--device_metrics" in optimize.__doc__


def test_image_metrics_has_no_cpu_fallback():
    import torch
    from codenerf_amd.metrics import image_metrics
    if torch.cuda.is_available():
        pytest.skip("device present")
    x = torch.zeros(49, 3)
    with pytest.raises(_lib.HipUnavailable):
        image_metrics(x, x, 7, 7, 2048)
