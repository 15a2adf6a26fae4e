"""CPU: optimize.py's mask flags (no device): defaults are the plain loop,
the values are typed, and the module docstring describes them."""
import pytest

import optimize


def test_defaults_are_the_plain_loop():
    a = optimize.build_parser().parse_args([])
    assert a.mask == "none"
    assert a.bg_weight == 0.0 and isinstance(a.bg_weight, float)
    assert a.sil_coef == 0.0 and isinstance(a.sil_coef, float)


def test_types_and_choices():
    a = optimize.build_parser().parse_args(["--mask", "files", "--bg_weight", "0.25", "--sil_coef", "1"])
    assert a.mask == "files"
    assert a.bg_weight == 0.25 and isinstance(a.bg_weight, float)
    assert a.sil_coef == 1.0 and isinstance(a.sil_coef, float)
    assert optimize.build_parser().parse_args(["--mask", "white"]).mask == "white"
    for bad in (["--mask", "alpha"], ["--bg_weight", "x"], ["--sil_coef", "lots"]):
        with pytest.raises(SystemExit):
            optimize.build_parser().parse_args(bad)


def test_the_existing_defaults_stay():
    a = optimize.build_parser().parse_args([])
    assert a.n_importance is None and a.device_metrics is False and a.optimize_pose is False
    assert a.num_opts == 200 and a.lr == 1e-2 and a.splits == "test"


def test_the_flags_are_described():
    for flag in ("--mask", "--bg_weight", "--sil_coef"):
        assert flag in optimize.__doc__
