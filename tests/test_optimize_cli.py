"""CPU: optimize.py's command line (no device).

--n_importance is left to the JSON config unless given: the default must be
None (not 0), so a config trained with the fine pass is optimised with it.
"""
import optimize


def test_n_importance_defaults_to_the_json():
    assert optimize.build_parser().parse_args([]).n_importance is None


def test_n_importance_is_an_int():
    a = optimize.build_parser().parse_args(["--n_importance", "32"])
    assert a.n_importance == 32 and isinstance(a.n_importance, int)
    assert optimize.build_parser().parse_args(["--n_importance", "0"]).n_importance == 0


def test_the_flag_is_described():
    assert "--n_importance" in optimize.__doc__
