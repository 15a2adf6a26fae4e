"""CPU: compose.py's flags and the scene description (codenerf_amd/scene.py):
parsing and validation of scene files, Scene.depth_range, rotation_zyx and
OccupancyGrid.full.  Nothing here needs a device."""
import copy
import math

import numpy as np
import pytest
import torch


def _parser():
    import compose
    return compose, compose.build_parser()


def test_flags_parse_and_default_as_documented():
    compose, ap = _parser()
    a = ap.parse_args(["--scene", "s.json"])
    assert (a.saved_dir, a.jsonfile, a.gpu, a.codes, a.scene) == ("srncar", "srncar.json", 0, None, "s.json")
    assert (a.frames, a.azimuth, a.elevation, a.radius, a.size, a.focal) == (1, [0.0], 20.0, 1.3, 128, 131.25)
    assert (a.near, a.far, a.n_samples, a.n_importance, a.labels, a.out) == (None, None, None, None, True, None)
    a = ap.parse_args(["--scene", "s.json", "--saved_dir", "run", "--jsonfile", "hp.json", "--gpu", "1", "--codes",
                       "codes.pth", "--frames", "8", "--azimuth", "0", "360", "--elevation", "35", "--radius", "2",
                       "--size", "64", "--focal", "70", "--near", "0.5", "--far", "3", "--n_samples", "48",
                       "--n_importance", "16", "--labels", "False", "--out", "o"])
    assert (a.saved_dir, a.jsonfile, a.gpu, a.codes, a.frames, a.azimuth) == ("run", "hp.json", 1, "codes.pth", 8,
                                                                             [0.0, 360.0])
    assert (a.elevation, a.radius, a.size, a.focal, a.near, a.far) == (35.0, 2.0, 64, 70.0, 0.5, 3.0)
    assert (a.n_samples, a.n_importance, a.labels, a.out) == (48, 16, False, "o")
    with pytest.raises(SystemExit):
        ap.parse_args([])                        # --scene is required
    with pytest.raises(SystemExit):
        compose.main(["--scene", "s.json", "--azimuth", "0", "1", "2"])


def test_every_flag_is_in_the_module_docstring():
    compose, ap = _parser()
    for act in ap._actions:
        for opt in act.option_strings:
            if opt not in ("-h", "--help"):
                assert opt in compose.__doc__, opt
    for name in ("rgb_%03d.png", "instance_%03d.png", "alpha_%03d.png", "depth_%03d.png", "scene_frames.json"):
        assert name in compose.__doc__


def _entry(**kw):
    e = dict(shape=0, texture=1, translation=[0.1, 0.0, -0.2], rotation_deg=[30, 10, -5], scale=1.25, bound=0.5)
    e.update(kw)
    return e


def test_scene_description_is_parsed():
    from codenerf_amd.optimizer import OCC_DILATE, OCC_GRID, OCC_TAU
    from codenerf_amd.scene import parse_scene, rotation_zyx
    desc = {"objects": [_entry(), _entry(shape=[0, 2, 0.25], texture=[1, 1, 1.0], occ_grid=64, occ_tau=0.5,
                                         occ_dilate=0)]}
    before = copy.deepcopy(desc)
    a, b = parse_scene(desc, 3)
    assert desc == before
    assert a["shape"] == (0,) and a["texture"] == (1,) and a["scale"] == 1.25 and a["bound"] == 0.5
    assert (a["occ_grid"], a["occ_tau"], a["occ_dilate"]) == (OCC_GRID, OCC_TAU, OCC_DILATE)
    assert np.array_equal(a["rotation"], rotation_zyx(30, 10, -5)) and a["translation"].tolist() == [0.1, 0.0, -0.2]
    assert b["shape"] == (0, 2, 0.25) and b["texture"] == (1, 1, 1.0)
    assert (b["occ_grid"], b["occ_tau"], b["occ_dilate"]) == (64, 0.5, 0)


@pytest.mark.parametrize("bad", [
    {"objects": []},
    {"objects": [_entry()] * 9},
    {"things": [_entry()]},
    [_entry()],
    {"objects": [_entry(shape=3)]},
    {"objects": [_entry(texture=-1)]},
    {"objects": [_entry(shape=[0, 3, 0.5])]},
    {"objects": [_entry(shape=[0, 1])]},
    {"objects": [_entry(shape=0.5)]},
    {"objects": [_entry(scale=0)]},
    {"objects": [_entry(scale=-1.0)]},
    {"objects": [_entry(scale=float("inf"))]},
    {"objects": [_entry(scale=float("nan"))]},
    {"objects": [_entry(bound=0)]},
    {"objects": [_entry(translation=[0, 0])]},
    {"objects": [_entry(translation=[0, float("nan"), 0])]},
    {"objects": [_entry(rotation_deg=[0, 0])]},
    {"objects": [_entry(occ_grid=48)]},
    {"objects": [_entry(occ_tau=-1)]},
    {"objects": [_entry(occ_dilate=5)]},
    {"objects": [_entry(colour="red")]},
    {"objects": [{k: v for k, v in _entry().items() if k != "bound"}]},
])
def test_bad_scene_descriptions_are_refused(bad):
    from codenerf_amd.scene import parse_scene
    with pytest.raises(ValueError):
        parse_scene(bad, 3)


def _grid(bound=0.5):
    from codenerf_amd.occupancy import OccupancyGrid
    return OccupancyGrid.full(32, bound)


def test_scene_object_validates_its_transform():
    from codenerf_amd.scene import Scene, SceneObject, rotation_zyx
    code = torch.zeros(256)
    o = SceneObject(code, code, _grid())
    assert np.array_equal(o.rotation, np.eye(3)) and not o.translation.any() and o.scale == 1.0 and o.inv_s == 1.0
    assert o.transform_row() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    rot = rotation_zyx(40, -20, 10)
    o = SceneObject(code, code, _grid(), rot, (0.1, 0.2, 0.3), 2.0)
    assert o.inv_s == 0.5 and o.transform_row()[:9] == [float(np.float32(v)) for v in rot.reshape(-1)]
    SceneObject(code, code, _grid(), rot + 1e-5)             # a float32 rotation's rounding passes: within 1e-4
    for bad_rot in (rot * 1.01, np.eye(4), np.eye(3)[:2], np.diag([1.0, 1.0, -1.0]), rot + 1e-3,
                    np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            SceneObject(code, code, _grid(), bad_rot)
    for bad_scale in (0, -1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            SceneObject(code, code, _grid(), scale=bad_scale)
    with pytest.raises(ValueError):
        SceneObject(code, code, _grid(), translation=(0, 0))
    with pytest.raises(ValueError):
        SceneObject(code, code, None)                        # no object without a grid
    for n in (0, 9):
        with pytest.raises(ValueError):
            Scene([o] * n)
    assert len(Scene([o] * 8)) == 8 and len(Scene([o])) == 1
    with pytest.raises(ValueError):
        Scene([o, "car"])


def test_depth_range():
    from codenerf_amd.scene import Scene, SceneObject
    code = torch.zeros(256)
    a = SceneObject(code, code, _grid(0.5), translation=(0.3, 0.0, 0.4), scale=1.0)      # |t| = 0.5
    b = SceneObject(code, code, _grid(0.25), translation=(0.0, 0.1, 0.0), scale=2.0)
    rho = max(0.5 + math.sqrt(3) * 0.5, 0.1 + math.sqrt(3) * 2.0 * 0.25)
    near, far = Scene([a, b]).depth_range(3.0)
    assert near == pytest.approx(3.0 - rho) and far == pytest.approx(3.0 + rho)
    near, far = Scene([a, b]).depth_range(1.0)
    assert near == 0.05 and far == pytest.approx(1.0 + rho)
    assert Scene([b]).depth_range(2.0) == pytest.approx((2.0 - 0.1 - math.sqrt(3) * 0.5, 2.0 + 0.1 + math.sqrt(3) * 0.5))


def test_rotation_zyx_is_a_rotation():
    from codenerf_amd.scene import rotation_zyx
    assert np.array_equal(rotation_zyx(0, 0, 0), np.eye(3))
    for ypr in [(30, 0, 0), (0, 45, 0), (0, 0, 60), (115, -25, 5), (-270, 89, 180), (720, 360, -360)]:
        r = rotation_zyx(*ypr)
        assert r.shape == (3, 3) and r.dtype == np.float64
        np.testing.assert_allclose(r @ r.T, np.eye(3), atol=1e-12)
        assert np.linalg.det(r) == pytest.approx(1.0, abs=1e-12)
    # degrees, yaw about z: x -> y
    np.testing.assert_allclose(rotation_zyx(90, 0, 0) @ [1, 0, 0], [0, 1, 0], atol=1e-12)
    np.testing.assert_allclose(rotation_zyx(0, 90, 0) @ [0, 0, 1], [1, 0, 0], atol=1e-12)
    np.testing.assert_allclose(rotation_zyx(0, 0, 90) @ [0, 1, 0], [0, 0, 1], atol=1e-12)
    np.testing.assert_allclose(rotation_zyx(20, 30, 40), rotation_zyx(20, 0, 0) @ rotation_zyx(0, 30, 0)
                               @ rotation_zyx(0, 0, 40), atol=1e-12)


def test_occupancy_grid_full():
    import occupancy_util as U
    from codenerf_amd.occupancy import OccupancyGrid
    g = OccupancyGrid.full(32, 0.4, (0.1, 0.0, -0.1))
    assert g.G == 32 and g.bound == 0.4 and g.center == (0.1, 0.0, -0.1)
    assert g.bits.dtype == torch.int32 and g.bits.numel() == 32 ** 3 // 32 and g.fraction() == 1.0
    assert U.unpack_cells(g.bits.numpy().view(np.uint32), 32).all()
    # the box alone: a sample is kept exactly when it lies in [center - bound, center + bound)^3
    ro, rd = U.rays(8)
    z = U.midpoints(16)
    keep = U.keep_mask(ro, rd, z, g.bits.numpy().view(np.uint32), 32, np.array(g.lo, np.float32),
                       np.float32(g.inv_cell), False)
    x = U.points(ro, rd, z).astype(np.float64)
    inside = (np.abs(x - np.array(g.center)) < 0.4 - 1e-5).all(-1)
    outside = (np.abs(x - np.array(g.center)) > 0.4 + 1e-5).any(-1)
    assert keep[inside].all() and not keep[outside].any() and inside.any() and outside.any()
    assert OccupancyGrid.full(64).bits.numel() == 64 ** 3 // 32
    with pytest.raises(ValueError):
        OccupancyGrid.full(48)
