"""CPU: the numpy restatements of the scene entries (tests/scene_util.py), which
the GPU tests compare the kernels against, checked against closed forms."""
import numpy as np
import pytest

import occupancy_util as ou
import scene_util as su

F = np.float32


def _random_rows(rng, K):
    rots = [su.random_rotation(rng) for _ in range(K)]
    ts = rng.uniform(-0.3, 0.3, (K, 3))
    ss = rng.uniform(0.5, 2.0, K)
    return rots, ts, ss, np.stack([su.transform_row(r, t, s) for r, t, s in zip(rots, ts, ss)])


def test_ray_transform_is_the_inverse_similarity():
    rng = np.random.default_rng(0)
    ro, rd = ou.rays(16)
    rots, ts, ss, rows = _random_rows(rng, 8)
    o, d = su.scene_rays(ro, rd, rows)
    assert o.shape == d.shape == (8, 256, 3) and o.dtype == d.dtype == F
    for k in range(8):
        want_o = (ro.astype(np.float64) - ts[k]) @ rots[k] / ss[k]     # rows: R^T (o - t) / s
        want_d = rd.astype(np.float64) @ rots[k]
        np.testing.assert_allclose(o[k], want_o, rtol=0, atol=4e-6)
        np.testing.assert_allclose(d[k], want_d, rtol=0, atol=1e-6)
        # not re-normalised: a rotation keeps the length
        np.testing.assert_allclose(np.linalg.norm(d[k].astype(np.float64), axis=1),
                                   np.linalg.norm(rd.astype(np.float64), axis=1), rtol=1e-6)


def test_identity_hands_the_rays_back():
    ro, rd = ou.rays(16)
    o, d = su.scene_rays(ro, rd, su.transform_row(np.eye(3), np.zeros(3), 1.0)[None])
    # up to the sign of a zero: x + 0 * y may turn -0 into +0
    assert np.array_equal(o[0], ro) and np.array_equal(d[0], rd)
    nz = (ro != 0) & (rd != 0)
    assert su.same_bits(o[0][nz], ro[nz]) and su.same_bits(d[0][nz], rd[nz])


def test_sample_points_in_the_object_frame():
    """x_obj = R^T (x_world - t) / s at the samples: the object's ray at z / s."""
    rng = np.random.default_rng(1)
    ro, rd = ou.rays(16)
    z = ou.midpoints(32)
    rots, ts, ss, rows = _random_rows(rng, 3)
    o, d = su.scene_rays(ro, rd, rows)
    world = ro[:, None, :].astype(np.float64) + rd[:, None, :].astype(np.float64) * z[None, :, None]
    for k in range(3):
        zk = z * rows[k, 12]
        got = ou.points(o[k], d[k], zk).astype(np.float64)
        want = (world - ts[k]) @ rots[k] / ss[k]
        np.testing.assert_allclose(got, want, rtol=0, atol=8e-6)


def test_combine_closed_forms():
    rng = np.random.default_rng(2)
    M = 300
    sig = rng.uniform(0, 6, (1, M)).astype(F)
    sig[0, ::7] = 0
    rgb = rng.uniform(-1, 1, (1, M, 3)).astype(F)
    # K = 1, s = 1: the identity where sigma > 0, 0 colour where it is not
    s, c = su.combine(sig, rgb, [1.0])
    assert su.same_bits(s, sig[0])
    assert su.same_bits(c[sig[0] > 0], rgb[0][sig[0] > 0]) and not c[sig[0] == 0].any()
    # two equal objects: f = 1/2 each, the density doubles, the colour is kept (x/2 + x/2 is exact)
    s2, c2 = su.combine(np.repeat(sig, 2, 0), np.repeat(rgb, 2, 0), [1.0, 1.0])
    assert su.same_bits(s2, 2 * sig[0])
    f = su.shares(np.repeat(sig, 2, 0), [1.0, 1.0], s2)
    assert (f[:, sig[0] > 0] == F(0.5)).all() and not f[:, sig[0] == 0].any()
    assert su.same_bits(c2[sig[0] > 0], rgb[0][sig[0] > 0]) and not c2[sig[0] == 0].any()
    # a / s: scale 2 halves the density
    s3, _ = su.combine(sig, rgb, [0.5])
    assert su.same_bits(s3, sig[0] * F(0.5))
    # a NaN density: NaN sigma, 0 colour
    bad = sig.copy()
    bad[0, 5] = np.nan
    s4, c4 = su.combine(bad, rgb, [1.0])
    assert np.isnan(s4[5]) and not c4[5].any()
    # the sums run left to right
    big = np.array([[1e8], [1.0], [-1e8]], dtype=F)
    assert su.combine(big, np.ones((3, 1, 3), dtype=F), [1.0, 1.0, 1.0])[0][0] == F(0)


def _one_ray(Nc, owners, K, dens=1e4):
    """One ray over z in [1, 2]: sample i is owned by object owners[i] (density dens) or empty (None)."""
    z = np.linspace(1.0, 2.0, Nc).astype(F)
    oc = np.zeros((K, 1, Nc), dtype=F)
    for i, k in enumerate(owners):
        if k is not None:
            oc[k, 0, i] = dens
    ck = np.ones((K, 1, Nc, 3), dtype=F) * (np.arange(K, dtype=F)[:, None, None, None] + 1) / K
    inv_s = [1.0] * K
    sc, rc = su.combine(oc.reshape(K, -1), ck.reshape(K, -1, 3), inv_s)
    return z, sc.reshape(1, Nc), rc.reshape(1, Nc, 3), oc, inv_s


def test_composite_closed_forms():
    K, Nc = 3, 8
    # an opaque sample owned by one object: the one-hot, and its label
    for k in range(K):
        z, sc, rc, oc, inv_s = _one_ray(Nc, [None, None, k] + [None] * 5, K)
        r = su.restate_composite(z, sc, rc, oc, inv_s)
        np.testing.assert_allclose(r["obj_acc"][0], np.eye(K)[k], atol=1e-12)
        assert r["instance"][0] == k and not r["undecided"][0]
        np.testing.assert_allclose(r["rgb"][0], (k + 1) / K, atol=1e-6)
    # an empty ray
    z, sc, rc, oc, inv_s = _one_ray(Nc, [None] * Nc, K)
    r = su.restate_composite(z, sc, rc, oc, inv_s)
    assert r["instance"][0] == -1 and r["acc"][0] == 0 and not r["obj_acc"].any()
    # occlusion: the nearer opaque object owns the ray
    z, sc, rc, oc, inv_s = _one_ray(Nc, [None, 2, None, 0, 1, None, None, None], K)
    r = su.restate_composite(z, sc, rc, oc, inv_s)
    assert r["instance"][0] == 2
    # (an opaque sample still passes the renderer's 1e-10 of transmittance)
    np.testing.assert_allclose(r["obj_acc"][0], [1e-10, 1e-20, 1], rtol=1e-6, atol=1e-12)
    # a tie goes to the lower index: objects 1 and 2 share every sample equally
    oc = np.zeros((K, 1, Nc), dtype=F)
    oc[1:, 0, 2:5] = 3.0
    ck = np.full((K, 1, Nc, 3), 0.5, dtype=F)
    sc, rc = su.combine(oc.reshape(K, -1), ck.reshape(K, -1, 3), inv_s)
    r = su.restate_composite(z, sc.reshape(1, Nc), rc.reshape(1, Nc, 3), oc, inv_s, acc_min=0.1)
    assert r["obj_acc"][0, 1] == r["obj_acc"][0, 2] > 0 and r["instance"][0] == 1 and r["undecided"][0]


def test_shares_sum_to_the_opacity():
    """sum_k obj_acc = acc within 1e-12 where the combined density is an exact
    sum (integer densities, power-of-two scales), fine samples included."""
    rng = np.random.default_rng(3)
    K, R, Nc, Nf = 3, 16, 12, 9
    inv_s = [1.0, 0.5, 2.0]
    oc = rng.integers(0, 8, (K, R, Nc)).astype(F)
    of = rng.integers(0, 8, (K, R, Nf)).astype(F)
    zc = np.linspace(0.8, 1.8, Nc).astype(F)
    zf = np.sort(rng.uniform(0.8, 1.8, (R, Nf)), -1).astype(F)
    sc, rc = su.combine(oc.reshape(K, -1), rng.uniform(0, 1, (K, R * Nc, 3)).astype(F), inv_s)
    sf, rf = su.combine(of.reshape(K, -1), rng.uniform(0, 1, (K, R * Nf, 3)).astype(F), inv_s)
    for fine in (False, True):
        r = su.restate_composite(zc, sc.reshape(R, Nc), rc.reshape(R, Nc, 3), oc, inv_s,
                                 *((zf, sf.reshape(R, Nf), rf.reshape(R, Nf, 3), of) if fine else ()))
        assert r["w"].shape == (R, Nc + (Nf if fine else 0))
        np.testing.assert_allclose(r["obj_acc"].sum(-1), r["acc"], rtol=0, atol=1e-12)


def test_weights_restatement_agrees_with_the_float64_one():
    d = su.inputs(64, 0, False, 3)
    r = su.restate_inputs(d)
    got = su.obj_acc_from_weights(r["w"].astype(F), d["sc"], d["oc"], d["inv_s"])
    np.testing.assert_allclose(got, r["obj_acc"], rtol=0, atol=4e-6)


@pytest.mark.parametrize("K", su.KS)
def test_the_kernel_inputs_decide_their_labels(K, capsys):
    """At most 2 % of a case's rays are undecided, and every label occurs."""
    total = und_total = 0
    for (Nc, Nf) in su.SHAPES:
        for per_ray_z in (False, True):
            d = su.inputs(Nc, Nf, per_ray_z, K)
            assert d["oc"].shape == (K, su.R_MAX, Nc) and d["of"].shape == (K, su.R_MAX, Nf)
            assert not d["oc"][:, 1].any() and not d["of"][:, 1].any() and d["oc"][K - 1, 2, Nc // 2] == F(1e4)
            r = su.restate_inputs(d)
            und = int(r["undecided"].sum())
            total += su.R_MAX
            und_total += und
            seen = set(r["instance"][~r["undecided"]].tolist())
            with capsys.disabled():
                print(f"scene inputs Nc {Nc} Nf {Nf} per-ray z {int(per_ray_z)} K {K}: {und} of {su.R_MAX} rays "
                      f"undecided, labels {sorted(seen)}")
            assert und <= su.MAX_UNDECIDED * su.R_MAX
            assert seen == set(range(-1, K))
            assert r["instance"][1] == -1 and r["acc"][2] > 0.99
    with capsys.disabled():
        print(f"K {K}: {und_total} of {total} rays undecided")
