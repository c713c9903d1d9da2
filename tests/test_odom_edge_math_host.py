"""The odometry-edge leaf functions of liodom_math.h (odom_scan_usable, odom_transport_term, odom_lane_partial, odom_combine64,
odom_edge_covariance, odom_edge_information, odom_edge_finish) compiled for the host with -ffp-contract=off
(tests/odom_edge_host.cc) and held to tests/odom_edge_model.py on designed inputs.

Z, Sigma and Sigma_e must be BIT-EQUAL: the model restates every operation in the library's order.  Omega is a Cholesky inverse
in the library and np.linalg.inv in the model: they differ by rounding x condition, eps kappa 100 = 2.2e-16 x 1e6 x 100 = 2.2e-8
at the worst, and the inputs are designed with kappa(Sigma_e) <= 1e6 (asserted), so the bound is 1e-8 relative in Frobenius
norm.  Omega and Sigma_e are symmetric bit for bit.  Every flag is reached.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from liodom_amd import api

import odom_edge_host_lib as hl
import odom_edge_model as om


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hl.build(tmp_path_factory.mktemp("odom_edge_host"))


@pytest.fixture(scope="module")
def stream():
    poses, covs = om.designed_stream(140, seed=3)
    return poses, om.records(covs)


def _same(host, model):
    """One host record against the model's dict: everything but Omega as bits."""
    assert int(host["flags"]) == model["flags"] and int(host["n_used"]) == model["n_used"] and int(host["n_missing"]) == model["n_missing"]
    assert int(host["reserved"]) == 0
    assert np.array_equal(host["z"], model["z"], equal_nan=True)
    assert np.array_equal(host["covariance"], model["covariance"], equal_nan=True)
    assert np.isnan(host["information"]).all() == np.isnan(model["information"]).all()


INTERVALS = [(0, 1), (0, 2), (3, 66), (1, 65), (2, 67), (5, 134), (70, 75), (63, 64), (64, 129), (0, 139)]


@pytest.mark.parametrize("options", [dict(), dict(inflation=2.5, floor_rotation=1e-4, floor_translation=2e-3)], ids=["raw", "inflated_floored"])
def test_records_equal_the_model(lib, stream, options):
    poses, recs = stream
    f, t = [i[0] for i in INTERVALS], [i[1] for i in INTERVALS]
    host = hl.chain(lib, poses, recs, f, t, **options)
    worst = 0.0
    for row, (a, b) in enumerate(INTERVALS):
        m = om.chain(poses, recs, a, b, **options)
        h = host[row]
        assert (int(h["scan_from"]), int(h["scan_to"])) == (a, b)
        assert m["flags"] == om.VALID and m["n_used"] == b - a and m["n_missing"] == 0
        _same(h, m)
        tot = hl.totals(lib, poses, recs, a, b, **options)
        sigma = np.array([[tot[om.sym(r, c)] for c in range(6)] for r in range(6)])
        assert np.array_equal(sigma, m["sigma"])                          # Sigma, bit for bit
        assert tot[21] == b - a and tot[22] == 0 and tot[23] == 0
        kappa = np.linalg.cond(m["covariance"])
        assert kappa <= 1e6, "the designed input must keep kappa(Sigma_e) <= 1e6, has %.3g" % kappa
        rel = np.linalg.norm(h["information"] - m["information"]) / np.linalg.norm(m["information"])
        worst = max(worst, rel)
        print("interval (%d, %d): kappa %.3g, Omega relative difference %.3g" % (a, b, kappa, rel))
        assert rel <= 1e-8
        assert np.array_equal(h["information"], h["information"].T) and np.array_equal(h["covariance"], h["covariance"].T)
        # and the dense restatement says the same to rounding
        S, Se, Om = om.chain_dense(poses, recs["covariance"], a, b, **options)
        assert np.linalg.norm(S - m["sigma"]) <= 1e-12 * np.linalg.norm(S) and np.linalg.norm(Se - m["covariance"]) <= 1e-12 * np.linalg.norm(Se)
    print("worst Omega difference %.3g" % worst)


def test_the_leaf_functions_one_by_one(lib, stream):
    poses, recs = stream
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(5)
    for k in (1, 17, 99):
        u = rng.normal(scale=20.0, size=3)
        M = np.zeros(21)
        Ck = np.ascontiguousarray(recs["covariance"][k])
        lib.oeh_term(dp(Ck), dp(u), 1.7, 1e-8, 4e-6, dp(M))
        assert np.array_equal(M, np.array(om.transport_term(Ck, u, 1.7, 1e-8, 4e-6)))
        T = om.transport(u)
        want = T @ (1.7 * Ck + np.diag([1e-8] * 3 + [4e-6] * 3)) @ T.T
        got = np.array([[M[om.sym(r, c)] for c in range(6)] for r in range(6)])
        assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    # the usable-scan test
    r = recs[5:6].copy()
    assert lib.oeh_usable(r.ctypes.data_as(C.c_void_p), 5) == 1 and lib.oeh_usable(r.ctypes.data_as(C.c_void_p), 6) == 0
    for flags in (0, api.COV_VALID | api.COV_SINGULAR, api.COV_NO_SOLVE, api.COV_EVAL_FAILURE, api.COV_VALID | api.COV_FEW_RESIDUALS):
        r2 = r.copy(); r2["flags"] = flags
        assert lib.oeh_usable(r2.ctypes.data_as(C.c_void_p), 5) == 0 and not om.usable(r2[0], 5)
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (5, 5), (2, 4), (4, 2)):
            r2 = r.copy(); r2["covariance"][0][at] = bad
            assert lib.oeh_usable(r2.ctypes.data_as(C.c_void_p), 5) == 0 and not om.usable(r2[0], 5)
    # a matrix that is not positive definite leaves Omega untouched
    Se, Om = -np.eye(6), np.full((6, 6), 7.0)
    assert lib.oeh_information(dp(Se), dp(Om)) == 0 and np.all(Om == 7.0)
    Se = np.diag([1e-6, 2e-6, 3e-6, 1e-5, 2e-5, 3e-5])
    assert lib.oeh_information(dp(Se), dp(Om)) == 1 and np.allclose(Om, np.linalg.inv(Se), rtol=1e-14, atol=0)


def _broken(recs, k, how):
    r = recs.copy()
    if how == "no_solve":
        r["flags"][k] = api.COV_NO_SOLVE
    elif how == "singular":
        r["flags"][k] = api.COV_VALID | api.COV_SINGULAR
    elif how == "index":
        r["scan_index"][k] = k - 1
    elif how == "nan":
        r["covariance"][k][3, 1] = np.nan
    return r


def test_gaps_at_the_start_in_the_middle_and_at_the_end(lib, stream):
    poses, recs = stream
    a, b = 10, 90
    clean = om.chain(poses, recs, a, b)
    for ks, how in (((a + 1,), "no_solve"), ((50,), "singular"), ((b,), "index"), ((a + 1, 50, 51, b), "nan"), ((a + 64,), "no_solve")):
        r = recs
        for k in ks:
            r = _broken(r, k, how)
        h = hl.chain(lib, poses, r, [a], [b])[0]
        m = om.chain(poses, r, a, b)
        assert m["flags"] == (om.VALID | om.GAPS) and m["n_missing"] == len(ks) and m["n_used"] == b - a - len(ks)
        _same(h, m)
        assert np.array_equal(h["z"], clean["z"])                         # Z does not depend on the records
        assert not np.array_equal(h["covariance"], clean["covariance"])
        assert np.linalg.norm(h["information"] - m["information"]) <= 1e-8 * np.linalg.norm(m["information"])
    # a broken record outside a + 1 .. b changes nothing: scan a's own record is not part of the interval
    h = hl.chain(lib, poses, _broken(_broken(recs, a, "no_solve"), b + 1, "nan"), [a], [b])[0]
    assert int(h["flags"]) == om.VALID and np.array_equal(h["covariance"], clean["covariance"])


def test_not_pd_and_no_pose(lib, stream):
    poses, recs = stream
    a, b = 20, 30
    clean = om.chain(poses, recs, a, b)
    # every scan missing: nothing to invert
    r = recs.copy(); r["flags"][a + 1:b + 1] = api.COV_EVAL_FAILURE
    h, m = hl.chain(lib, poses, r, [a], [b])[0], om.chain(poses, r, a, b)
    assert m["flags"] == (om.NOT_PD | om.GAPS) and m["n_used"] == 0 and m["n_missing"] == b - a
    _same(h, m)
    assert np.isnan(h["covariance"]).all() and np.isnan(h["information"]).all() and np.array_equal(h["z"], clean["z"])
    # a singular Sigma: zero covariances and zero floors; with floors the same records are fine
    r = recs.copy(); r["covariance"][a + 1:b + 1] = 0.0
    h, m = hl.chain(lib, poses, r, [a], [b])[0], om.chain(poses, r, a, b)
    assert m["flags"] == om.NOT_PD and m["n_used"] == b - a and m["n_missing"] == 0
    _same(h, m)
    assert np.isnan(h["covariance"]).all() and np.isnan(h["information"]).all() and np.array_equal(h["z"], clean["z"])
    h = hl.chain(lib, poses, r, [a], [b], floor_rotation=1e-3, floor_translation=1e-2)[0]
    m = om.chain(poses, r, a, b, floor_rotation=1e-3, floor_translation=1e-2)
    assert m["flags"] == om.VALID
    _same(h, m)
    assert np.linalg.norm(h["information"] - m["information"]) <= 1e-8 * np.linalg.norm(m["information"])
    # a pose that is not finite at a, at b, in between — and a zero quaternion at an end —: everything is NaN
    for k, col, bad in ((a, 5, np.nan), (b, 0, np.inf), (25, 6, np.nan), (25, 2, -np.inf), (a, None, 0.0), (b, None, 0.0)):
        p = poses.copy()
        if col is None:
            p[k, :4] = bad
        else:
            p[k, col] = bad
        h, m = hl.chain(lib, p, recs, [a], [b])[0], om.chain(p, recs, a, b)
        assert m["flags"] == om.NO_POSE
        _same(h, m)
        assert np.isnan(h["z"]).all() and np.isnan(h["covariance"]).all() and np.isnan(h["information"]).all()
    # a quaternion in between is not read: only its being finite counts; one that is merely not normalised at an end is normalised
    p = poses.copy(); p[a, :4] *= 3.0; p[b, :4] *= 0.25
    h = hl.chain(lib, p, recs, [a], [b])[0]
    assert int(h["flags"]) == om.VALID and np.allclose(h["z"], clean["z"], rtol=0, atol=1e-15)
    _same(h, om.chain(p, recs, a, b))
