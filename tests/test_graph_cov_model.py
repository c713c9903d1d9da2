"""tests/graph_cov_model.py — the NumPy restatement of the graph's covariances and of the loop gate — checked against closed forms,
and graph_gate of liodom_math.h, compiled for the host with -ffp-contract=off (tests/graph_gate_host.cc), held to it.  Also the
conditions on the designed graphs that the bounds of tests/test_gpu_pose_graph_cov.py rest on.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_cov_model as gc
import graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check"
    so = str(tmp_path_factory.mktemp("graph_gate") / "libgraphgate.so")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "graph_gate_host.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ggh_gate.restype = C.c_int
    L.ggh_gate.argtypes = [C.POINTER(C.c_double)] * 8
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_two_nodes_one_fixed_closed_form():
    rng = np.random.default_rng(1)
    Xi, Xj = gm.random_pose(rng), gm.random_pose(rng)
    M = rng.normal(size=(6, 6))
    Om = M @ M.T + np.eye(6)
    Om = 0.5 * (Om + Om.T)
    edges = gm.api.graph_edges([0], [1], [gm.random_pose(rng, 3.0)], Om)
    fixed = np.array([1, 0], np.int32)
    poses = np.stack([Xi, Xj])
    lin = gm.linearize(poses, fixed, edges)
    s = gc.system(lin, fixed, edges)
    B = lin["B"][0]
    want = np.linalg.inv(B.T @ Om @ B)
    Sg, st = gc.block(s, 1, 1)
    assert st == gc.OK and np.max(np.abs(Sg - want)) <= 1e-12 * np.linalg.cond(B.T @ Om @ B) * np.max(np.abs(want))
    for r, c in ((0, 0), (0, 1), (1, 0)):
        Z, st = gc.block(s, r, c)
        assert st == gc.OK and not Z.any()
    assert s["anchored"].all() and list(s["nodes"]) == [1]


def test_sigma_is_symmetric_positive_definite_on_every_designed_graph_and_the_drift_stays_below_a_tenth_of_the_tolerance():
    for case in gc.designed():
        s = gc.system(gc.lin_of(case), case["fixed"], case["edges"], case["active"])
        assert s["pd"], case["name"]
        if s["Sigma"] is not None:
            assert np.array_equal(s["Sigma"], s["Sigma"].T) and np.linalg.eigvalsh(s["Sigma"])[0] > 0.0
        worst = 0.0
        for q in case["query"]:
            Sg, st = gc.block(s, q, q)
            if s["fixed"][q]:
                assert st == gc.OK and not Sg.any()
            elif not s["anchored"][q]:
                assert st == gc.UNANCHORED and np.isnan(Sg).all()
            else:
                assert st == gc.OK and np.linalg.eigvalsh(0.5 * (Sg + Sg.T))[0] > 0.0
                worst = max(worst, max(float(np.linalg.norm(gc.column(s, q, b))) for b in range(6)))
        d = gc.drift_allowance(s, case["max_pcg_iterations"], worst)
        print("%s: | |H| | %.3g, max |x| %.3g, d at the cap of %d iterations %.3g, tolerance %.1g" %
              (case["name"], s["norm_abs"], worst, case["max_pcg_iterations"], d, case["pcg_tolerance"]))
        assert d <= case["pcg_tolerance"] / 10.0, case["name"]
        assert len(case["query"]) <= 8 + 1


def test_anchoring_and_statuses():
    case = [c for c in gc.designed() if c["name"] == "two_components"][0]
    s = gc.system(gc.lin_of(case), case["fixed"], case["edges"])
    assert s["anchored"][:6].all() and not s["anchored"][6:].any()
    assert gc.block(s, 7, 7)[1] == gc.UNANCHORED and gc.block(s, 1, 7)[1] == gc.UNANCHORED and gc.block(s, 0, 7)[1] == gc.OK
    cand = gm.api.graph_edges([1], [7], [gm.between(case["poses"][1], case["poses"][7])], gm.OMEGA)
    d2, st = gc.gate(s, case["poses"], cand[0])
    assert st == gc.UNANCHORED and np.isnan(d2)
    cand = gm.api.graph_edges([1], [2], [gm.between(case["poses"][1], case["poses"][2])], -gm.OMEGA)
    d2, st = gc.gate(s, case["poses"], cand[0])
    assert st == gc.NOT_PD and np.isnan(d2)
    # a stored edge with a negative definite Omega: H is not positive definite
    bad = case["edges"].copy()
    bad["info"][2] = -bad["info"][2]
    s = gc.system(gm.linearize(case["poses"], case["fixed"], bad), case["fixed"], bad)
    assert not s["pd"] and gc.block(s, 1, 1)[1] == gc.BREAKDOWN and gc.block(s, 0, 1)[1] == gc.OK and gc.block(s, 7, 7)[1] == gc.UNANCHORED
    # inactive edges cut the anchor
    case = [c for c in gc.designed() if c["name"] == "weighted_ring"][0]
    act = case["active"].copy()
    assert gc.anchored(case["fixed"], case["edges"], act).all()
    act[[3, 11, 12]] = 0          # odometry 3-4 and both loops: nodes 4 .. 11 hang on nothing fixed
    assert gc.anchored(case["fixed"], case["edges"], act).tolist() == [True] * 4 + [False] * 8


def test_the_gate_is_zero_at_the_prediction_and_grows_with_the_offset():
    init, fixed, odo, true, false = gc.gate_ring()
    s = gc.system(gm.linearize(init, fixed, odo), fixed, odo)
    exact = gm.api.graph_edges([0], [11], [gm.between(init[0], init[11])], gc.GATE_INFO)
    d2, st = gc.gate(s, init, exact[0])
    assert st == gc.OK and 0.0 <= d2 <= 1e-24
    last = 0.0
    for off in (0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 20.0):
        c = exact.copy()
        c["z"][0, 4:] += off * np.array([0.6, 0.8, 0.0])
        d2, st = gc.gate(s, init, c[0])
        assert st == gc.OK and d2 > last
        last = d2
    d_true, st_t = gc.gate(s, init, true[0])
    d_false, st_f = gc.gate(s, init, false[0])
    print("ring of 12, seed %d: d2 of the true closing edge %.3f, displaced by 5 m %.3f" % (gc.GATE_SEED, d_true, d_false))
    assert st_t == gc.OK and st_f == gc.OK and d_true < gc.CHI2_6_099 and d_false > 100.0
    assert abs(float(np.linalg.norm(false["z"][0, 4:] - true["z"][0, 4:])) - 5.0) <= 1e-12


def _gate_inputs():
    """Per jacobian case: Omega and a 12 x 12 symmetric positive definite Sigma cut into its three blocks."""
    rng = np.random.default_rng(31)
    out = []
    for name, Xi, Xj, Z in gm.jacobian_cases():
        M = rng.normal(size=(12, 12))
        Sg = 1e-3 * (M @ M.T + 12.0 * np.eye(12))
        Sg = 0.5 * (Sg + Sg.T)
        K = rng.normal(size=(6, 6))
        Om = 50.0 * (K @ K.T + 6.0 * np.eye(6))
        Om = 0.5 * (Om + Om.T)
        out.append((name, Xi, Xj, Z, Om, Sg))
    return out


@pytest.mark.parametrize("name,Xi,Xj,Z,Om,Sg", _gate_inputs(), ids=[c[0] for c in _gate_inputs()])
def test_graph_gate_on_the_host_equals_the_model(lib, name, Xi, Xj, Z, Om, Sg):
    """1e-9 relative, double against double — where the condition number of S leaves it room.  Both sides FORM S = J Sigma J^T +
    Omega^-1 in double: every entry is two nested sums of 12 products, rounded at the size of |S|_2, 26 eps |S|_2 for each side,
    and d2 = e^T S^-1 e moves by kappa_2(S) times that, relatively: 52 eps kappa_2(S).  Ten of the eleven cases have kappa_2(S) <=
    6e4 — 3e-10, the bound is the 1e-9 — and differ by 3e-14 .. 2e-13.  The 100 km case does not: J holds 2 W [t_j - t_i]x with
    |t_j - t_i| = 1.7e5 m, which has no component along t_j - t_i, so S has two eigenvalues of 1e9 and one of 1e-2 in its
    translation block, kappa_2(S) = 1.06e12, and the two sides differ by 1.0e-6 of d2 = 7.6e11 (measured; the bound there is
    52 eps kappa = 6e-3).  The digits are lost where S is formed, not in the Cholesky solve.  The zero-error cases have d2 = 0 in
    exact arithmetic: e is what rounding left, at most 1e-13 (1 + |t_j - t_i| + |t_z|) per component off the model's
    (tests/test_graph_math_host.py), and d2 <= |S^-1|_2 |e|^2."""
    Sii, Sij, Sjj = (np.ascontiguousarray(b) for b in (Sg[:6, :6], Sg[:6, 6:], Sg[6:, 6:]))
    want, st, S, e, J = gc.gate_blocks(Xi, Xj, Z, Om, Sii, Sij, Sjj)
    assert st == gc.OK
    got = np.zeros(1)
    assert lib.ggh_gate(_p(np.ascontiguousarray(Xi)), _p(np.ascontiguousarray(Xj)), _p(np.ascontiguousarray(Z)), _p(np.ascontiguousarray(Om)),
                        _p(Sii), _p(Sij), _p(Sjj), _p(got)) == 1
    cond = float(np.linalg.cond(S))
    print("%s: d2 %.17g, model %.17g, relative difference %.3g, cond(S) %.3g" % (name, got[0], want, abs(got[0] - want) / max(want, 1e-300), cond))
    if "zero_error" in name:
        e_max = float(np.linalg.norm(e)) + np.sqrt(6.0) * 1e-13 * gm.edge_scale(Xi, Xj, Z)
        assert 0.0 <= got[0] <= float(np.linalg.norm(np.linalg.inv(S), 2)) * e_max ** 2
    else:
        assert abs(got[0] - want) <= max(1e-9, 52.0 * gc.EPS * cond) * want
        assert cond <= 6e4 or name == "100km"


def test_graph_gate_on_the_host_refuses_what_is_not_positive_definite(lib):
    name, Xi, Xj, Z, Om, Sg = _gate_inputs()[0]
    Sii, Sij, Sjj = (np.ascontiguousarray(b) for b in (Sg[:6, :6], Sg[:6, 6:], Sg[6:, 6:]))
    args = [_p(np.ascontiguousarray(v)) for v in (Xi, Xj, Z)]
    got = np.zeros(1)
    assert lib.ggh_gate(*args, _p(np.ascontiguousarray(-Om)), _p(Sii), _p(Sij), _p(Sjj), _p(got)) == 0 and np.isnan(got[0])
    assert lib.ggh_gate(*args, _p(np.ascontiguousarray(Om)), _p(np.ascontiguousarray(-1e3 * Sii)), _p(Sij), _p(Sjj), _p(got)) == 0 and np.isnan(got[0])
    sing = Om.copy()
    sing[:] = 0.0
    assert lib.ggh_gate(*args, _p(sing), _p(Sii), _p(Sij), _p(Sjj), _p(got)) == 0 and np.isnan(got[0])
