"""The pose-graph leaf functions of liodom_math.h (graph_edge_error, graph_edge_blocks, graph_retract, graph_damped_inverse) compiled
for the host with -ffp-contract=off (tests/graph_math_host.cc) and held to tests/graph_model.py.  e, A and B within
1e-13 * (1 + |t_j - t_i| + |t_z|): three chained unit-quaternion products and two rotations of a vector of that length come to
roughly 30 eps * scale, so the bound is about 15 x the estimate.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check"
    so = str(tmp_path_factory.mktemp("graph_math") / "libgraphmath.so")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "graph_math_host.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.gmh_edge.argtypes = [dp] * 6
    L.gmh_error.argtypes = [dp] * 4
    L.gmh_chi2.restype = C.c_double
    L.gmh_chi2.argtypes = [dp, dp]
    L.gmh_blocks.argtypes = [dp] * 10
    L.gmh_retract.argtypes = [dp] * 3
    L.gmh_damped_inverse.restype = C.c_int
    L.gmh_damped_inverse.argtypes = [dp, C.c_double, dp]
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _edge(L, Xi, Xj, Z):
    e, A, B = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    L.gmh_edge(_p(np.ascontiguousarray(Xi)), _p(np.ascontiguousarray(Xj)), _p(np.ascontiguousarray(Z)), _p(e), _p(A), _p(B))
    return e, A, B


@pytest.mark.parametrize("name,Xi,Xj,Z", gm.jacobian_cases(), ids=[c[0] for c in gm.jacobian_cases()])
def test_error_and_jacobians_equal_the_model(lib, name, Xi, Xj, Z):
    e, A, B = _edge(lib, Xi, Xj, Z)
    em, Am, Bm = gm.edge_jacobians(Xi, Xj, Z)
    bound = 1e-13 * gm.edge_scale(Xi, Xj, Z)
    worst = max(float(np.max(np.abs(e - em))), float(np.max(np.abs(A - Am))), float(np.max(np.abs(B - Bm))))
    print("%s: worst difference %.3g, bound %.3g" % (name, worst, bound))
    assert worst <= bound
    only = np.zeros(6)
    lib.gmh_error(_p(np.ascontiguousarray(Xi)), _p(np.ascontiguousarray(Xj)), _p(np.ascontiguousarray(Z)), _p(only))
    assert np.array_equal(only, e)                     # the error alone is the same code
    if "w_negative" in name:
        assert gm.compose(gm.inverse(Z), gm.between(Xi, Xj))[3] < 0.0


def test_the_blocks_equal_the_model(lib):
    rng = np.random.default_rng(4)
    for k in range(8):
        Xi, Xj, Z = gm.random_pose(rng), gm.random_pose(rng), gm.random_pose(rng, 3.0)
        M = rng.normal(size=(6, 6))
        Om = M @ M.T + np.eye(6)
        Om = 0.5 * (Om + Om.T) if k % 2 else np.diag(np.diag(Om))
        e, A, B = _edge(lib, Xi, Xj, Z)
        chi2 = np.zeros(1)
        gi, gj, Hii, Hij, Hjj = np.zeros(6), np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6))
        lib.gmh_blocks(_p(e), _p(A), _p(B), _p(Om), _p(chi2), _p(gi), _p(gj), _p(Hii), _p(Hij), _p(Hjj))
        aO, aA, aB, ae = np.abs(Om), np.abs(A), np.abs(B), np.abs(e)
        # each entry is a sum of 36 products of three factors: 1e-13 of the same sum over absolute values is ~ 10 x its rounding
        assert abs(chi2[0] - e @ Om @ e) <= 1e-13 * (ae @ aO @ ae)
        assert chi2[0] == lib.gmh_chi2(_p(e), _p(Om))
        assert np.all(np.abs(gi - A.T @ Om @ e) <= 1e-13 * (aA.T @ aO @ ae)) and np.all(np.abs(gj - B.T @ Om @ e) <= 1e-13 * (aB.T @ aO @ ae))
        assert np.all(np.abs(Hii - A.T @ Om @ A) <= 1e-13 * (aA.T @ aO @ aA))
        assert np.all(np.abs(Hij - A.T @ Om @ B) <= 1e-13 * (aA.T @ aO @ aB))
        assert np.all(np.abs(Hjj - B.T @ Om @ B) <= 1e-13 * (aB.T @ aO @ aB))
        assert np.array_equal(Hii, Hii.T) and np.array_equal(Hjj, Hjj.T)


def test_retraction_and_damped_inverse(lib):
    rng = np.random.default_rng(6)
    for scale in (0.0, 1e-9, 1e-3, 0.3, 0.6, 2.0):
        X = gm.random_pose(rng)
        d = np.concatenate([rng.normal(size=3) * scale, rng.normal(size=3)])
        out = np.zeros(7)
        lib.gmh_retract(_p(X), _p(d), _p(out))
        assert np.max(np.abs(out - gm.retract(X, d))) <= 1e-14 * (1.0 + np.linalg.norm(X[4:]))
        assert abs(np.linalg.norm(out[:4]) - 1.0) <= 4e-16
    M = rng.normal(size=(6, 6))
    D = M @ M.T + np.eye(6)
    D = 0.5 * (D + D.T)
    inv = np.zeros((6, 6))
    for lam in (0.0, 1e-4, 10.0):
        assert lib.gmh_damped_inverse(_p(D), lam, _p(inv)) == 1
        want = np.linalg.inv(D + lam * np.diag(np.diag(D)))
        assert np.max(np.abs(inv - want)) <= 1e-12 * np.linalg.cond(D) * np.max(np.abs(want))
    before = inv.copy()
    assert lib.gmh_damped_inverse(_p(-D), 0.0, _p(inv)) == 0 and np.array_equal(inv, before)
