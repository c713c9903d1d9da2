"""Pose covariance arithmetic (liodom_amd/csrc/liodom_math.h: spd_inverse6, sym_eig6, pose_cov_compute, pose_cov_to_ros — what
k_pose_cov runs on the device), compiled for the host by tests/covcheck.cc, against numpy and the oracle.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_oracle_odometry import _make_problem

HERE = os.path.dirname(os.path.abspath(__file__))
VALID, SINGULAR, NO_SOLVE, EVAL_FAILURE, FEW_RESIDUALS = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def cc():
    so = os.path.join(HERE, "libcovcheck.so")
    src = os.path.join(HERE, "covcheck.cc")
    hdr = os.path.join(HERE, "..", "liodom_amd", "csrc", "liodom_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.cc_inverse.restype = C.c_int
    L.cc_inverse.argtypes = [dp, dp]
    L.cc_eig.restype = C.c_int
    L.cc_eig.argtypes = [dp, dp, dp]
    L.cc_record.restype = C.c_uint
    L.cc_record.argtypes = [dp, C.c_double, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp]
    L.cc_to_ros.argtypes = [dp, dp, dp, dp]
    L.cc_iso_from_qt.argtypes = [dp, dp, dp]
    L.cc_information.argtypes = [dp, C.c_int, dp, dp, C.c_double, C.c_double, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


IU = np.triu_indices(6)       # row-major upper triangle = h_idx order


def _h21(A):
    return np.ascontiguousarray(A[IU], dtype=np.float64)


def _inverse(cc, A):
    out = np.zeros(36)
    ok = cc.cc_inverse(_dp(_h21(A)), _dp(out))
    return bool(ok), out.reshape(6, 6)


def _eig(cc, A):
    w, V = np.zeros(6), np.zeros(36)
    sweeps = cc.cc_eig(_dp(np.ascontiguousarray(A, dtype=np.float64)), _dp(w), _dp(V))
    return w, V.reshape(6, 6), sweeps


def _inverse_extended(A):
    """Gauss-Jordan with partial pivoting in numpy's extended precision (x87 80-bit on x86-64), rounded to FP64."""
    M = np.concatenate([A.astype(np.longdouble), np.eye(6, dtype=np.longdouble)], axis=1)
    for c in range(6):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] /= M[c, c]
        for r in range(6):
            if r != c:
                M[r] -= M[r, c] * M[c]
    return M[:, 6:].astype(np.float64)


def _spd(rng, cond):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    lam = np.geomspace(1.0, 1.0 / cond, 6) * 10.0 ** rng.uniform(-3, 3)
    rng.shuffle(lam)
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def test_inverse_and_eigen_decomposition_against_numpy(cc):
    rng = np.random.default_rng(11)
    conds = np.geomspace(1.0, 1e10, 200)
    for i, cond in enumerate(conds):
        A = _spd(rng, cond)
        w, V, sweeps = _eig(cc, A)
        wr, Vr = np.linalg.eigh(A)
        lmax = wr[-1]
        assert sweeps < 12, (i, cond)
        assert np.all(np.diff(w) >= 0), i
        assert np.max(np.abs(w - wr)) <= 1e-12 * lmax, (i, cond, np.max(np.abs(w - wr)) / lmax)
        assert np.allclose(np.linalg.norm(V, axis=0), 1.0, atol=1e-13)
        for j in range(6):
            gap = min([abs(wr[j] - wr[k]) for k in range(6) if k != j])
            if gap > 1e-6 * lmax:
                # (1e-10; near the 1e-6 gap the Davis-Kahan bound of an FP64 decomposition, eps ||A|| / gap, is larger: numpy's
                #  vectors are themselves only that accurate)
                v, vr = V[:, j], Vr[:, j]
                tol = max(1e-10, 4e-16 * lmax / gap)
                assert min(np.linalg.norm(v - vr), np.linalg.norm(v + vr)) <= tol, (i, j, cond)
            else:       # (near-degenerate: the pair spans the same subspace)
                cl = [k for k in range(6) if abs(wr[j] - wr[k]) <= 1e-6 * lmax]
                P = Vr[:, cl] @ Vr[:, cl].T
                assert np.linalg.norm(V[:, j] - P @ V[:, j]) <= 1e-8, (i, j)
        ok, X = _inverse(cc, A)
        if cond <= 1e8:
            # (at condition 1e8 numpy.linalg.inv itself is off by up to ~1e-9 of the norm — cond x eps: the reference is the inverse of
            #  the same FP64 matrix in extended precision, and numpy's is checked against it with the same bound)
            Xr = _inverse_extended(A)
            assert ok, (i, cond)
            assert np.array_equal(X, X.T)
            assert np.linalg.norm(X - Xr) <= 1e-9 * np.linalg.norm(Xr), (i, cond, np.linalg.norm(X - Xr) / np.linalg.norm(Xr))
            assert np.linalg.norm(X - np.linalg.inv(A)) <= 2e-9 * np.linalg.norm(Xr), (i, cond)


def test_sign_rule_is_deterministic(cc):
    rng = np.random.default_rng(5)
    A = _spd(rng, 1e3)
    w, V, _ = _eig(cc, A)
    for j in range(6):
        k = int(np.argmax(np.abs(V[:, j])))
        assert V[k, j] > 0
    # the same matrix with two basis vectors flipped: the vectors come back flipped the same way, each then signed by the rule
    D = np.diag([1.0, -1.0, 1.0, 1.0, -1.0, 1.0])
    w2, V2, _ = _eig(cc, D @ A @ D)
    assert np.allclose(w2, w, rtol=0, atol=1e-12 * w[-1])
    E = D @ V
    E *= np.sign(E[np.argmax(np.abs(E), axis=0), np.arange(6)])
    assert np.allclose(V2, E, rtol=0, atol=1e-10)
    # and identical input gives identical bits
    w3, V3, _ = _eig(cc, A)
    assert np.array_equal(w3, w) and np.array_equal(V3, V)


def _record(cc, H, cost, n, term, has_solve=1):
    s2 = np.zeros(1)
    info, cov, ev, evec = np.zeros(36), np.zeros(36), np.zeros(6), np.zeros(36)
    flags = cc.cc_record(_dp(_h21(H)), cost, n, term, has_solve, _dp(s2), _dp(info), _dp(cov), _dp(ev), _dp(evec))
    return flags, s2[0], info.reshape(6, 6), cov.reshape(6, 6), ev, evec.reshape(6, 6)


def test_singular_matrix_sets_the_flag_and_a_zero_eigenvalue(cc):
    rng = np.random.default_rng(2)
    A = _spd(rng, 10.0)
    A[4, :] = 0.0
    A[:, 4] = 0.0
    ok, _ = _inverse(cc, A)
    assert not ok
    flags, s2, info, cov, ev, evec = _record(cc, A, 3.0, 100, 2)
    assert flags == VALID | SINGULAR
    assert np.all(np.isnan(cov)) and s2 == pytest.approx(6.0 / 294.0)
    assert ev[0] == 0.0 and abs(evec[4, 0]) == 1.0
    assert np.array_equal(info, A)


def test_record_flags(cc):
    rng = np.random.default_rng(3)
    A = _spd(rng, 100.0)
    flags, s2, info, cov, ev, _ = _record(cc, A, 2.5, 500, 2)
    assert flags == VALID
    assert s2 == 2.0 * 2.5 / (3 * 500 - 6)
    assert np.allclose(cov, s2 * np.linalg.inv(A), rtol=1e-12, atol=0)
    for n in (0, 1, 2):
        flags, s2, _, cov, ev, _ = _record(cc, A, 1.0, n, 2)
        assert flags & FEW_RESIDUALS and np.isnan(s2) and np.all(np.isnan(cov)), n
        assert np.all(np.isfinite(ev)), n
    flags, s2, info, cov, ev, evec = _record(cc, A, 1.0, 500, 5)
    assert flags == EVAL_FAILURE and np.isnan(s2)
    assert all(np.all(np.isnan(x)) for x in (info, cov, ev, evec))
    flags, s2, info, cov, ev, evec = _record(cc, A, 0.0, 0, 4, has_solve=0)
    assert flags == NO_SOLVE and np.all(np.isnan(info))


def test_information_matches_oracle_autodiff(cc, orc):
    """The accumulator's analytic J^T J (what the LM controller holds) against sum rho' J^T J from the oracle's autodiff Jacobians."""
    rng = np.random.default_rng(9)
    blocks, q, t = _make_problem(rng, 200, outliers=10)
    q = q + np.array([1e-3, -2e-3, 5e-4, 0.0])
    q /= np.linalg.norm(q)
    t = t + np.array([0.02, -0.01, 0.005])
    H = np.zeros(21)
    cc.cc_information(_dp(np.ascontiguousarray(blocks)), len(blocks), _dp(q), _dp(t), 3.0, 75.0, _dp(H))
    Href = np.zeros((6, 6))
    for b in blocks:
        r, J, _ = orc.point2line(q, t, b[:3], b[3:6], b[6:9])
        s = float(r @ r)
        rho1 = 1.0 if s <= 0.04 else max(0.2 / np.sqrt(s), np.finfo(float).tiny)
        Href += rho1 * J.T @ J
    assert np.linalg.norm(_full(H) - Href) <= 1e-10 * np.linalg.norm(Href)


def _full(H21):
    A = np.zeros((6, 6))
    A[IU] = H21
    return A + np.triu(A, 1).T


def _rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rotvec(R):
    c = (np.trace(R) - 1.0) / 2.0
    ang = np.arccos(np.clip(c, -1.0, 1.0))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v * (0.5 if ang < 1e-12 else ang / (2.0 * np.sin(ang)))


@pytest.mark.parametrize("l2b", ["identity", "mounted"])
def test_ros_conversion_against_finite_differences(cc, orc, l2b):
    q = np.array([0.1, -0.2, 0.3, 0.9])
    q /= np.linalg.norm(q)
    t = np.array([4.0, -2.0, 0.7])
    T = np.zeros(12)
    cc.cc_iso_from_qt(_dp(q), _dp(t), _dp(T))
    if l2b == "identity":
        L = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    else:
        qL = np.array([0.05, 0.02, -0.7, 0.7])
        qL /= np.linalg.norm(qL)
        L = np.concatenate([np.c_[_rot(qL), [0.3, -0.15, 1.2]]]).reshape(12)
    RL, tL = L.reshape(3, 4)[:, :3], L.reshape(3, 4)[:, 3]
    R = _rot(q)
    RP, pP = R @ RL, R @ tL + t

    def f(x):
        q2 = orc.quat_plus(q, x[:3])
        R2 = _rot(q2)
        p2 = R2 @ tL + t + x[3:]
        return np.concatenate([p2 - pP, _rotvec(R2 @ RL @ RP.T)])

    h = 1e-6
    Jn = np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        Jn[:, k] = (f(e) - f(-e)) / (2 * h)
    rng = np.random.default_rng(4)
    M = rng.normal(size=(6, 6))
    S = M @ M.T
    out = np.zeros(36)
    cc.cc_to_ros(_dp(np.ascontiguousarray(S)), _dp(T), _dp(L), _dp(out))
    ref = Jn @ S @ Jn.T
    assert np.allclose(out.reshape(6, 6), ref, rtol=0, atol=1e-7 * np.abs(ref).max())
    # the rotation block is 4 x the tangent's: the tangent is a half-angle
    assert np.allclose(out.reshape(6, 6)[3:, 3:], 4.0 * S[:3, :3], rtol=1e-12, atol=0)
