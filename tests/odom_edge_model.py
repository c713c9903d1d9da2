"""Odometry edges from the scans' own covariances (include/liodom_hip.h "odometry edges from the scans' own covariances";
liodom_math.h "Odometry edges from the scans' covariances"; kernels_odom_edges.h) restated in float64 NumPy.

Two restatements.  chain() is the library's arithmetic operation for operation — scalar float64, every sum in the library's order,
the 64 lanes and the tree that combines them — so Z, Sigma and Sigma_e can be compared with the library's as bits; Omega is
np.linalg.inv of Sigma_e (the library's is a Cholesky inverse: they agree to rounding x condition).  chain_dense() is the same
definition in matrix form, T (inflation C + F) T^T summed in scan order, for the checks that need no bits: the Monte-Carlo
simulation and the invariance under a change of frame.  No GPU, no library call (api is imported for the record layouts)."""
import math

import numpy as np

from liodom_amd import api

VALID, GAPS, NOT_PD, NO_POSE = 1, 2, 4, 8


# ---------------------------------------------------------------------------------------------
# the library's scalar arithmetic (pg_quat_mul, pg_rot3, the B of graph_edge_error), in its order
# ---------------------------------------------------------------------------------------------
def qmul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def rot3(q):
    x, y, z, w = q[0], q[1], q[2], q[3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1 - (txx + tyy)]


def pose_in(X):
    """The pose with its quaternion divided by its norm, and whether every entry of the result is finite."""
    X = [np.float64(v) for v in X]
    n = np.sqrt(((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]) + X[3] * X[3])
    with np.errstate(all="ignore"):
        out = [X[i] / n if i < 4 else X[i] for i in range(7)]
    return out, all(math.isfinite(v) for v in out)


def relative_pose(Xa, Xb):
    """Z = X_a^-1 o X_b of two poses already taken in."""
    z = qmul([-Xa[0], -Xa[1], -Xa[2], Xa[3]], Xb[:4])
    Ra = rot3(Xa)
    d = [Xb[4] - Xa[4], Xb[5] - Xa[5], Xb[6] - Xa[6]]
    return z + [Ra[r] * d[0] + Ra[3 + r] * d[1] + Ra[6 + r] * d[2] for r in range(3)]


def jacobian_j(Xi, Xj, Z):
    """B = de / d(delta_j) of graph_edge_error, 6 x 6 as nested lists."""
    Ri, Rz = rot3(Xi), rot3(Z)
    a = qmul([-Z[0], -Z[1], -Z[2], Z[3]], [-Xi[0], -Xi[1], -Xi[2], Xi[3]])
    qd = qmul(a, Xj[:4])
    s = 1.0 if qd[3] >= 0.0 else -1.0
    B = [[0.0] * 6 for _ in range(6)]
    for k in range(3):
        ek = [1.0 if k == 0 else 0.0, 1.0 if k == 1 else 0.0, 1.0 if k == 2 else 0.0, 0.0]
        d = qmul(qmul(a, ek), Xj[:4])
        for r in range(3):
            B[r][k] = s * d[r]
    for r in range(3):
        for c in range(3):
            B[3 + r][3 + c] = Rz[r] * Ri[c * 3] + Rz[3 + r] * Ri[c * 3 + 1] + Rz[6 + r] * Ri[c * 3 + 2]
    return B


# ---------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------
def lt(r, c):
    return r * (r + 1) // 2 + c            # packed lower triangle, c <= r


def sym(r, c):
    return lt(r, c) if r >= c else lt(c, r)


def usable(rec, k):
    return int(rec["scan_index"]) == k and int(rec["flags"]) == api.COV_VALID and bool(np.isfinite(rec["covariance"]).all())


def transport_term(C, u, inflation, fr2, ft2):
    """M_k as its 21 lower-triangle entries: T (inflation C + F) T^T, T = [[I, 0], [G, I]], G = -2 [u]x; the lower triangle of C is
    read.  M_rr = P_rr, N = M_tr = G P_rr + P_tr, M_tt = (N G^T + G P_rt) + P_tt; the sums run over the zeros of G too, from 0."""
    C = np.asarray(C, np.float64).reshape(6, 6)
    P = [0.0] * 21
    for r in range(6):
        for c in range(r + 1):
            P[lt(r, c)] = inflation * C[r, c] + (fr2 if r < 3 else ft2) if r == c else inflation * C[r, c]
    g0, g1, g2 = 2.0 * u[0], 2.0 * u[1], 2.0 * u[2]
    G = [0.0, g2, -g1, -g2, 0.0, g0, g1, -g0, 0.0]
    M = [0.0] * 21
    N = [0.0] * 9
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += G[i * 3 + k] * P[sym(k, j)]
            N[i * 3 + j] = s + P[lt(3 + i, j)]
            M[lt(3 + i, j)] = N[i * 3 + j]
            if j <= i:
                M[lt(i, j)] = P[lt(i, j)]
    for i in range(3):
        for j in range(i + 1):
            s1 = s2 = 0.0
            for k in range(3):
                s1 += N[i * 3 + k] * G[j * 3 + k]
                s2 += G[i * 3 + k] * P[lt(3 + j, k)]
            M[lt(3 + i, 3 + j)] = (s1 + s2) + P[lt(3 + i, 3 + j)]
    return M


def lane_partial(poses, recs, a, b, lane, inflation, fr2, ft2):
    """What lane `lane` of 64 accumulates: 21 sums over its scans k = lane (mod 64), a < k <= b, ascending, then the usable, the
    unusable and the non-finite-pose scans it met."""
    acc = [np.float64(0.0)] * 24
    tb = [np.float64(v) for v in poses[b][4:7]]
    k = a + 1 + ((lane - (a + 1)) % 64)
    while k <= b:
        X = [np.float64(v) for v in poses[k]]
        pose_ok = all(math.isfinite(v) for v in X)
        ok = usable(recs[k], k)
        acc[21 if ok else 22] += 1.0
        if not pose_ok:
            acc[23] += 1.0
        if ok and pose_ok:
            M = transport_term(recs[k]["covariance"], [tb[0] - X[4], tb[1] - X[5], tb[2] - X[6]], inflation, fr2, ft2)
            for i in range(21):
                acc[i] = acc[i] + M[i]
        k += 64
    return acc


def combine64(v):
    """The fixed tree in which the 64 lanes' partials of one entry are added."""
    p = [v[r] + v[r + 32] for r in range(32)]
    p = [p[r] + p[r + 16] for r in range(16)]
    p = [p[r] + p[15 - r] for r in range(8)]
    p = [p[r] + p[7 - r] for r in range(4)]
    p = [p[r] + p[r + 2] for r in range(2)]
    return p[0] + p[1]


def edge_covariance(B, S21):
    """B Sigma B^T, the upper triangle computed and mirrored."""
    T = [[0.0] * 6 for _ in range(6)]
    for r in range(6):
        for c in range(6):
            s = 0.0
            for k in range(6):
                s += B[r][k] * S21[sym(k, c)]
            T[r][c] = s
    Se = np.zeros((6, 6))
    for r in range(6):
        for c in range(r, 6):
            s = 0.0
            for k in range(6):
                s += T[r][k] * B[c][k]
            Se[r, c] = Se[c, r] = s
    return Se


def chain(poses, recs, a, b, inflation=1.0, floor_rotation=0.0, floor_translation=0.0):
    """The record of interval (a, b) -> dict(flags, n_used, n_missing, z (7,), sigma [6, 6] (the chained covariance in world
    coordinates; not part of the library's record), covariance = Sigma_e, information = Omega), NaN where the library writes NaN."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    with np.errstate(all="ignore"):
        parts = [lane_partial(poses, recs, a, b, lane, inflation, floor_rotation * floor_rotation, floor_translation * floor_translation)
                 for lane in range(64)]
        tot = [combine64([parts[lane][e] for lane in range(64)]) for e in range(24)]
    n_used, n_missing = int(tot[21]), int(tot[22])
    sigma = np.array([[tot[sym(r, c)] for c in range(6)] for r in range(6)], np.float64)
    Xa, oka = pose_in(poses[a])
    Xb, okb = pose_in(poses[b])
    out = dict(flags=NO_POSE, n_used=n_used, n_missing=n_missing, z=np.full(7, np.nan), sigma=sigma, covariance=np.full((6, 6), np.nan),
               information=np.full((6, 6), np.nan))
    if not (oka and okb and tot[23] == 0.0):
        return out
    Z = relative_pose(Xa, Xb)
    out["z"] = np.array(Z, np.float64)
    out["flags"] = GAPS if n_missing > 0 else 0
    pd = False
    if n_used > 0:
        with np.errstate(all="ignore"):
            Se = edge_covariance(jacobian_j(Xa, Xb, Z), tot)
        try:
            np.linalg.cholesky(Se)
            Om = np.linalg.inv(Se)
            pd = bool(np.isfinite(Om).all())
        except np.linalg.LinAlgError:
            pd = False
        if pd:
            out["covariance"], out["information"] = Se, 0.5 * (Om + Om.T)
    out["flags"] |= VALID if pd else NOT_PD
    return out


# ---------------------------------------------------------------------------------------------
# the same definition in matrix form
# ---------------------------------------------------------------------------------------------
def skew(u):
    return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])


def transport(u, lever_sign=1.0):
    """T_k = [[I, 0], [-2 [u]x, I]]; lever_sign = -1 is the wrong sign, the control of the Monte-Carlo check."""
    T = np.eye(6)
    T[3:, :3] = -2.0 * lever_sign * skew(u)
    return T


def chain_dense(poses, covs, a, b, inflation=1.0, floor_rotation=0.0, floor_translation=0.0, lever_sign=1.0):
    """(Sigma, Sigma_e, Omega) of interval (a, b), every scan usable: covs [m, 6, 6]."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    F = np.diag([floor_rotation ** 2] * 3 + [floor_translation ** 2] * 3)
    S = np.zeros((6, 6))
    for k in range(a + 1, b + 1):
        T = transport(poses[b, 4:] - poses[k, 4:], lever_sign)
        S += T @ (inflation * np.asarray(covs[k], np.float64) + F) @ T.T
    Xa, Xb = pose_in(poses[a])[0], pose_in(poses[b])[0]
    B = np.array(jacobian_j(Xa, Xb, relative_pose(Xa, Xb)), np.float64)
    Se = B @ S @ B.T
    Se = 0.5 * (Se + Se.T)
    return S, Se, np.linalg.inv(Se)


# ---------------------------------------------------------------------------------------------
# designed inputs
# ---------------------------------------------------------------------------------------------
def records(covs, flags=None, scan_index=None):
    """POSE_COV_DTYPE records with the given covariances [m, 6, 6]; flags default COV_VALID, scan_index default k; the other
    fields are zero (the chain reads none of them)."""
    covs = np.asarray(covs, np.float64).reshape(-1, 6, 6)
    r = np.zeros(covs.shape[0], api.POSE_COV_DTYPE)
    r["covariance"] = covs
    r["flags"] = api.COV_VALID if flags is None else flags
    r["scan_index"] = np.arange(covs.shape[0]) if scan_index is None else scan_index
    return r


def designed_stream(m, seed=0, sigma_r=1e-3, sigma_t=3e-3):
    """m scans along a bending path, about 0.5 m and 0.03 rad apart with seeded jitter, and a symmetric positive definite
    covariance per scan: D (I + 0.3 E) D with D = diag(sigma_r x 3, sigma_t x 3) and E a seeded correlation-like matrix — well
    conditioned, so that Sigma_e of any interval of up to ~150 scans keeps its condition number below 1e6 -> (poses [m, 7],
    covs [m, 6, 6])."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((m, 7))
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    D = np.diag([sigma_r] * 3 + [sigma_t] * 3)
    covs = np.zeros((m, 6, 6))
    for k in range(m):
        poses[k, :4], poses[k, 4:] = q, t
        A = rng.normal(size=(6, 6))
        E = A @ A.T / 6.0
        E = E / np.sqrt(np.outer(np.diag(E), np.diag(E)))
        C = D @ (0.7 * np.eye(6) + 0.3 * E) @ D
        covs[k] = 0.5 * (C + C.T)
        w = np.array([0.002, -0.001, 0.015]) + rng.normal(scale=0.002, size=3)         # half-angle step
        dq = np.concatenate([np.sin(np.linalg.norm(w)) * w / np.linalg.norm(w), [np.cos(np.linalg.norm(w))]])
        R = np.array(rot3(q)).reshape(3, 3)
        t = t + R @ (np.array([0.5, 0.0, 0.02]) + rng.normal(scale=0.05, size=3))
        q = np.array(qmul(q, dq))
        q = q / np.linalg.norm(q)
    return poses, covs
