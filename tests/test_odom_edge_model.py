"""The definition of the chained odometry covariance (tests/odom_edge_model.py) against a simulation, and its invariance.

Monte Carlo.  A 5-scan chain with random rotations and lever arms; scan k's solve errs by a world-frame tangent perturbation
(d, dt) ~ N(0, C_k) of X_k — q <- [sin|d| d/|d|, cos|d|] (x) q, t <- t + dt — and every later pose rides on it rigidly:
X_j <- (rotation by d about t_k, then dt) X_j for j >= k.  40 000 draws with a fixed seed, noise 1e-3 rad (half angle) and
3e-3 m; e is the error of the edge (X_0, X_5', Z_true).  The sample covariance of e must agree with Sigma_e to 3 % in Frobenius
norm: an entry's sampling error is sqrt(2 / N) = 0.7 %, and the second-order terms the linear model drops are 1e-3 of it.  With
the sign of [u]x flipped the model must be off by at least 20 %: the control that the check can see the lever arm at all.
The lever arms are about a metre (positions drawn with sigma 1 m), where the sign shows most: flipping it changes the
rotation-translation block, 2 |u| sigma_r^2 an entry, while the translation block, 4 |u|^2 sigma_r^2 + sigma_t^2, does not change —
the ratio falls like 1 / |u| for long arms and like |u| sigma_r^2 / sigma_t^2 for short ones.
Invariance.  Omega is unchanged to 1e-9 relative when every pose is left-composed with an arbitrary pose G (and the covariances,
which are world-frame quantities, are turned with it: C' = diag(R_G, R_G) C diag(R_G, R_G)^T).  No GPU."""
import numpy as np

import graph_model as gm
import odom_edge_model as om

N_DRAWS = 40000


def _qmul(a, b):
    """Rows of quaternions [n, 4] (x) rows [n, 4] (either may be one row)."""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def _rotate(q, v):
    """R(q) v for rows of unit quaternions and rows of vectors."""
    qv = np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], axis=-1)
    qc = q * np.array([-1.0, -1.0, -1.0, 1.0])
    return _qmul(_qmul(q, qv), qc)[..., :3]


def _expq(d):
    n = np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([np.sin(n) * d / n, np.cos(n)], axis=-1)


def _chain5(seed):
    rng = np.random.default_rng(seed)
    poses = np.stack([gm.pose(rng.normal(size=4), rng.normal(scale=1.0, size=3)) for _ in range(6)])
    D = np.diag([1e-3] * 3 + [3e-3] * 3)
    covs = np.zeros((6, 6, 6))
    for k in range(6):
        A = rng.normal(size=(6, 6))
        E = A @ A.T / 6.0
        E = E / np.sqrt(np.outer(np.diag(E), np.diag(E)))
        C = D @ (0.6 * np.eye(6) + 0.4 * E) @ D
        covs[k] = 0.5 * (C + C.T)
    return poses, covs


def _simulate(poses, covs, rng):
    """e [N_DRAWS, 6] of the edge (X_0, X_5 perturbed, Z true)."""
    q = np.repeat(poses[None, :, :4], N_DRAWS, axis=0)          # [N, 6, 4]
    t = np.repeat(poses[None, :, 4:], N_DRAWS, axis=0)          # [N, 6, 3]
    for k in range(1, 6):
        delta = rng.multivariate_normal(np.zeros(6), covs[k], size=N_DRAWS)
        dq = _expq(delta[:, :3])
        tk = t[:, k].copy()
        for j in range(k, 6):
            t[:, j] = tk + _rotate(dq, t[:, j] - tk) + delta[:, 3:]
            q[:, j] = _qmul(dq, q[:, j])
    Z = gm.between(poses[0], poses[5])
    # e = [s vec(q_d); t_d], D = Z^-1 o X_0^-1 o X_5'
    q0c = poses[0, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    zc = Z[:4] * np.array([-1.0, -1.0, -1.0, 1.0])
    qd = _qmul(_qmul(zc[None], q0c[None]), q[:, 5])
    m = _rotate(np.repeat(q0c[None], N_DRAWS, axis=0), t[:, 5] - poses[0, 4:]) - Z[4:]
    td = _rotate(np.repeat(zc[None], N_DRAWS, axis=0), m)
    s = np.where(qd[:, 3:4] >= 0.0, 1.0, -1.0)
    return np.concatenate([s * qd[:, :3], td], axis=1)


def test_monte_carlo_agrees_and_the_flipped_sign_does_not():
    poses, covs = _chain5(seed=12)
    e = _simulate(poses, covs, np.random.default_rng(2024))
    assert np.max(np.abs(e.mean(axis=0))) <= 5.0 * np.sqrt(np.max(np.diag(np.cov(e.T))) / N_DRAWS) + 1e-6
    sample = np.cov(e.T)
    _, Se, _ = om.chain_dense(poses, covs, 0, 5)
    _, Se_flipped, _ = om.chain_dense(poses, covs, 0, 5, lever_sign=-1.0)
    good = np.linalg.norm(Se - sample) / np.linalg.norm(sample)
    flipped = np.linalg.norm(Se_flipped - sample) / np.linalg.norm(sample)
    print("relative Frobenius error of Sigma_e against %d draws: %.4f; with the sign of [u]x flipped: %.4f" % (N_DRAWS, good, flipped))
    assert good <= 0.03
    assert flipped >= 0.20
    # the scalar restatement (the one compared with the library as bits) is the same definition
    m = om.chain(poses, om.records(covs), 0, 5)
    assert m["flags"] == om.VALID and np.linalg.norm(m["covariance"] - Se) <= 1e-12 * np.linalg.norm(Se)


def test_omega_does_not_depend_on_the_frame():
    poses, covs = om.designed_stream(40, seed=8)
    rng = np.random.default_rng(9)
    for trial in range(4):
        G = gm.pose(rng.normal(size=4), rng.normal(scale=50.0, size=3))
        RG = gm.rot(G[:4])
        R6 = np.zeros((6, 6))
        R6[:3, :3] = R6[3:, 3:] = RG
        moved = np.stack([gm.compose(G, p) for p in poses])
        turned = np.stack([R6 @ c @ R6.T for c in covs])
        turned = 0.5 * (turned + np.transpose(turned, (0, 2, 1)))
        for a, b in ((0, 1), (3, 20), (0, 39)):
            for options in (dict(), dict(inflation=3.0, floor_rotation=2e-4, floor_translation=1e-3)):
                want = om.chain(poses, om.records(covs), a, b, **options)
                got = om.chain(moved, om.records(turned), a, b, **options)
                assert want["flags"] == om.VALID and got["flags"] == om.VALID
                rel = np.linalg.norm(got["information"] - want["information"]) / np.linalg.norm(want["information"])
                assert rel <= 1e-9, (trial, a, b, rel)
                assert np.max(np.abs(got["z"] - want["z"])) <= 1e-12 * (1.0 + np.linalg.norm(G[4:]))
