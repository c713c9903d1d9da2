"""The pose graph (include/liodom_hip.h "closing loops"; liodom_math.h "Pose graph"; kernels_graph.h) restated in float64 NumPy:
the error of an edge, its analytic Jacobians, what an edge gives the normal equations, the node sums — each beside the same sum
over the absolute values of the products it is made of, which is what a rounding bound scales with —, H x, and a dense Levenberg-Marquardt with
the library's rules.  Also the designed graphs of the tests.  No GPU, no library call (api is imported for the record layout)."""
import math

import numpy as np

from liodom_amd import api

OMEGA = np.diag([400.0, 400.0, 400.0, 100.0, 100.0, 100.0])        # rotation (half angle) first, then translation


# ---------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose(q, t):
    q = np.asarray(q, np.float64)
    return np.concatenate([q / np.linalg.norm(q), np.asarray(t, np.float64)])


def compose(X, Y):
    return np.concatenate([qmul(X[:4], Y[:4]), rot(X[:4]) @ Y[4:] + X[4:]])


def inverse(X):
    return np.concatenate([qconj(X[:4]), -(rot(X[:4]).T @ X[4:])])


def between(Xi, Xj):
    """X_i^-1 o X_j: what an ideal edge (i, j) measures."""
    return compose(inverse(Xi), Xj)


def expq(d):
    """[sin|d| d/|d|, cos|d|]"""
    d = np.asarray(d, np.float64)
    n = float(np.linalg.norm(d))
    if n == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([math.sin(n) * d / n, [math.cos(n)]])


def retract(X, delta):
    q = qmul(expq(delta[:3]), X[:4])
    return np.concatenate([q / np.linalg.norm(q), X[4:] + delta[3:]])


def from_axis_angle(axis, angle, t=(0.0, 0.0, 0.0)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return pose(np.concatenate([math.sin(angle / 2.0) * a, [math.cos(angle / 2.0)]]), t)


def pose_distance(a, b):
    """(metres, radians) between two poses."""
    dot = min(1.0, abs(float(np.dot(a[:4], b[:4]))))
    return float(np.linalg.norm(a[4:] - b[4:])), 2.0 * math.acos(dot)


# ---------------------------------------------------------------------------------------------
# one edge
# ---------------------------------------------------------------------------------------------
def edge_error(Xi, Xj, Z):
    D = compose(inverse(Z), between(Xi, Xj))
    s = 1.0 if D[3] >= 0.0 else -1.0
    return np.concatenate([s * D[:3], D[4:]])


def _left(q):
    """L(q) p = q (x) p, as a 4 x 4 matrix on [x y z w]."""
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def _right(q):
    """R(q) p = p (x) q."""
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def skew(u):
    return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])


def edge_jacobians(Xi, Xj, Z):
    """e, A = de/d(delta_i), B = de/d(delta_j) at delta = 0, exact."""
    e = edge_error(Xi, Xj, Z)
    a = qmul(qconj(Z[:4]), qconj(Xi[:4]))
    qd = qmul(a, Xj[:4])
    s = 1.0 if qd[3] >= 0.0 else -1.0
    Q = s * (_left(a) @ _right(Xj[:4]))[:3, :3]          # d vec(a (x) [d, .] (x) q_j) / dd
    Wm = rot(Z[:4]).T @ rot(Xi[:4]).T
    u = Xj[4:] - Xi[4:]
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    A[:3, :3], B[:3, :3] = -Q, Q
    A[3:, :3] = 2.0 * Wm @ skew(u)
    A[3:, 3:], B[3:, 3:] = -Wm, Wm
    return e, A, B


def numeric_jacobians(Xi, Xj, Z, h=1e-6):
    """Central differences of the error through the retraction."""
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        A[:, k] = (edge_error(retract(Xi, d), Xj, Z) - edge_error(retract(Xi, -d), Xj, Z)) / (2.0 * h)
        B[:, k] = (edge_error(Xi, retract(Xj, d), Z) - edge_error(Xi, retract(Xj, -d), Z)) / (2.0 * h)
    return A, B


def edge_scale(Xi, Xj, Z):
    """1 + |t_j - t_i| + |t_z|: what the rounding of an edge's quantities scales with."""
    return 1.0 + float(np.linalg.norm(Xj[4:] - Xi[4:])) + float(np.linalg.norm(Z[4:]))


# ---------------------------------------------------------------------------------------------
# the graph
# ---------------------------------------------------------------------------------------------
def normalised(poses):
    p = np.array(poses, np.float64).reshape(-1, 7)
    p[:, :4] /= np.linalg.norm(p[:, :4], axis=1, keepdims=True)
    return p


def linearize(poses, fixed, edges):
    """dict: e [E, 6], A, B [E, 6, 6], chi2 (E,), gi, gj [E, 6], Hii, Hij, Hjj [E, 6, 6]; per node in edge order g [N, 6], D
    [N, 6, 6] and the same sums over absolute values g_abs, D_abs; scale (E,) = edge_scale.  g of a fixed node is 0.
    The absolute values are those of the PRODUCTS a sum is made of — an entry of a node sum is a sum over its edges of 36
    products J_ka Omega_kl e_l (or J_ka Omega_kl J_lb), so g_abs = sum |J|^T |Omega| |e| and D_abs = sum |J|^T |Omega| |J| — because
    that is what a rounding error scales with.  The absolute value of an edge's finished entry does not: W^T (100 I) W is 100 I,
    its off-diagonal entries are what is left of products of size 100 after they cancel, 1e-14, and no two summation orders —
    NumPy's and NumPy's — agree on them to 1e-12 of themselves."""
    poses = normalised(poses)
    N, E = poses.shape[0], len(edges)
    out = dict(e=np.zeros((E, 6)), A=np.zeros((E, 6, 6)), B=np.zeros((E, 6, 6)), chi2=np.zeros(E), gi=np.zeros((E, 6)), gj=np.zeros((E, 6)),
               Hii=np.zeros((E, 6, 6)), Hij=np.zeros((E, 6, 6)), Hjj=np.zeros((E, 6, 6)), g=np.zeros((N, 6)), D=np.zeros((N, 6, 6)),
               g_abs=np.zeros((N, 6)), D_abs=np.zeros((N, 6, 6)), scale=np.zeros(E), degree=np.zeros(N, np.int64))
    for k, ed in enumerate(edges):
        i, j = int(ed["i"]), int(ed["j"])
        Z = normalised(ed["z"])[0]
        Om = np.asarray(ed["info"], np.float64).reshape(6, 6)
        e, A, B = edge_jacobians(poses[i], poses[j], Z)
        out["e"][k], out["A"][k], out["B"][k] = e, A, B
        out["scale"][k] = edge_scale(poses[i], poses[j], Z)
        out["chi2"][k] = e @ Om @ e
        out["gi"][k], out["gj"][k] = A.T @ Om @ e, B.T @ Om @ e
        out["Hii"][k], out["Hij"][k], out["Hjj"][k] = A.T @ Om @ A, A.T @ Om @ B, B.T @ Om @ B
        aO, ae = np.abs(Om), np.abs(e)
        for n, gk, Hk, J in ((i, out["gi"][k], out["Hii"][k], np.abs(A)), (j, out["gj"][k], out["Hjj"][k], np.abs(B))):
            out["g"][n] += gk
            out["g_abs"][n] += J.T @ aO @ ae
            out["D"][n] += Hk
            out["D_abs"][n] += J.T @ aO @ J
            out["degree"][n] += 1
    fx = np.asarray(fixed).reshape(-1) != 0
    out["g"][fx] = 0.0
    return out


def multiply(lin, fixed, edges, x, lam=0.0):
    """y = (H + lam diag H) x with the fixed rows and columns dropped, and y_abs, the same sums over absolute values of the
    products.  A free node without edges: y = x."""
    fx = np.asarray(fixed).reshape(-1) != 0
    x = np.asarray(x, np.float64).reshape(-1, 6)
    N = x.shape[0]
    y, y_abs = np.zeros((N, 6)), np.zeros((N, 6))
    for n in range(N):
        if fx[n]:
            continue
        if lin["degree"][n] == 0:
            y[n], y_abs[n] = x[n], np.abs(x[n])
            continue
        Dn = lin["D"][n] + lam * np.diag(np.diag(lin["D"][n]))
        y[n] += Dn @ x[n]
        y_abs[n] += np.abs(Dn) @ np.abs(x[n])
    for k, ed in enumerate(edges):
        i, j = int(ed["i"]), int(ed["j"])
        if fx[i] or fx[j]:
            continue
        y[i] += lin["Hij"][k] @ x[j]
        y_abs[i] += np.abs(lin["Hij"][k]) @ np.abs(x[j])
        y[j] += lin["Hij"][k].T @ x[i]
        y_abs[j] += np.abs(lin["Hij"][k]).T @ np.abs(x[i])
    return y, y_abs


def dense(lin, edges):
    """H [6N, 6N] and g (6N,), nothing dropped."""
    N = lin["g"].shape[0]
    Hm = np.zeros((6 * N, 6 * N))
    for n in range(N):
        Hm[6 * n:6 * n + 6, 6 * n:6 * n + 6] = lin["D"][n]
    for k, ed in enumerate(edges):
        i, j = int(ed["i"]), int(ed["j"])
        Hm[6 * i:6 * i + 6, 6 * j:6 * j + 6] += lin["Hij"][k]
        Hm[6 * j:6 * j + 6, 6 * i:6 * i + 6] += lin["Hij"][k].T
    return Hm, lin["g"].reshape(-1).copy()


def chi2(poses, edges):
    poses = normalised(poses)
    total = 0.0
    for ed in edges:
        e = edge_error(poses[int(ed["i"])], poses[int(ed["j"])], normalised(ed["z"])[0])
        total += e @ np.asarray(ed["info"], np.float64).reshape(6, 6) @ e
    return float(total)


def lm(poses, fixed, edges, max_iterations=20, gradient_tolerance=1e-9, cost_tolerance=1e-10, trace=None):
    """The library's Levenberg-Marquardt with a dense solve in place of the conjugate gradients -> (poses, report dict with
    initial_cost, final_cost, max_gradient, final_lambda, iterations, accepted_steps, termination, costs = chi2 after each
    accepted step).  trace (a list): gets ("gradient", max |g|) wherever the library would launch a solve and ("cost", chi2 of the
    candidate) after every step tried, in order."""
    trace = [] if trace is None else trace
    poses = normalised(poses)
    fx = np.asarray(fixed).reshape(-1) != 0
    N = poses.shape[0]
    free = np.repeat(~fx, 6)
    lin = linearize(poses, fixed, edges)
    cost = float(np.sum(lin["chi2"]))
    rep = dict(initial_cost=cost, final_cost=cost, max_gradient=0.0, final_lambda=1e-4, iterations=0, accepted_steps=0, termination="gradient", costs=[cost])
    if not np.any(~fx) or len(edges) == 0:
        return poses, rep
    lam = 1e-4
    while True:
        Hm, g = dense(lin, edges)
        rep["max_gradient"] = float(np.max(np.abs(g[free])))
        trace.append(("gradient", rep["max_gradient"]))
        if rep["max_gradient"] <= gradient_tolerance:
            rep["termination"] = "gradient"
            break
        if rep["iterations"] >= max_iterations:
            rep["termination"] = "max_iterations"
            break
        Hf = Hm[np.ix_(free, free)]
        iso = np.diag(Hf) == 0.0
        Hf = Hf + lam * np.diag(np.diag(Hf)) + np.diag(iso.astype(np.float64))
        try:
            np.linalg.cholesky(Hf)
        except np.linalg.LinAlgError:
            rep["termination"] = "breakdown"
            break
        delta = np.zeros(6 * N)
        delta[free] = np.linalg.solve(Hf, -g[free])
        rep["iterations"] += 1
        cand = np.stack([retract(poses[n], delta[6 * n:6 * n + 6]) if not fx[n] else poses[n] for n in range(N)])
        c = chi2(cand, edges)
        trace.append(("cost", c))
        if c < cost:
            decrease = (cost - c) / cost
            poses, cost = cand, c
            rep["accepted_steps"] += 1
            rep["costs"].append(c)
            lam = max(lam / 10.0, 1e-12)
            rep["final_lambda"], rep["final_cost"] = lam, c
            lin = linearize(poses, fixed, edges)
            if decrease <= cost_tolerance:
                Hm, g = dense(lin, edges)
                rep["max_gradient"] = float(np.max(np.abs(g[free])))
                trace.append(("gradient", rep["max_gradient"]))
                rep["termination"] = "cost"
                break
        else:
            lam *= 10.0
            rep["final_lambda"] = lam
            if lam > 1e12:
                rep["termination"] = "lambda"
                break
    return poses, rep


# ---------------------------------------------------------------------------------------------
# designed graphs
# ---------------------------------------------------------------------------------------------
def random_pose(rng, spread=10.0):
    return pose(rng.normal(size=4), rng.normal(scale=spread, size=3))


def drifted_ring(n, n_loops=1, seed=0, info=OMEGA):
    """A ring of n key frames 1 m apart, driven once around: ground truth, the dead-reckoned poses of an odometry with a constant
    bias and seeded noise, the odometry edges 0-1, 1-2, ... and n_loops ideal loop edges from the last nodes back to the first
    -> (gt [n, 7], init [n, 7], fixed (n,), edges).  The bias is what the CPU oracle shows on the project's circle, whatever n:
    about 0.10 rad and 2 m off after one lap (2.06 m and 0.10 rad there, most of it in z, roll and pitch), i.e. per step a
    rotation of 0.10 / n rad about (0.6, 0.6, 0.5) — half of it in the half-angle tangent — and (0.6, 0.3, 1.9) / n m; the noise
    per step is a tenth of a lap's bias over sqrt(n)."""
    rng = np.random.default_rng(seed)
    R = n / (2.0 * math.pi)
    gt = np.stack([from_axis_angle((0, 0, 1), 2.0 * math.pi * k / n + math.pi / 2.0,
                                   (R * math.cos(2.0 * math.pi * k / n), R * math.sin(2.0 * math.pi * k / n), 0.0)) for k in range(n)])
    axis = np.array([0.6, 0.6, 0.5]) / np.linalg.norm([0.6, 0.6, 0.5])
    bias = np.concatenate([0.5 * 0.10 * axis, [0.6, 0.3, 1.9]]) / n
    sigma = np.array([0.005] * 3 + [0.2] * 3) / math.sqrt(n)
    init, zs = [gt[0]], []
    for k in range(1, n):
        Z = retract(between(gt[k - 1], gt[k]), bias + rng.normal(scale=sigma))
        zs.append(Z)
        init.append(compose(init[-1], Z))
    ii, jj = list(range(n - 1)), list(range(1, n))
    kinds = [0] * (n - 1)
    for k in range(n_loops):
        i, j = n - 1 - k * max(1, n // 16), k * max(1, n // 16)
        if i <= j + 1:
            break
        ii.append(i); jj.append(j); kinds.append(1)
        zs.append(between(gt[i], gt[j]))
    edges = api.graph_edges(ii, jj, np.stack(zs), info)
    edges["kind"] = kinds
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    return gt, np.stack(init), fixed, edges


def chain(n, seed=0, loop=True, info=OMEGA):
    """n nodes in a line 1 m apart with seeded pose noise, node 0 fixed, edges k - (k + 1) and, with loop and n > 2, one from the
    last node to the first -> (poses, fixed, edges)."""
    rng = np.random.default_rng(seed)
    gt = np.stack([from_axis_angle((0, 0, 1), 0.01 * k, (float(k), 0.0, 0.0)) for k in range(n)])
    poses = np.stack([retract(gt[k], rng.normal(scale=[2e-3] * 3 + [2e-2] * 3)) for k in range(n)])
    ii, jj = list(range(n - 1)), list(range(1, n))
    if loop and n > 2:
        ii.append(n - 1); jj.append(0)
    zs = np.stack([between(gt[i], gt[j]) for i, j in zip(ii, jj)]) if ii else np.zeros((0, 7))
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    return poses, fixed, api.graph_edges(ii, jj, zs, info)


def hub(degree, side, seed=0, info=None):
    """A hub (node 0) with `degree` edges to nodes 1 .. degree, the hub as every edge's i (side 0) or j (side 1); random poses,
    measurements and — info None — a random symmetric positive definite, non-diagonal Omega per edge."""
    rng = np.random.default_rng(seed)
    poses = np.stack([random_pose(rng) for _ in range(degree + 1)])
    zs = np.stack([random_pose(rng, 3.0) for _ in range(degree)])
    if info is None:
        M = rng.normal(size=(degree, 6, 6))
        info = M @ np.transpose(M, (0, 2, 1)) + 6.0 * np.eye(6)
        info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    hubs, leaves = [0] * degree, list(range(1, degree + 1))
    edges = api.graph_edges(hubs if side == 0 else leaves, leaves if side == 0 else hubs, zs, info)
    return poses, np.zeros(degree + 1, np.int32), edges


def jacobian_cases():
    """[(name, Xi, Xj, Z)]: random edges, a zero error on either sign of w_d, w_d < 0 away from zero, translations of 100 km."""
    rng = np.random.default_rng(11)
    cases = []
    for k in range(6):
        cases.append(("random%d" % k, random_pose(rng), random_pose(rng), random_pose(rng, 3.0)))
    Xi, Xj = random_pose(rng), random_pose(rng)
    Z = between(Xi, Xj)
    cases.append(("zero_error", Xi, Xj, Z))
    cases.append(("zero_error_w_negative", Xi, Xj, np.concatenate([-Z[:4], Z[4:]])))
    # w_d < 0 away from zero: the measurement is the true one turned by 4 rad, the long way round
    Zt = compose(Z, from_axis_angle((0.3, -0.5, 0.8), 4.0))
    cases.append(("w_negative", Xi, Xj, Zt))
    far_i = pose(rng.normal(size=4), [1e5, -2e4, 3e3])
    far_j = pose(rng.normal(size=4), [-4e4, 7e4, -1e3])
    cases.append(("100km", far_i, far_j, pose(rng.normal(size=4), [-9e4, 3e4, 2e3])))
    cases.append(("100km_zero_error", far_i, far_j, between(far_i, far_j)))
    return cases
