"""Robust losses and switched-off edges of the pose graph (include/liodom_hip.h "closing loops", "robust losses"; liodom_math.h
graph_loss; kernels_graph.h k_graph_linearize<true>) restated in float64 NumPy on top of graph_model: the losses, the weighted
linearisation — every FINISHED per-edge entry times w, inactive edges left out —, H x, the cost, and a dense Levenberg-Marquardt
with the library's rules.  Also the designed graphs of the tests.  No GPU, no library call."""
import math

import numpy as np

import graph_model as gm

LOSSES = ("none", "huber", "cauchy", "geman_mcclure")
N_KINDS = 16


def loss(name, c, s):
    """(rho, w = d rho / d s) of one loss with scale c at s = e^T Omega e; s <= 0 is quadratic."""
    s, c = float(s), float(c)
    if name == "none" or not s > 0.0:
        return s, 1.0
    if name == "huber":
        r = math.sqrt(s)
        return (s, 1.0) if r <= c else (c * (2.0 * r - c), c / r)
    u = (s / c) / c
    if name == "cauchy":
        return c * (c * math.log1p(u)), 1.0 / (1.0 + u)
    if name == "geman_mcclure":
        q = 1.0 / (1.0 + u)
        return s * q, q * q
    raise ValueError(name)


def dw_ds(name, c, s):
    """d w / d s: what an error of s does to the weight."""
    s, c = float(s), float(c)
    if name == "none" or not s > 0.0:
        return 0.0
    if name == "huber":
        return 0.0 if s <= c * c else -0.5 * c / (s * math.sqrt(s))
    u = s / (c * c)
    if name == "cauchy":
        return -1.0 / ((1.0 + u) ** 2 * c * c)
    return -2.0 / ((1.0 + u) ** 3 * c * c)


def edge_error(Xi, Xj, Z):
    """graph_model.edge_error with the translation part taken as R_z^T (R_i^T (t_j - t_i) - t_z), the difference FIRST.
    graph_model composes X_i^-1 o X_j as R_i^T t_j + (-R_i^T t_i): two vectors as long as the poses are far from the origin, whose
    difference carries eps x that distance — 1e-13 at 1 km, against an error of centimetres.  That is nothing to a bound that
    scales with 1 + |t_j - t_i| + |t_z|, but a weight is a function of e^T Omega e itself, and a model that is to hold a weighted
    H x to 1e-12 needs its s to 1e-12: t_j - t_i of two neighbouring key frames is exact (Sterbenz), the rest is of the size of
    the edge."""
    e = gm.edge_error(Xi, Xj, Z)
    m = gm.rot(Xi[:4]).T @ (Xj[4:] - Xi[4:]) - Z[4:]
    return np.concatenate([e[:3], gm.rot(Z[:4]).T @ m])


def edge_losses(edges, table):
    """Per edge (name, scale) from table = {kind: (name, scale)}; a kind outside 0 .. 15 or not in the table is quadratic."""
    out = []
    for ed in edges:
        k = int(ed["kind"])
        out.append(table.get(k, ("none", 1.0)) if 0 <= k < N_KINDS else ("none", 1.0))
    return out


def linearize(poses, fixed, edges, table=None, active=None):
    """graph_model.linearize with every finished per-edge entry (gi, gj, Hii, Hij, Hjj) multiplied by w = rho'(chi2) and the
    inactive edges left out of the node sums and degrees.  chi2 stays the raw s (inactive edges too); adds rho, w (0 for an
    inactive edge), and g_abs0 / D_abs0, the node sums of the unweighted absolute products times |1| per edge — what an error of
    w scales with.  g_abs, D_abs are the weighted ones.  e — and with it chi2, gi, gj — is this file's edge_error."""
    table = table or {}
    lin = gm.linearize(poses, fixed, edges)
    pn = gm.normalised(poses)
    for k, ed in enumerate(edges):
        Om = np.asarray(ed["info"], np.float64).reshape(6, 6)
        e = edge_error(pn[int(ed["i"])], pn[int(ed["j"])], gm.normalised(ed["z"])[0])
        lin["e"][k], lin["chi2"][k] = e, e @ Om @ e
        lin["gi"][k], lin["gj"][k] = lin["A"][k].T @ Om @ e, lin["B"][k].T @ Om @ e
    N, E = lin["g"].shape[0], len(edges)
    act = np.ones(E, bool) if active is None else np.asarray(active).reshape(-1) != 0
    names = edge_losses(edges, table)
    lin["rho"], lin["w"] = np.zeros(E), np.zeros(E)
    for k in ("g", "D", "g_abs", "D_abs"):
        lin[k] = np.zeros_like(lin[k])
    lin["g_abs0"], lin["D_abs0"] = np.zeros((N, 6)), np.zeros((N, 6, 6))
    lin["degree"] = np.zeros(N, np.int64)
    lin["active"] = act
    for k, ed in enumerate(edges):
        if not act[k]:
            for key in ("gi", "gj", "Hii", "Hij", "Hjj"):
                lin[key][k] = 0.0
            continue
        r, w = loss(names[k][0], names[k][1], lin["chi2"][k])
        lin["rho"][k], lin["w"][k] = r, w
        for key in ("gi", "gj", "Hii", "Hij", "Hjj"):
            lin[key][k] = lin[key][k] * w
        i, j = int(ed["i"]), int(ed["j"])
        Om = np.asarray(ed["info"], np.float64).reshape(6, 6)
        aO, ae = np.abs(Om), np.abs(lin["e"][k])
        for n, gk, Hk, J in ((i, lin["gi"][k], lin["Hii"][k], np.abs(lin["A"][k])), (j, lin["gj"][k], lin["Hjj"][k], np.abs(lin["B"][k]))):
            lin["g"][n] += gk
            lin["D"][n] += Hk
            lin["g_abs0"][n] += J.T @ aO @ ae
            lin["D_abs0"][n] += J.T @ aO @ J
            lin["g_abs"][n] += w * (J.T @ aO @ ae)
            lin["D_abs"][n] += w * (J.T @ aO @ J)
            lin["degree"][n] += 1
    fx = np.asarray(fixed).reshape(-1) != 0
    lin["g"][fx] = 0.0
    return lin


def multiply(lin, fixed, edges, x, lam=0.0):
    """graph_model.multiply on the weighted blocks; an inactive edge's Hij is 0 and its nodes do not count it as a neighbour."""
    return gm.multiply(lin, fixed, edges, x, lam)


def edge_costs(poses, edges, table=None, active=None):
    """(s, rho, w) per edge at poses; rho = w = 0 for an inactive edge."""
    table = table or {}
    poses = gm.normalised(poses)
    E = len(edges)
    act = np.ones(E, bool) if active is None else np.asarray(active).reshape(-1) != 0
    names = edge_losses(edges, table)
    s, rho, w = np.zeros(E), np.zeros(E), np.zeros(E)
    for k, ed in enumerate(edges):
        e = edge_error(poses[int(ed["i"])], poses[int(ed["j"])], gm.normalised(ed["z"])[0])
        s[k] = e @ np.asarray(ed["info"], np.float64).reshape(6, 6) @ e
        if act[k]:
            rho[k], w[k] = loss(names[k][0], names[k][1], s[k])
    return s, rho, w


def cost(poses, edges, table=None, active=None):
    """The sum of rho over the active edges."""
    return float(np.sum(edge_costs(poses, edges, table, active)[1]))


def lm(poses, fixed, edges, table=None, active=None, max_iterations=20, gradient_tolerance=1e-9, cost_tolerance=1e-10):
    """graph_model.lm — the library's schedule, a dense solve — on the weighted system and the robust cost."""
    poses = gm.normalised(poses)
    fx = np.asarray(fixed).reshape(-1) != 0
    N = poses.shape[0]
    free = np.repeat(~fx, 6)
    lin = linearize(poses, fixed, edges, table, active)
    c0 = float(np.sum(lin["rho"]))
    rep = dict(initial_cost=c0, final_cost=c0, max_gradient=0.0, final_lambda=1e-4, iterations=0, accepted_steps=0, termination="gradient", costs=[c0])
    if not np.any(~fx) or not np.any(lin["active"]):
        return poses, rep
    cur, lam = c0, 1e-4
    while True:
        Hm, g = gm.dense(lin, edges)
        rep["max_gradient"] = float(np.max(np.abs(g[free])))
        if rep["max_gradient"] <= gradient_tolerance:
            rep["termination"] = "gradient"
            break
        if rep["iterations"] >= max_iterations:
            rep["termination"] = "max_iterations"
            break
        Hf = Hm[np.ix_(free, free)]
        iso = np.repeat(lin["degree"] == 0, 6)[free]
        Hf = Hf + lam * np.diag(np.diag(Hf)) + np.diag(iso.astype(np.float64))
        try:
            np.linalg.cholesky(Hf)
        except np.linalg.LinAlgError:
            rep["termination"] = "breakdown"
            break
        delta = np.zeros(6 * N)
        delta[free] = np.linalg.solve(Hf, -g[free])
        rep["iterations"] += 1
        cand = np.stack([gm.retract(poses[n], delta[6 * n:6 * n + 6]) if not fx[n] else poses[n] for n in range(N)])
        c = cost(cand, edges, table, active)
        if c < cur:
            decrease = (cur - c) / abs(cur) if cur != 0.0 else 0.0
            poses, cur = cand, c
            rep["accepted_steps"] += 1
            rep["costs"].append(c)
            lam = max(lam / 10.0, 1e-12)
            rep["final_lambda"], rep["final_cost"] = lam, c
            lin = linearize(poses, fixed, edges, table, active)
            if decrease <= cost_tolerance:
                Hm, g = gm.dense(lin, edges)
                rep["max_gradient"] = float(np.max(np.abs(g[free])))
                rep["termination"] = "cost"
                break
        else:
            lam *= 10.0
            rep["final_lambda"] = lam
            if lam > 1e12:
                rep["termination"] = "lambda"
                break
    return poses, rep


def max_distance(a, b):
    """(metres, radians): the largest pose_distance over two sets of poses."""
    d = [gm.pose_distance(x, y) for x, y in zip(a, b)]
    return max(v[0] for v in d), max(v[1] for v in d)


# ---------------------------------------------------------------------------------------------
# designed graphs
# ---------------------------------------------------------------------------------------------
def ring_with_false_loop(n, n_loops, seed, step=1.0):
    """graph_model.drifted_ring(n, n_loops, seed) plus ONE false loop edge, the last edge: 3n/4 -> n/4 measured as the identity
    ("these two key frames are the same place" — they are a diameter apart), gm.OMEGA, kind 1 -> (gt, init, fixed, edges,
    false_index).  step: the ring rescaled to that distance between key frames (translations of poses and measurements alike; the
    information matrix is left as it is)."""
    gt, init, fixed, edges = gm.drifted_ring(n, n_loops, seed)
    false = gm.api.graph_edges([3 * n // 4], [n // 4], [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]], gm.OMEGA, kind=1)
    edges = np.concatenate([edges, false])
    if step != 1.0:
        gt, init, edges = gt.copy(), init.copy(), edges.copy()
        gt[:, 4:] *= step
        init[:, 4:] *= step
        edges["z"][:, 4:] *= step
    return gt, init, fixed, edges, len(edges) - 1


def clean(edges, false_index):
    """The edges without the false one."""
    return np.delete(edges, false_index)


def closer_ring(n=48, n_loops=2, seed=48, step=4.0):
    """ring_with_false_loop(n, n_loops, seed, step) as a LoopCloser holds it: every loop edge runs from the older key frame to the
    newer one — drifted_ring's true loops (i > j, Z) turned round to (j, i, Z^-1), the false one (n/4, 3n/4, identity) —, and the
    odometry edges measure what lies between consecutive dead-reckoned poses -> (init, fixed, edges, loops = [(place, node, Z)] in
    edge order, false_index)."""
    _, init, fixed, edges, fi = ring_with_false_loop(n, n_loops, seed, step)
    odo = [gm.between(init[k - 1], init[k]) for k in range(1, n)]
    loops = []
    for k in range(len(edges)):
        if int(edges["kind"][k]) != 1:
            continue
        i, j, Z = int(edges["i"][k]), int(edges["j"][k]), gm.normalised(edges["z"][k])[0]
        loops.append((j, i, gm.inverse(Z)) if i > j else (i, j, Z))
    out = gm.api.graph_edges(list(range(n - 1)) + [l[0] for l in loops], list(range(1, n)) + [l[1] for l in loops],
                             np.stack(odo + [l[2] for l in loops]), gm.OMEGA)
    out["kind"] = [0] * (n - 1) + [1] * len(loops)
    return init, fixed, out, loops, len(out) - 1
