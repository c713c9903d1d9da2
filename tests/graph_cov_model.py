"""Covariances of the pose graph and the loop gate (include/liodom_hip.h "covariances of the graph"; graph_marginals.h; the kernels
in kernels_graph.h) restated in float64 NumPy on top of graph_model.linearize / graph_model.dense (or their robust twins in
graph_robust_model): which nodes are anchored, the dense H over the free anchored nodes and its inverse, the statuses, the gate's
d2 — and the error bounds the GPU tests hold the library to, with the designed graphs they run on.  No GPU, no library call."""
import math

import numpy as np

import graph_model as gm
import graph_robust_model as grm

EPS = 2.0 ** -53
OK, NOT_CONVERGED, BREAKDOWN, UNANCHORED, NOT_PD = range(5)
CHI2_6_099 = 16.81          # the 0.99 quantile of chi-square with 6 degrees of freedom


def anchored(fixed, edges, active=None):
    """(N,) bool: the node's connected component over the active edges holds a fixed node (a fixed node is anchored)."""
    fx = np.asarray(fixed).reshape(-1) != 0
    N = fx.shape[0]
    act = np.ones(len(edges), bool) if active is None else np.asarray(active).reshape(-1) != 0
    root = list(range(N))

    def find(n):
        while root[n] != n:
            n = root[n]
        return n
    for k, ed in enumerate(edges):
        if act[k]:
            a, b = find(int(ed["i"])), find(int(ed["j"]))
            root[max(a, b)] = min(a, b)
    holds = {find(n) for n in range(N) if fx[n]}
    return np.array([find(n) in holds for n in range(N)], bool)


def full_matrix(lin, fixed, edges):
    """The matrix liodom_graph_multiply(g, 0, .) applies, dense [6N, 6N]: graph_model.dense with the rows and columns of fixed nodes
    0 and the identity on a free node without (active) edges.  lin of a graph with switched-off edges or losses: graph_robust_model's."""
    Hm, _ = gm.dense(lin, edges)
    fx = np.repeat(np.asarray(fixed).reshape(-1) != 0, 6)
    Hm[fx, :] = 0.0
    Hm[:, fx] = 0.0
    for n in np.nonzero(lin["degree"] == 0)[0]:
        if not fx[6 * n]:
            Hm[6 * n:6 * n + 6, 6 * n:6 * n + 6] = np.eye(6)
    return Hm


DENSE_LIMIT = 600          # unknowns up to which system() inverts H densely; beyond, a sparse LU gives the columns asked for


def system(lin, fixed, edges, active=None):
    """dict: nodes = the free anchored nodes, place[n] = a node's place among them (-1), H [6m, 6m] the dense matrix over them,
    pd = whether it is positive definite, anchored, fixed, and the norms the bounds use: norm_inv = |H^-1|_2, cond = kappa_2(H),
    norm_abs = | |H| |_2 of the full matrix, max_degree.  Up to DENSE_LIMIT unknowns Sigma = the dense inverse, symmetrised; beyond
    that Sigma is None, the extreme eigenvalues come from Lanczos (shift-invert at 0 for the smallest) and node_columns() solves
    with a sparse LU in float64 — the same H^-1, without the hour a dense 6000 x 6000 eigenproblem takes."""
    fx = np.asarray(fixed).reshape(-1) != 0
    anc = anchored(fixed, edges, active)
    nodes = np.nonzero(~fx & anc)[0]
    place = -np.ones(fx.shape[0], np.int64)
    place[nodes] = np.arange(nodes.shape[0])
    full = full_matrix(lin, fixed, edges)
    sel = (6 * nodes[:, None] + np.arange(6)[None, :]).reshape(-1)
    H = full[np.ix_(sel, sel)]
    H = 0.5 * (H + H.T)
    out = dict(nodes=nodes, place=place, H=H, full=full, anchored=anc, fixed=fx, Sigma=None, lu=None, cols={}, pd=False, norm_inv=float("nan"),
               cond=float("nan"), norm_abs=0.0, max_degree=int(np.max(lin["degree"])) if len(lin["degree"]) else 0)
    if full.shape[0] <= DENSE_LIMIT:
        out["norm_abs"] = float(np.linalg.norm(np.abs(full), 2)) if full.size else 0.0
        if H.size:
            w = np.linalg.eigvalsh(H)
            out["pd"] = bool(w[0] > 0.0)
            if out["pd"]:
                Sg = np.linalg.inv(H)
                out["Sigma"] = 0.5 * (Sg + Sg.T)
                out["norm_inv"], out["cond"] = 1.0 / float(w[0]), float(w[-1] / w[0])
        return out
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    out["norm_abs"] = float(spl.eigsh(sp.csr_matrix(np.abs(full)), k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])
    Hs = sp.csc_matrix(H)
    hi = float(spl.eigsh(Hs, k=1, which="LA", tol=1e-10, return_eigenvectors=False)[0])
    lo = float(spl.eigsh(Hs, k=1, sigma=0.0, which="LM", tol=1e-10, return_eigenvectors=False)[0])
    out["pd"] = lo > 0.0
    if out["pd"]:
        out["lu"] = spl.splu(Hs)
        out["norm_inv"], out["cond"] = 1.0 / lo, hi / lo
    return out


def node_columns(sysm, node):
    """The six columns of Sigma of a free anchored node over the free anchored nodes, [6m, 6]."""
    p = int(sysm["place"][node])
    if sysm["Sigma"] is not None:
        return sysm["Sigma"][:, 6 * p:6 * p + 6]
    if node not in sysm["cols"]:
        rhs = np.zeros((sysm["H"].shape[0], 6))
        rhs[6 * p + np.arange(6), np.arange(6)] = 1.0
        sysm["cols"][node] = sysm["lu"].solve(rhs)
    return sysm["cols"][node]


def column(sysm, node, b):
    """Column b of `node` of Sigma as the library lays it out, [N, 6]: 0 outside the free anchored nodes."""
    N = sysm["fixed"].shape[0]
    x = np.zeros((N, 6))
    x[sysm["nodes"]] = node_columns(sysm, node)[:, b].reshape(-1, 6)
    return x


def block(sysm, r, c):
    """(Sigma[r, c] 6 x 6, status): a fixed node gives 0 and OK; else an unanchored one NaN and UNANCHORED; H not positive definite
    BREAKDOWN and NaN."""
    if sysm["fixed"][r] or sysm["fixed"][c]:
        return np.zeros((6, 6)), OK
    if not sysm["anchored"][r] or not sysm["anchored"][c]:
        return np.full((6, 6), np.nan), UNANCHORED
    if not sysm["pd"]:
        return np.full((6, 6), np.nan), BREAKDOWN
    pr = int(sysm["place"][r])
    return node_columns(sysm, c)[6 * pr:6 * pr + 6, :].copy(), OK


def gate_blocks(Xi, Xj, Z, Om, Sii, Sij, Sjj):
    """(d2, status, S, e, J = [A B]) of one candidate edge from the three blocks: S = J [[Sii, Sij], [Sij^T, Sjj]] J^T + Omega^-1,
    d2 = e^T S^-1 e; NOT_PD and NaN where Omega or S is not positive definite."""
    e, A, B = gm.edge_jacobians(Xi, Xj, Z)
    J = np.hstack([A, B])
    Om = np.asarray(Om, np.float64).reshape(6, 6)
    try:
        np.linalg.cholesky(Om)
        Sg = np.block([[Sii, Sij], [Sij.T, Sjj]])
        S = J @ Sg @ J.T + np.linalg.inv(Om)
        S = 0.5 * (S + S.T)
        np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return float("nan"), NOT_PD, None, e, J
    return float(e @ np.linalg.solve(S, e)), OK, S, e, J


def gate(sysm, poses, cand):
    """(d2, status) of one candidate edge record at `poses` by the library's rules: the worst status of the two nodes first."""
    poses = gm.normalised(poses)
    i, j = int(cand["i"]), int(cand["j"])
    (Sii, si), (Sij, _), (Sjj, sj) = block(sysm, i, i), block(sysm, i, j), block(sysm, j, j)
    worst = max(si, sj)
    if worst in (BREAKDOWN, UNANCHORED):
        return float("nan"), worst
    d2, st, _, _, _ = gate_blocks(poses[i], poses[j], gm.normalised(cand["z"])[0], cand["info"], Sii, Sij, Sjj)
    return d2, max(worst, st)


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def drift_allowance(sysm, iterations, x_norm):
    """d = eps * iterations * (6 (max degree + 1) + 4) * | |H| |_2 * |x|_2: how far the residual the conjugate-gradient recurrence
    carries (r <- r - alpha A p, never recomputed) can drift from e_c - H x.  Each iteration adds to r a row product of 6 (max
    degree + 1) terms and to x and r one multiply-add each (the + 4), each rounded once, at the scale | |H| | |x|."""
    return EPS * iterations * (6.0 * (sysm["max_degree"] + 1) + 4.0) * sysm["norm_abs"] * x_norm


def block_bound(sysm, tolerance, d, Sigma_block):
    """|Sigma_gpu - Sigma_dense|_2 <= |H^-1|_2 (tolerance + d) sqrt(6) + 64 eps kappa_2(H) |Sigma_dense|_2: six columns with a true
    residual of at most tolerance + d each, through H^-1; and the dense inverse's own error."""
    return sysm["norm_inv"] * (tolerance + d) * math.sqrt(6.0) + 64.0 * EPS * sysm["cond"] * float(np.linalg.norm(Sigma_block, 2))


def gate_bound(S, e, J, bb):
    """What an error of at most bb (2-norm) in each of the three blocks does to d2 = e^T S^-1 e.  The 12 x 12 matrix of the blocks
    moves by at most 2 bb (the diagonal blocks' maximum plus the off-diagonal one), S by dS <= 2 bb |J|_2^2, and with |S^-1| dS <=
    1/2, d2 by at most 2 |S^-1 e|^2 dS (the first-order term e^T S^-1 dS S^-1 e and a geometric series that at most doubles it).
    The gate's own arithmetic — a 6 x 6 Cholesky in double — adds 1e-9 d2, the bound tests/test_graph_cov_model.py holds it to."""
    dS = 2.0 * bb * float(np.linalg.norm(J, 2)) ** 2
    y = np.linalg.solve(S, e)
    if float(np.linalg.norm(np.linalg.inv(S), 2)) * dS > 0.5:
        return float("inf")
    return 2.0 * float(y @ y) * dS + 1e-9 * float(e @ y)


# ---------------------------------------------------------------------------------------------
# designed graphs
# ---------------------------------------------------------------------------------------------
def two_components(n=6, m=4, seed=3):
    """drifted_ring(n) (node 0 fixed) and, apart from it, a chain of m free nodes n .. n + m - 1 without a fixed one."""
    _, init, fixed, edges = gm.drifted_ring(n, 1, seed)
    rng = np.random.default_rng(seed)
    extra = np.stack([gm.from_axis_angle((0, 0, 1), 0.1 * k, (20.0 + k, 5.0, 0.0)) for k in range(m)])
    noisy = np.stack([gm.retract(p, rng.normal(scale=[2e-3] * 3 + [2e-2] * 3)) for p in extra])
    more = gm.api.graph_edges([n + k for k in range(m - 1)], [n + k + 1 for k in range(m - 1)],
                              np.stack([gm.between(extra[k], extra[k + 1]) for k in range(m - 1)]), gm.OMEGA)
    return np.concatenate([init, noisy]), np.concatenate([fixed, np.zeros(m, np.int32)]), np.concatenate([edges, more])


def weighted_ring(n=12, seed=5):
    """drifted_ring(n, 2) with Geman-McClure (scale 3) on the loop edges (kind 1) and the odometry edge 4-5's twin — a second edge
    4-5 appended last — switched off -> (poses, fixed, edges, table, active)."""
    _, init, fixed, edges = gm.drifted_ring(n, 2, seed)
    twin = edges[4:5].copy()
    edges = np.concatenate([edges, twin])
    active = np.ones(len(edges), np.int32)
    active[-1] = 0
    return init, fixed, edges, {1: ("geman_mcclure", 3.0)}, active


def rescaled(poses, edges, step):
    """The graph with every translation — of poses and measurements alike — times step; the information matrices stay."""
    poses, edges = np.array(poses, np.float64), edges.copy()
    poses[:, 4:] *= step
    edges["z"][:, 4:] *= step
    return poses, edges


LONG_STEP = 0.01          # the long chains and rings are walked in steps of a centimetre: see designed()


def designed():
    """[dict(name, poses, fixed, edges, table, active, query, max_pcg_iterations, pcg_tolerance)]: the graphs of
    tests/test_gpu_pose_graph_cov.py.  query: at most 8 nodes — the first free one, the last, the middle, a fixed one, a
    duplicate.  (max_pcg_iterations, pcg_tolerance) are chosen so that drift_allowance at the cap stays below a tenth of the
    tolerance (tests/test_graph_cov_model.py asserts it): the preconditioner makes a chain exact and leaves the loop edges to the
    iterations, so a few dozen iterations are many, and the long chains — whose | |H| | |x| grows with the cube of their length —
    are solved to a looser tolerance than the short ones."""
    out = []

    def add(name, poses, fixed, edges, cap, tol, table=None, active=None, query=None):
        N = len(fixed)
        if query is None:
            query = sorted({1 % N, N - 1, N // 2, 0})[:8] + [N - 1]
        out.append(dict(name=name, poses=np.asarray(poses), fixed=np.asarray(fixed), edges=edges, table=table, active=active, query=list(query),
                        max_pcg_iterations=cap, pcg_tolerance=tol))
    for n in (2, 5, 64, 65):
        p, f, e = gm.chain(n, seed=n)
        p, e = rescaled(p, e, 1.0 if n < 64 else LONG_STEP)
        add("chain%d" % n, p, f, e, *CAPS["chain%d" % n])
    for n in (1024, 1025, 1030):
        _, p, f, e = gm.drifted_ring(n, 1, seed=n)
        p, e = rescaled(p, e, LONG_STEP)
        add("ring%d" % n, p, f, e, *CAPS["ring%d" % n])
    _, p, f, e = gm.drifted_ring(12, 2, seed=GATE_SEED)
    add("ring12_two_loops", p, f, e, *CAPS["ring12_two_loops"])
    p, f, e = gm.hub(40, 0, seed=2)
    f = f.copy()
    f[0] = 1
    add("hub40", p, f, e, *CAPS["hub40"])
    p, f, e = two_components()
    add("two_components", p, f, e, *CAPS["two_components"], query=[1, 5, 0, 7, 9, 5])
    p, f, e, table, active = weighted_ring()
    add("weighted_ring", p, f, e, *CAPS["weighted_ring"], table=table, active=active)
    return out


# (max_pcg_iterations, pcg_tolerance) per designed graph; see designed()
CAPS = {
    "chain2": (12, 1e-8), "chain5": (48, 1e-8), "chain64": (64, 1e-8), "chain65": (64, 1e-8),
    "ring1024": (64, 1e-6), "ring1025": (64, 1e-6), "ring1030": (64, 1e-6),
    "ring12_two_loops": (66, 1e-8), "hub40": (48, 1e-8), "two_components": (60, 1e-8), "weighted_ring": (66, 1e-8),
}
# The ring of the gate and LoopCloser tests: drifted_ring(12, 1, GATE_SEED, GATE_INFO).  Its bias is drifted_ring's own, the seed
# moves only the noise: over seeds 0 .. 11 and gm.OMEGA the true closing edge has d2 = 4.5 .. 9.1 and the one displaced by 5 m
# 64 .. 93, whatever the direction — the ring's predicted sigma is half a metre, so 5 m cannot reach 100.  Every information
# matrix doubled doubles both exactly (S halves); seed 5 then gives 8.9 and 137 (tests/test_graph_cov_model.py asserts both).
GATE_SEED = 5
GATE_INFO = 2.0 * gm.OMEGA


def lin_of(case):
    if case["table"] or case["active"] is not None:
        return grm.linearize(case["poses"], case["fixed"], case["edges"], case["table"], case["active"])
    return gm.linearize(case["poses"], case["fixed"], case["edges"])


def gate_ring(seed=None):
    """The 12-ring of the gate tests as a LoopCloser holds it -> (poses [12, 7] dead-reckoned, fixed, odometry edges (kind 0, each
    measuring what lies between consecutive poses), true = the closing edge (0, 11, Z) from the ground truth, false = the same with
    Z displaced by 5 m)."""
    gt, init, fixed, edges = gm.drifted_ring(12, 1, GATE_SEED if seed is None else seed)
    odo = gm.api.graph_edges(list(range(11)), list(range(1, 12)), np.stack([gm.between(init[k], init[k + 1]) for k in range(11)]), GATE_INFO)
    Z = gm.between(gt[0], gt[11])
    true = gm.api.graph_edges([0], [11], [Z], GATE_INFO, kind=1)
    Zf = Z.copy()
    Zf[4:] += np.array([3.0, 4.0, 0.0])
    false = gm.api.graph_edges([0], [11], [Zf], GATE_INFO, kind=1)
    return init, fixed, odo, true, false
