"""liodom_map_register_poses restated on the CPU oracle's pieces (contract: include/liodom_hip.h "registering a scan to the map"):
localize_model.seeded_first_scan's pass, carried on until the pose stops moving or the passes run out.

One row:  s = the start pose with its quaternion normalised in double; local = Map.local(T(s), cells) fetched once; then per pass,
from (q, t): queries = transform(T(q, t), edges) as floats; correspondences = orc.match_edges with knn_mode = 0 (brute force: the
exact five nearest, ties to the lower index, fifth closer than 1 m, line gate); blocks_of; orc.lm_solve from (q, t).
Ending: empty local map NO_MAP; fewer than min_matches FEW_MATCHES; solve termination 5 EVAL_FAILURE (all three: the pose before
that pass); |dt| <= stop_translation and |vec(q_new (x) conj(q_old))| <= stop_rotation CONVERGED; else MAX_PASSES after the last.
The final evaluation (information, sigma2) is that of the pose-covariance tests: sum rho' J^T J from the oracle's autodiff
Jacobians at the returned pose over the last pass's correspondences, 2 cost / (3 C - 6).

Nothing here is modified after it is computed; results are cached by their arguments."""
import numpy as np

from designed_solves import blocks_of, rho1

CONVERGED, MAX_PASSES, FEW_MATCHES, NO_MAP, EVAL_FAILURE = 0, 1, 2, 3, 4
DEFAULTS = dict(cells_xy=2, cells_z=1, max_passes=10, min_matches=6, stop_translation=1e-4, stop_rotation=1e-5, min_range=3.0,
                max_range=75.0)
# the starts of the issue's table: metres off the truth, then half-angles about x, y, z
START_A = (np.array([0.2, -0.1, 0.05]), np.array([0.0, 0.0, 0.005]))
START_B = (np.array([0.15, -0.1, 0.12]), np.array([0.004, -0.003, 0.005]))

_CACHE = {}


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def displaced(pose7, start):
    """pose7 moved by a start of the table: the translation added, the rotation [sin|h| h/|h|, cos|h|] applied on the right."""
    dt, h = start
    a = float(np.linalg.norm(h))
    dq = np.array([0.0, 0.0, 0.0, 1.0]) if a == 0.0 else np.concatenate([np.sin(a) * h / a, [np.cos(a)]])
    q = quat_mul(np.asarray(pose7[:4], np.float64), dq)
    return np.concatenate([q / np.linalg.norm(q), np.asarray(pose7[4:], np.float64) + dt])


def normalised(pose7):
    p = np.array(pose7, dtype=np.float64)
    p[:4] = p[:4] / np.sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
    return p


def pass_move(q_old, t_old, q_new, t_new):
    """(|t_new - t_old|, |vec(q_new (x) conj(q_old))|): register_pass_converged's two norms."""
    conj = np.array([-q_old[0], -q_old[1], -q_old[2], q_old[3]])
    v = quat_mul(np.asarray(q_new, np.float64), conj)[:3]
    d = np.asarray(t_new, np.float64) - np.asarray(t_old, np.float64)
    return float(np.sqrt(np.sum(d * d))), float(np.sqrt(np.sum(v * v)))


def information(orc, pose, edges, local, valid, ia, ib, min_range, max_range):
    H = np.zeros((6, 6))
    for e in np.nonzero(valid)[0]:
        r, J, _ = orc.point2line(pose[:4], pose[4:], edges[e, :3], local[ia[e], :3], local[ib[e], :3], min_range, max_range)
        H += rho1(float(r @ r)) * (J.T @ J)
    return H


def brute_params(orc):
    return orc.make_params(knn_mode=0)


def register(orc, map_o, edges, pose7, local=None, **options):
    """One row on the oracle.  map_o: an orc.Map (or None with `local` given).  Returns dict(pose, termination, passes, matches,
    n_residuals, local_points, last_move_t, last_move_r, corr [E, 2], information, final_cost, sigma2, last_lm, moves: per taken
    pass (move_t, move_r), poses: the pose after every taken pass)."""
    o = dict(DEFAULTS, **options)
    edges = np.ascontiguousarray(edges, np.float32).reshape(-1, 4)
    po = brute_params(orc)
    s = normalised(pose7)
    if local is None:
        T0, _ = orc.pose_ops(s[:4], s[4:])
        local = map_o.local(T0, o["cells_xy"], o["cells_z"])
    local = np.ascontiguousarray(local, np.float32).reshape(-1, 4)
    E = edges.shape[0]
    out = dict(pose=s.copy(), termination=None, passes=0, matches=0, n_residuals=0, local_points=int(local.shape[0]), last_move_t=0.0,
               last_move_r=0.0, corr=np.full((E, 2), -1, np.int32), information=np.full((6, 6), np.nan), final_cost=0.0,
               sigma2=float("nan"), last_lm=(0, 0, 0), moves=[], poses=[], local=local)
    if local.shape[0] == 0:
        out["termination"] = NO_MAP
        return out
    q, t = s[:4].copy(), s[4:].copy()
    for p in range(o["max_passes"]):
        T, _ = orc.pose_ops(q, t)
        queries = orc.transform(T, edges)[:, :3] if E else np.zeros((0, 3), np.float32)
        if E:
            v, ia, ib = orc.match_edges(po, local, queries)
        else:
            v = ia = ib = np.zeros(0, np.int32)
        out["corr"] = np.stack([np.where(v != 0, ia, -1), np.where(v != 0, ib, -1)], axis=1).astype(np.int32).reshape(E, 2)
        out["matches"] = int(np.sum(v != 0))
        if out["matches"] < o["min_matches"]:
            out["termination"], out["last_lm"], out["final_cost"] = FEW_MATCHES, (0, 0, 0), 0.0
            return out
        blocks = blocks_of(edges, local, v, ia, ib)
        q1, t1, tr = orc.lm_solve(blocks, q, t, o["min_range"], o["max_range"])
        out["last_lm"] = (int(tr.termination), int(tr.iterations), int(tr.accepted))
        if tr.termination == 5:
            out["termination"], out["final_cost"] = EVAL_FAILURE, 0.0
            return out
        mt, mr = pass_move(q, t, q1, t1)
        q, t = q1.copy(), t1.copy()
        out["pose"] = np.concatenate([q, t])
        out["passes"] = p + 1
        out["last_move_t"], out["last_move_r"] = mt, mr
        out["moves"].append((mt, mr))
        out["poses"].append(out["pose"].copy())
        out["final_cost"] = float(tr.final_cost)
        out["valid"] = (v, ia, ib)
        if mt <= o["stop_translation"] and mr <= o["stop_rotation"]:
            out["termination"] = CONVERGED
            break
    if out["termination"] is None:
        out["termination"] = MAX_PASSES
    v, ia, ib = out["valid"]
    n = out["matches"]
    out["n_residuals"] = n
    out["information"] = information(orc, out["pose"], edges, local, v, ia, ib, o["min_range"], o["max_range"])
    out["sigma2"] = 2.0 * out["final_cost"] / (3 * n - 6) if 3 * n > 6 else float("nan")
    return out


def site_case(orc, synth, scan, start, **options):
    """A row of the issue's table on localize_model's site map: scan `scan` of the localising traversal from its ground truth
    displaced by `start` (None: the truth itself).  Cached."""
    import localize_model as lm
    key = ("site", scan, None if start is None else (tuple(start[0]), tuple(start[1])), tuple(sorted(options.items())))
    if key not in _CACHE:
        _, edges, gt = lm.traversal(orc, synth, 1)[scan]
        pose = gt.copy() if start is None else displaced(gt, start)
        r = register(orc, lm.site_map(orc, synth), edges, pose, **options)
        r["start"], r["edges"], r["truth"] = pose, edges, gt.copy()
        _CACHE[key] = r
    return _CACHE[key]
