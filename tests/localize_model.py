"""Shared by the localisation tests: the site map, the localising traversal, the reader loop on the CPU oracle and the seeded first
scan built from oracle pieces.  Everything here is computed once and never modified.

Shapes: those of mapper_lag_common (16 x 900, 6 regions, 10 edges per region, P = 4, 14 scans).
The site map: the edges of synth stream 0, inserted at their ground-truth poses (orc.Map.update(edges, T_of(gt)); on the GPU
liodom_map_update, which test_gpu_map holds bit-equal).  The localising traversal is synth stream 1: the same world under other
noise, so no map leaf is a bit-copy of a window point (the degeneracy of the synchronous mapper, DESIGN.md §4, cannot occur).

The reader loop (liodom_attach_map_reader): orc.Odometer(mapping=2) whose received map is set to local(T_j, 2, 1) of the frozen
map after each step j.
The seeded first scan (liodom_seed_stream), from pieces: T = pose_ops(seed); queries = transform(T, edges); correspondences =
match_edges on the received map local(T, 2, 1) (the window is empty); blocks_of; lm_solve from the seed; and the same once more
from the first solve's result."""
import numpy as np

from designed_solves import blocks_of, trace_of
from mapper_lag_common import EPR, H, K, P, R, W, T_of

CELLS = (2, 1)
SEED_OFFSET_T = np.array([0.2, -0.1, 0.05])      # the perturbed seed: metres off the ground truth ...
SEED_HALF_ANGLE = 0.005                          # ... and this half-angle about z [rad]

_CACHE = {}


def params(orc, mapping=2):
    return orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, knn_mode=1, mapping=mapping)


def traversal(orc, synth, stream, count=K):
    """[(scan, edges, gt pose[7])] of a synth stream."""
    key = ("trav", stream, count)
    if key not in _CACHE:
        cfg = synth.make_cfg(H, W, 0)
        po = params(orc)
        out = []
        for k in range(count):
            x, gt = synth.scan(cfg, stream, k)
            out.append((x, orc.extract(po, x, H, W)["edges"], gt.copy()))
        _CACHE[key] = out
    return _CACHE[key]


def site_updates(orc, synth):
    """The updates that build the site map: [(edges, T_of(gt))] of stream 0."""
    return [(e, T_of(gt)) for _, e, gt in traversal(orc, synth, 0)]


def site_map(orc, synth):
    if "site" not in _CACHE:
        mo = orc.Map()
        for e, T in site_updates(orc, synth):
            mo.update(e, T)
        _CACHE["site"] = mo
    return _CACHE["site"]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def seeds(orc, synth):
    """The two seeds of the tests for scan 0 of the localising traversal: its ground truth, and the perturbed one."""
    gt = traversal(orc, synth, 1)[0][2]
    q = quat_mul(gt[:4], np.array([0.0, 0.0, np.sin(SEED_HALF_ANGLE), np.cos(SEED_HALF_ANGLE)]))
    return dict(truth=gt.copy(), perturbed=np.concatenate([q / np.linalg.norm(q), gt[4:] + SEED_OFFSET_T]))


def normalised(pose7):
    """The seed as liodom_seed_stream takes it: quaternion normalised in double."""
    p = np.array(pose7, dtype=np.float64)
    p[:4] = p[:4] / np.sqrt(np.sum(p[:4] * p[:4]))
    return p


def oracle_reader_run(orc, synth):
    """One record per scan of the oracle's reader loop: pose, LM terminations / iterations, matches, the correspondences of both
    passes, the window size they index into and the received map the scan searched.  Also checks that the map stays frozen."""
    if "reader" in _CACHE:
        return _CACHE["reader"]
    mo = site_map(orc, synth)
    before = mo.all()
    od = orc.Odometer(params(orc))
    out = []
    for _, e, _ in traversal(orc, synth, 1):
        n_window, recv = od.window().shape[0], od.received_map()
        pose, info = od.step(e)
        out.append(dict(pose=pose.copy(), term=[info.lm[i].termination for i in (0, 1)], iters=[info.lm[i].iterations for i in (0, 1)],
                        matches=[int(info.matches[i]) for i in (0, 1)], corr=[tuple(a.copy() for a in od.last_corr(it)) for it in (0, 1)],
                        n_window=n_window, recv=recv))
        od.set_received_map(mo.local(T_of(pose), *CELLS))
    od.close()
    assert np.array_equal(before.view(np.uint32), mo.all().view(np.uint32))
    _CACHE["reader"] = out
    return out


def solve_from(orc, po, edges, local_map, q, t):
    """One pass of a scan from explicit inputs: queries under (q, t), correspondences on local_map, the LM solve from (q, t)."""
    T, _ = orc.pose_ops(q, t)
    queries = orc.transform(T, edges)[:, :3]
    v, ia, ib = orc.match_edges(po, local_map, queries)
    blocks = blocks_of(edges, local_map, v, ia, ib)
    q1, t1, tr = orc.lm_solve(blocks, q, t)
    return dict(T=T, queries=queries, corr=(v, ia, ib), blocks=blocks, q=q1, t=t1, trace=trace_of(tr), matches=int(v.sum()))


def seeded_first_scan(orc, synth, seed7):
    """Scan 0 of the localising traversal from the seed, on the oracle's pieces: the two passes and the pose they end with."""
    mo, po = site_map(orc, synth), params(orc)
    edges = traversal(orc, synth, 1)[0][1]
    s = normalised(seed7)
    T_seed, _ = orc.pose_ops(s[:4], s[4:])
    recv = mo.local(T_seed, *CELLS)
    p0 = solve_from(orc, po, edges, recv, s[:4], s[4:])
    p1 = solve_from(orc, po, edges, recv, p0["q"], p0["t"])
    return dict(T_seed=T_seed, recv=recv, edges=edges, passes=[p0, p1], pose=np.concatenate([p1["q"], p1["t"]]))
