"""Shared by the lagged-mapper tests: the shapes of the existing mapping tests, and the lagged loop on the CPU oracle
(orc.Odometer + orc.Map), computed once and never modified.

The loop ("Lagged mapper"): after step j >= P the mapper integrates the frame that has just left the sliding
window, update(e_{j-P}, T_{j-P}), and the odometer receives local(T_j, 2, 1) for scan j + 1."""
import numpy as np

H, W, R, EPR, P, K = 16, 900, 6, 10, 4, 14      # P, K and the stream seed (0): test_gpu_map.test_external_map_feeds_the_knn_cloud
POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4             # the project's per-scan pose tolerance [m], [rad]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rot_angle(qa, qb):
    return 2.0 * np.arccos(min(1.0, abs(float(np.dot(qa, qb)))))


def T_of(pq):
    qx, qy, qz, qw = pq[:4]
    Rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                   [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                   [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return np.concatenate([Rm, np.array(pq[4:]).reshape(3, 1)], axis=1)


def scans_of(synth, stream=0, count=K):
    cfg = synth.make_cfg(H, W, 0)
    return [synth.scan(cfg, stream, k)[0] for k in range(count)]


_ORACLE = {}


def oracle_lagged_run(orc, synth):
    """One record per scan of the oracle's lagged loop: pose, LM terminations / iterations, map_points, the correspondences of
    both passes, the window size they index into and the received map the scan searched."""
    if "run" in _ORACLE:
        return _ORACLE["run"]
    po = orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, knn_mode=1, mapping=2)
    od, mo = orc.Odometer(po), orc.Map()
    hist, out = [], []
    for j, x in enumerate(scans_of(synth)):
        e = orc.extract(po, x, H, W)["edges"]
        n_window, recv = od.window().shape[0], od.received_map()
        pose, info = od.step(e)
        hist.append((e, T_of(pose)))
        out.append(dict(pose=pose.copy(), term=[info.lm[i].termination for i in (0, 1)], iters=[info.lm[i].iterations for i in (0, 1)],
                        map_points=info.map_points, corr=[tuple(a.copy() for a in od.last_corr(it)) for it in (0, 1)],
                        n_window=n_window, n_recv=recv.shape[0]))
        if j >= P:
            mo.update(*hist[j - P])
            od.set_received_map(mo.local(hist[j][1], 2, 1))
    _ORACLE["run"] = out
    od.close()
    return out


def map_part_correspondences(rec):
    """Accepted correspondences of a scan (both passes) whose nearest neighbour lies in the received-map part of window ++ map."""
    return sum(int((a[v == 1] >= rec["n_window"]).sum()) for v, a, _ in rec["corr"])
