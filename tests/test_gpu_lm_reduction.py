"""The solve's reduction of the normal equations (k_lm_solve: per-wave reduce-scatter in registers, per-wave sums through LDS, the
exchange between the G workgroups of a stream) on an MI355X: deterministic for G = 1 and G = 8, the sums equal J^T J at the
returned pose, and one path for every edge capacity (also past the size at which the solve once fell back to another reduction)."""
import os

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd.api import COV_VALID

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDL64 = (64, 1800, 0, 8, 10, 20)      # H, W, lidar_type, R, epr, P (bench.py's headline shape)
POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4


def _clear_env(monkeypatch):
    for name in ("LIODOM_SPECULATE", "LIODOM_CHAIN", "LIODOM_KNN_OVERLAP", "LIODOM_SAFE_MODE", "LIODOM_PIPE_FLAGS", "LIODOM_KNN8",
                 "LIODOM_HASH_INCR", "LIODOM_RING_SPLIT_LB", "LIODOM_EARLY_REBUILD"):
        monkeypatch.delenv(name, raising=False)


def _rot(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _rot_angle(qa, qb):
    R = _rot(qa).T @ _rot(qb)
    return float(np.arccos(np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)))


def _replay(synth, scans, shape, lm_workgroups, K, cov=0):
    H, W, lt, R, epr, P = shape
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(max_points=H * W, max_width=W, pose_log_capacity=K + 8, lm_workgroups=lm_workgroups, pose_covariance=cov))
    g.alloc_resident(K)
    for k in range(K):
        g.upload_scan(0, k, scans[k])
    g.sync()
    poses, infos = g.replay_resident(0, K, H * W, H, W, depth=1)
    plog, ilog = g.pose_log(0, 0, K)
    modes = g.modes()
    g.close()
    assert all(i.status == 0 for i in ilog)
    return poses.copy(), bytes(infos), plog.copy(), bytes(ilog), modes


@pytest.mark.parametrize("G", [8, 1])
def test_fresh_handles_give_identical_bits(synth, monkeypatch, G):
    _clear_env(monkeypatch)
    H, W, lt = HDL64[:3]
    K = 60
    cfg = synth.make_cfg(H, W, lt)
    scans = [synth.scan(cfg, 0, k)[0] for k in range(K)]
    a = _replay(synth, scans, HDL64, G, K)
    b = _replay(synth, scans, HDL64, G, K)
    assert a[4]["lm_groups"] == str(G) and b[4]["lm_groups"] == str(G), a[4]
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert a[1] == b[1] and a[3] == b[3]


def _h_ref(orc, pose, edges, local_map, valid, ia, ib):
    """sum rho' J^T J (Huber a = 0.2) over the correspondences at `pose`, float64, with the oracle's autodiff Jacobians."""
    Hs = np.zeros((6, 6))
    n = 0
    for e in np.nonzero(valid)[0]:
        r, J, _ = orc.point2line(pose[:4], pose[4:], edges[e, :3], local_map[ia[e], :3], local_map[ib[e], :3])
        s = float(r @ r)
        rho1 = 1.0 if s <= 0.04 else max(0.2 / np.sqrt(s), np.finfo(float).tiny)
        Hs += rho1 * (J.T @ J)
        n += 1
    return Hs, n


@pytest.mark.parametrize("G", [1, 8])
def test_information_matrix_is_jtj_at_the_returned_pose(orc, synth, monkeypatch, G):
    """pose_covariance = 1: the H of every record, entry by entry, against a float64 sum over the scan's correspondences.  The error
    of entry (i, j) is measured against its natural scale sqrt(H_ii H_jj) (an off-diagonal sum may cancel to near zero)."""
    _clear_env(monkeypatch)
    H, W, lt, R, epr, P = HDL64
    K = P + 6
    N = H * W
    cfg = synth.make_cfg(H, W, lt)
    scans = [synth.scan(cfg, 7, k)[0] for k in range(K)]
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8, lm_workgroups=G, pose_covariance=1))
    assert g.modes()["lm_groups"] == str(G)
    g.alloc_resident(K + 1)
    for k in range(K):
        g.upload_scan(0, k, scans[k])
    g.sync()
    steps = []
    for k in range(K):
        lmap, _ = g.local_map()
        poses, infos = g.replay_resident(k, 1, N, H, W, ahead=True, depth=1)
        steps.append((poses[0][0].copy(), infos[0], lmap, g.get_edges()["edges"], g.correspondences(1)))
    log = g.pose_covariance_log(0, 0, K)
    g.close()
    worst = 0.0
    for k in range(1, K):
        pose, info, lmap, edges, (valid, ia, ib) = steps[k]
        rec = log[k]
        assert rec["flags"] == COV_VALID, (k, rec["flags"])
        Hr, n = _h_ref(orc, pose, edges, lmap, valid, ia, ib)
        assert rec["n_residuals"] == n == info.matches[1], k
        Hd = rec["information"]
        scale = np.sqrt(np.outer(np.diag(Hr), np.diag(Hr)))
        err = float(np.max(np.abs(Hd - Hr) / scale))
        worst = max(worst, err)
        assert err <= 1e-12, (k, err)
    print("G = %d: largest scaled error of an entry of H: %.3g" % (G, worst))


def test_edge_capacity_beyond_the_old_lds_matrix(orc, synth, monkeypatch):
    """edge_cap = 64 * 8 * 48 = 24 576 edges: more than the old transposed LDS matrix left room for (24 064 with a 256-thread
    solve), which then reduced through a second path.  Creates, and follows the oracle over a short stream."""
    _clear_env(monkeypatch)
    H, W, lt, R, epr, P = 64, 1800, 0, 8, 47, 6
    K = P + 4
    cfg = synth.make_cfg(H, W, lt)
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1)
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(max_points=H * W, max_width=W))
    od = orc.Odometer(po)
    for k in range(K):
        x, _ = synth.scan(cfg, 0, k)
        pose_o, info_o = od.step(orc.extract(po, x, H, W)["edges"])
        pose_g, info_g = g.process_scan(x, H, W)
        assert info_g.status == 0, k
        assert np.linalg.norm(pose_g[4:] - pose_o[4:]) <= POSE_TOL_T and _rot_angle(pose_g[:4], pose_o[:4]) <= POSE_TOL_R, k
        if k > 0:
            assert list(info_g.matches) == list(info_o.matches), k
            assert [info_g.lm[0].iterations, info_g.lm[1].iterations] == [info_o.lm[0].iterations, info_o.lm[1].iterations], k
            assert [info_g.lm[0].termination, info_g.lm[1].termination] == [info_o.lm[0].termination, info_o.lm[1].termination], k
    g.close()
