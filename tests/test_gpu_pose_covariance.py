"""Per-scan pose covariance (config.pose_covariance = 1: the finalising solve's H, k_pose_cov, liodom_get_pose_covariance_log /
liodom_wait_pose_covariance) on an MI355X.  The information matrix is checked against sum rho' J^T J built from the oracle's
autodiff Jacobians (oracle.point2line) on the correspondences, edges and pose of the same scan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd.api import COV_VALID, COV_SINGULAR, COV_NO_SOLVE, COV_EVAL_FAILURE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2
SHAPES = {
    # name: H, W, lidar_type, R, epr, P  (as the chain-mode tests of test_gpu_parity.py)
    "hdl64": (64, 1800, 0, 8, 10, 20),
    "vlp16": (16, 1800, 0, 8, 20, 10),
    "ouster128": (128, 2048, 1, 8, 10, 30),
}


def _clear_env(monkeypatch):
    for name in ("LIODOM_SPECULATE", "LIODOM_CHAIN", "LIODOM_KNN_OVERLAP", "LIODOM_SAFE_MODE", "LIODOM_PIPE_FLAGS", "LIODOM_KNN8",
                 "LIODOM_HASH_INCR", "LIODOM_RING_SPLIT_LB", "LIODOM_EARLY_REBUILD"):
        monkeypatch.delenv(name, raising=False)


def mk(orc, H, W, lt=0, R=8, epr=10, P=5, S=1, cov=1, **kw):
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1)
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(n_streams=S, max_points=H * W, max_width=W, pose_covariance=cov, **kw))
    return po, g


def _rot(q):
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _bits(x):
    return np.atleast_1d(np.asarray(x)).view(np.uint8)


def h_ref(orc, pose, edges, local_map, valid, ia, ib):
    """sum rho' J^T J (Huber a = 0.2) over the valid correspondences at `pose`, with the oracle's autodiff Jacobians."""
    H = np.zeros((6, 6))
    n = 0
    for e in np.nonzero(valid)[0]:
        r, J, _ = orc.point2line(pose[:4], pose[4:], edges[e, :3], local_map[ia[e], :3], local_map[ib[e], :3])
        s = float(r @ r)
        rho1 = 1.0 if s <= 0.04 else max(0.2 / np.sqrt(s), np.finfo(float).tiny)
        H += rho1 * (J.T @ J)
        n += 1
    return H, n


def check_record(orc, rec, info, pose, edges, local_map, corr, what):
    valid, ia, ib = corr
    Hr, n = h_ref(orc, pose, edges, local_map, valid, ia, ib)
    assert rec["flags"] == COV_VALID, (what, rec["flags"])
    assert rec["scan_index"] == info.scan_index, what
    assert rec["n_residuals"] == n == info.matches[1], (what, rec["n_residuals"], n, info.matches[1])
    assert rec["termination"] == info.lm[1].termination, what
    assert np.float64(rec["final_cost"]).view(np.uint64) == np.float64(info.lm[1].final_cost).view(np.uint64), what
    H = rec["information"]
    assert np.array_equal(H, H.T), what
    assert np.linalg.norm(H - Hr) <= 1e-8 * np.linalg.norm(Hr), (what, np.linalg.norm(H - Hr) / np.linalg.norm(Hr))
    s2 = 2.0 * rec["final_cost"] / (3 * n - 6)
    assert rec["sigma2"] == pytest.approx(s2, rel=1e-15), what
    cref = s2 * np.linalg.inv(Hr)
    assert np.linalg.norm(rec["covariance"] - cref) <= 1e-6 * np.linalg.norm(cref), what
    w = np.linalg.eigvalsh(Hr)
    assert np.max(np.abs(rec["eigenvalues"] - w)) <= 1e-9 * w[-1], what
    V = rec["eigenvectors"]
    assert np.allclose(H @ V, V * rec["eigenvalues"], rtol=0, atol=1e-9 * w[-1]), what


def _chain_against_the_oracle(orc, synth, shape, apply_on_ftol=0, extra=10):
    H, W, lt, R, epr, P = SHAPES[shape]
    N, K = H * W, P + extra
    cfg = synth.make_cfg(H, W, lt)
    scans = [synth.scan(cfg, 7, k)[0] for k in range(K)]
    po, g = mk(orc, H, W, lt, R, epr, P, pose_log_capacity=K + 8, lm_apply_step_on_ftol=apply_on_ftol)
    g.alloc_resident(K + 1)
    for k in range(K):
        g.upload_scan(0, k, scans[k])
    g.sync()
    od = orc.Odometer(po)
    steps = []
    for k in range(K):
        lmap, _ = g.local_map()                     # the cloud this scan's kNN passes search
        # one scan per call, the next scan's extraction issued ahead: every scan runs the chain of replay_resident(depth = 1)
        poses, infos = g.replay_resident(k, 1, N, H, W, ahead=True, depth=1)
        pose_o, info_o = od.step(orc.extract(po, scans[k], H, W)["edges"])
        steps.append((poses[0][0].copy(), infos[0], lmap, g.get_edges()["edges"], g.correspondences(1), info_o))
    modes = g.modes()
    assert modes["chain"] == "1" and modes["pose_cov"] == "1", modes
    log = g.pose_covariance_log(0, 0, K)
    plog, ilog = g.pose_log(0, 0, K)
    g.close()
    for k, (pose, info, lmap, edges, corr, info_o) in enumerate(steps):
        assert np.array_equal(plog[k], pose) and ilog[k].scan_index == k
        if k == 0:
            assert log[0]["flags"] == COV_NO_SOLVE and np.all(np.isnan(log[0]["covariance"]))
            continue
        # (the oracle's own run may pick a different line at a handful of edges: the trajectories differ in the last bits)
        assert abs(int(log[k]["n_residuals"]) - int(info_o.matches[1])) <= 6, k
        check_record(orc, log[k], info, pose, edges, lmap, corr, (shape, k))


@pytest.mark.parametrize("shape", ["hdl64", "vlp16", "ouster128"])
def test_chain_mode_records_against_the_oracle(orc, synth, monkeypatch, shape):
    _clear_env(monkeypatch)
    _chain_against_the_oracle(orc, synth, shape)


def test_records_with_apply_step_on_ftol(orc, synth, monkeypatch):
    _clear_env(monkeypatch)
    _chain_against_the_oracle(orc, synth, "vlp16", apply_on_ftol=1)


def test_switch_off_changes_nothing(synth, monkeypatch):
    _clear_env(monkeypatch)
    H, W, R, epr, P, K = 64, 1800, 8, 10, 20, 30
    N = H * W
    cfg = synth.make_cfg(H, W, 0)
    scans = [synth.scan(cfg, 0, k)[0] for k in range(K)]
    out = {}
    for cov in (0, 1):
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                      la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8, pose_covariance=cov))
        g.alloc_resident(K)
        for k in range(K):
            g.upload_scan(0, k, scans[k])
        g.sync()
        poses, infos = g.replay_resident(0, K, N, H, W, depth=1)
        modes = g.modes()
        plog, ilog = g.pose_log(0, 0, K)
        out[cov] = (poses.copy(), bytes(infos), plog.copy(), bytes(ilog), g.window()[0].copy(), modes)
        if cov == 0:
            assert "pose_cov" not in modes
            rec = la.PoseCov()
            assert g.L.liodom_get_pose_covariance_log(g.h, 0, 0, 1, C.byref(rec)) == ERR_UNSUPPORTED
            assert g.L.liodom_wait_pose_covariance(g.h, 0, K - 1, C.byref(rec)) == ERR_UNSUPPORTED
        else:
            assert modes["pose_cov"] == "1"
            log = g.pose_covariance_log(0, 0, K)
            assert [r["scan_index"] for r in log] == list(range(K))
            assert all(r["flags"] == COV_VALID for r in log[1:])
        g.close()
    a, b = out[0], out[1]
    assert a[5]["chain"] == "1" and b[5]["chain"] == "1"
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
    assert a[1] == b[1] and a[3] == b[3]
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))
    assert {k: v for k, v in a[5].items() if not k.startswith("replay_")} == \
        {k: v for k, v in b[5].items() if not k.startswith("replay_") and k != "pose_cov"}


def test_lockstep_batch_records(orc, synth, monkeypatch):
    _clear_env(monkeypatch)
    H, W, R, epr, P, S, K = 64, 1800, 8, 10, 20, 16, 8
    N = H * W
    cfg = synth.make_cfg(H, W, 0)
    data = {d: [synth.scan(cfg, 30 + d, k)[0] for k in range(K)] for d in (0, 3, 5)}
    data[3] = [synth.ragged(x, H, W, 0, seed=200 + k) for k, x in enumerate(data[3])]
    src = [0] * S
    src[3], src[5], src[9] = 3, 5, 5
    po, g = mk(orc, H, W, 0, R, epr, P, S=S, pose_log_capacity=K + 8)
    modes = g.modes()
    assert modes["knn8"] == "1" and modes["hash_incr"] == "1" and modes["ring_split_lb"] == "1" and modes["pose_cov"] == "1", modes
    g.alloc_resident(K)
    for s in range(S):
        for k in range(K):
            g.upload_scan(s, k, data[src[s]][k] if s in (3, 5, 9) else synth.scan(cfg, 40 + s, k)[0])
    steps = []
    for k in range(K):
        maps = {d: g.local_map(d)[0] for d in (0, 3)}
        poses, infos = g.process_resident(k, N, H, W, readback=True, next_slot=(k + 1 if k + 1 < K else -1))
        assert all(i.status == 0 for i in infos), k
        steps.append({d: (poses[d].copy(), infos[d], maps[d], g.get_edges(d)["edges"], g.correspondences(1, stream=d)) for d in (0, 3)})
    logs = {s: g.pose_covariance_log(s, 0, K) for s in (0, 3, 5, 9)}
    g.close()
    for k in range(1, K):
        for d in (0, 3):
            pose, info, lmap, edges, corr = steps[k][d]
            check_record(orc, logs[d][k], info, pose, edges, lmap, corr, (k, d))
    for k in range(K):
        a, b = logs[5][k], logs[9][k]
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (k, key)


def test_per_scan_paths_wait_for_the_record(orc, synth, monkeypatch):
    _clear_env(monkeypatch)
    H, W, R, epr, P, K = 16, 900, 6, 10, 5, 10
    cfg = synth.make_cfg(H, W, 0)
    scans = [synth.scan(cfg, 3, k)[0] for k in range(K)]
    po, g = mk(orc, H, W, 0, R, epr, P, pose_log_capacity=K + 8)
    # ticket API at depth 1: scan k + 1 is submitted before pose k is collected
    got = []
    t = g.extract_edges_device(scans[0], H, W)
    assert g.odometry_submit_device(t)
    for k in range(K):
        if k + 1 < K:
            t = g.extract_edges_device(scans[k + 1], H, W)
            assert g.odometry_submit_device(t)
        pose, info = g.odometry_collect()
        assert info.scan_index == k
        got.append(g.wait_pose_covariance(0, k))
        if k >= 2:
            rec = la.PoseCov()
            assert g.L.liodom_wait_pose_covariance(g.h, 0, k - 2, C.byref(rec)) == ERR_INVALID_ARG
    log = g.pose_covariance_log(0, 0, K)
    for k in range(K):
        for key in got[k]:
            assert np.array_equal(_bits(got[k][key]), _bits(log[k][key])), (k, key)
    assert got[0]["flags"] == COV_NO_SOLVE and all(r["flags"] == COV_VALID for r in got[1:])
    # liodom_process_scan, after a reset: the first scan is NO_SOLVE again
    g.reset()
    got = []
    for k in range(4):
        _, info = g.process_scan(scans[k], H, W)
        got.append(g.wait_pose_covariance(0, info.scan_index))
    log = g.pose_covariance_log(0, 0, 4)
    for k in range(4):
        assert got[k]["scan_index"] == k
        for key in got[k]:
            assert np.array_equal(_bits(got[k][key]), _bits(log[k][key])), (k, key)
    assert got[0]["flags"] == COV_NO_SOLVE and got[1]["flags"] == COV_VALID
    g.close()


def _vertical_lines(k):
    """Edges on twelve vertical lines at exact float x, y around a static sensor; the heights move from scan to scan (no point
    repeats), so nothing constrains a vertical translation."""
    ang = np.arange(12) * (2 * np.pi / 12) + 0.1
    rad = 6.0 + 1.5 * (np.arange(12) % 4)
    xs, ys = np.float32(rad * np.cos(ang)), np.float32(rad * np.sin(ang))
    z = np.float32(-1.0 + 0.1 * np.arange(30) + 0.0137 * k)
    pts = [(x, y, zz, 0.0) for x, y in zip(xs, ys) for zz in z]
    return np.array(pts, dtype=np.float32)


def test_degenerate_geometry_is_visible(orc, synth, monkeypatch):
    _clear_env(monkeypatch)
    H, W, R, epr, P = 16, 900, 6, 10, 5
    po, g = mk(orc, H, W, 0, R, epr, P)
    recs = []
    for k in range(8):
        _, info = g.odometry_step(_vertical_lines(k))
        recs.append(g.wait_pose_covariance(0, info.scan_index))
    assert recs[0]["flags"] == COV_NO_SOLVE
    for k in range(2, 8):
        r = recs[k]
        assert r["flags"] & COV_VALID, (k, r["flags"])
        w, V = r["eigenvalues"], r["eigenvectors"]
        assert w[0] <= 1e-8 * w[-1], (k, w)
        assert abs(V[5, 0]) >= 0.999, (k, V[:, 0])
        d = np.diag(r["covariance"])
        assert (r["flags"] & COV_SINGULAR) or d[5] >= 1e6 * np.median(d), (k, d)
    # the synthetic box world on the same handle is well conditioned
    g.reset()
    cfg = synth.make_cfg(H, W, 0)
    for k in range(6):
        _, info = g.process_scan(synth.scan(cfg, 0, k)[0], H, W)
        r = g.wait_pose_covariance(0, info.scan_index)
        if k == 0:
            assert r["flags"] == COV_NO_SOLVE
        else:
            assert r["flags"] == COV_VALID and r["eigenvalues"][0] >= 1e-6 * r["eigenvalues"][-1], (k, r["eigenvalues"])
    g.close()


def test_mapping_mode_degeneracy_is_flagged(orc, synth):
    """The attached-mapper replay of test_gpu_map.py::test_attached_mapper_replays_the_mapping_node: every solve after the first
    scan ends with termination 5 (mapping mode degenerates) — the records say so."""
    H, W, R, epr, P, K = 16, 900, 6, 10, 5, 6
    cfg = synth.make_cfg(H, W, 0)
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, mapping=1),
                  la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 17, pose_covariance=1))
    mg = la.Map(max_cells=256, cell_capacity=32768)
    g.attach_mapper(mg, 2, 1)
    for k in range(K):
        _, info = g.process_scan(synth.scan(cfg, 0, k)[0], H, W)
        r = g.wait_pose_covariance(0, info.scan_index)
        if k == 0:
            assert r["flags"] == COV_NO_SOLVE
        else:
            assert info.lm[1].termination == 5 and r["flags"] == COV_EVAL_FAILURE, (k, r["flags"])
            assert np.all(np.isnan(r["covariance"])) and np.all(np.isnan(r["information"]))
    g.attach_mapper(None)
    g.close()
    mg.close()


def _to_ros(cov, pose, l2b34):
    """pose_cov_to_ros restated: A = [[-2 [R t_L]x, I], [2 I, 0]] on (half-angle tangent, translation)."""
    u = _rot(pose[:4]) @ l2b34[:, 3]
    X = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    A = np.zeros((6, 6))
    A[:3, :3], A[:3, 3:], A[3:, :3] = -2 * X, np.eye(3), 2 * np.eye(3)
    return A @ cov @ A.T


def test_replay_tool_writes_covariances(synth, tmp_path):
    exe = os.path.join(ROOT, "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (__graft_entry__.build())"
    H, W, R, epr, P, K = 16, 900, 6, 10, 5, 8
    cfg = synth.make_cfg(H, W, 0)
    scan_dir, out_dir = tmp_path / "scans", tmp_path / "out"
    scan_dir.mkdir(); out_dir.mkdir()
    scans = [synth.scan(cfg, 0, k)[0].astype(np.float32) for k in range(K)]
    for k, x in enumerate(scans):
        x.tofile(str(scan_dir / ("%06d.bin" % k)))
    r = subprocess.run([exe, str(scan_dir), str(out_dir) + "/", "scan_lines=16", "scan_regions=6", "edges_per_region=10",
                        "prev_frames=5", "covariance=1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = np.loadtxt(str(out_dir / "covariances.txt")).reshape(-1, 38)
    assert rows.shape[0] == K and rows[:, 0].astype(int).tolist() == list(range(K))
    # the same scans through a handle configured as the tool's Engine (liodom_process_scan per scan)
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(max_points=H * W, max_width=H * W // H + 1, pose_covariance=1, pose_log_capacity=K + 8))
    poses = [g.process_scan(x, H, W)[0] for x in scans]
    log = g.pose_covariance_log(0, 0, K)
    g.close()
    l2b = np.eye(3, 4)
    for k in range(K):
        assert int(rows[k, 1]) == log[k]["flags"], k
        if k == 0:
            assert np.all(np.isnan(rows[0, 2:]))
            continue
        ref = _to_ros(log[k]["covariance"], poses[k], l2b)
        assert np.allclose(rows[k, 2:].reshape(6, 6), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max()), k
