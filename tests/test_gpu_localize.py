"""Localising in a saved map: map readers (liodom_attach_map_reader), seeded streams (liodom_seed_stream) and batched local maps
(liodom_map_get_local_batch / k_map_local_rows), against the CPU oracle's loop and pieces (tests/localize_model.py)."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import localize_model as lm
from designed_solves import blocks_of, trace_of
from mapper_lag_common import EPR, H, P, POSE_TOL_R, POSE_TOL_T, R, W, T_of, rot_angle, same

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)
_SITE = {}


def _handle(n_streams=1, recv_capacity=1 << 16, mapping=1, **cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=mapping),
                     la.make_config(n_streams=n_streams, max_points=H * W, max_width=W, recv_capacity=recv_capacity, **cfg))


def _site_map(orc, synth, **caps):
    """The site map on the device: built once by liodom_map_update (bit-equal to the oracle's), then imported."""
    if "blob" not in _SITE:
        m = la.Map(**CAPS)
        for e, T in lm.site_updates(orc, synth):
            m.update(e, T)
        assert same(m.all(), lm.site_map(orc, synth).all()) and m.num_cells() == 29 and m.status() == 0
        _SITE["blob"] = m.export_state()
        m.close()
    m = la.Map(**(caps or CAPS))
    m.import_state(_SITE["blob"])
    return m


def _corr_equal(got, want):
    (vg, ag, bg), (vo, ao, bo) = got, want
    ok = vg == 1
    return vg.shape == vo.shape and np.array_equal(vg, vo) and np.array_equal(ag[ok], ao[ok]) and np.array_equal(bg[ok], bo[ok])


def _pose_close(a, b, tol_t, tol_r):
    return np.linalg.norm(a[4:] - b[4:]) <= tol_t and rot_angle(a[:4], b[:4]) <= tol_r


def _one_stream_reader_run(orc, synth, count):
    """Poses and received maps (after each scan) of a one-stream handle reading the site map, unseeded."""
    key = ("one", count)
    if key not in _SITE:
        g, m = _handle(), _site_map(orc, synth)
        g.attach_map_reader(m, *lm.CELLS)
        out = []
        for x, _, _ in lm.traversal(orc, synth, 1)[:count]:
            pose, _ = g.process_scan(x, H, W)
            out.append((pose.copy(), g.received_map()))
        g.attach_mapper(None)
        g.close(); m.close()
        _SITE[key] = out
    return _SITE[key]


def test_reader_loop_against_the_oracle_loop(orc, synth):
    run = lm.oracle_reader_run(orc, synth)
    g, m = _handle(), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    assert g.modes()["map_readers"] == "1" and "mapper_lag" not in g.modes()
    before, cells = m.export_state(), m.num_cells()
    for j, (x, _, _) in enumerate(lm.traversal(orc, synth, 1)):
        rec = run[j]
        n_window, recv = g.window()[0].shape[0], g.received_map()
        assert same(recv, rec["recv"]), j
        pose, info = g.process_scan(x, H, W)
        print("scan %d: dt %.3e dr %.3e" % (j, np.linalg.norm(pose[4:] - rec["pose"][4:]), rot_angle(pose[:4], rec["pose"][:4])))
        assert _pose_close(pose, rec["pose"], POSE_TOL_T, POSE_TOL_R), j
        if j == 0:
            continue
        assert n_window == rec["n_window"], j
        assert [info.lm[i].termination for i in (0, 1)] == rec["term"], j
        assert [info.lm[i].iterations for i in (0, 1)] == rec["iters"], j
        for it in (0, 1):
            got = g.correspondences(it)
            assert _corr_equal(got, rec["corr"][it]), (j, it)
            assert int((got[1][got[0] == 1] >= n_window).sum()) > 0, (j, it)      # the map part is in use
    assert m.export_state() == before and m.num_cells() == cells and m.status() == 0
    g.attach_mapper(None)
    assert "map_readers" not in g.modes()
    g.close(); m.close()


@pytest.mark.parametrize("which", ["truth", "perturbed"])
def test_seeded_first_scan_on_the_gpus_own_inputs(orc, synth, which):
    seed = lm.normalised(lm.seeds(orc, synth)[which])
    po = lm.params(orc)
    g, m = _handle(debug_buffers=1, pose_covariance=1, pose_log_capacity=8), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    g.seed_stream(lm.seeds(orc, synth)[which])
    T_seed, _ = orc.pose_ops(seed[:4], seed[4:])
    st = api.parse_stream_state(g.export_stream_state(0))
    for name in ("odom", "prev_odom", "final_odom"):
        assert np.abs(st[name] - T_seed).max() <= 1e-15, name
    assert np.abs(st["param_q"] - seed[:4]).max() <= 1e-15 and np.array_equal(st["param_t"], seed[4:])
    assert (st["initialized"], st["append_raw"], st["frame_count"], st["n_frames"], st["scan_counter"]) == (1, 0, 0, 0, 0)
    recv = g.received_map()
    assert recv.shape[0] == 1609 and same(recv, m.get_local(T_seed, *lm.CELLS)) and same(recv, st["received_map"])
    x = lm.traversal(orc, synth, 1)[0][0]
    pose, info = g.process_scan(x, H, W)
    assert info.scan_index == 0 and info.status == 0
    e = g.get_edges()["edges"]
    # pass 0: the queries are the edges under the seed, the correspondences the oracle's on those queries and that map
    q0 = g.knn_queries(0)
    assert same(np.ascontiguousarray(q0), np.ascontiguousarray(orc.transform(T_seed, e)[:, :3]))
    c0 = g.correspondences(0)
    assert _corr_equal(c0, orc.match_edges(po, recv, q0))
    qa, ta, tr0 = orc.lm_solve(blocks_of(e, recv, *c0), seed[:4], seed[4:])
    assert trace_of(tr0) == trace_of(info.lm[0]) and tr0.termination == 2, (trace_of(tr0), trace_of(info.lm[0]))
    # pass 1, on the GPU's own queries; the solve chained from the oracle's first
    q1 = g.knn_queries(1)
    c1 = g.correspondences(1)
    assert _corr_equal(c1, orc.match_edges(po, recv, q1))
    qb, tb, tr1 = orc.lm_solve(blocks_of(e, recv, *c1), qa, ta)
    assert trace_of(tr1) == trace_of(info.lm[1]) and tr1.termination == 2, (trace_of(tr1), trace_of(info.lm[1]))
    want = np.concatenate([qb, tb]) * (1.0 if np.dot(qb, pose[:4]) >= 0 else -1.0)
    want[4:] = tb
    print("chained pose error:", np.abs(pose - want).max())
    assert np.abs(pose - want).max() <= 1e-8, np.abs(pose - want)
    # the new window frame: the edges under the returned pose
    w, nf = g.window()
    T_ret, _ = orc.pose_ops(pose[:4], pose[4:])
    ref = orc.transform(T_ret, e)
    assert nf == 1 and w.shape == ref.shape
    ulp = np.spacing(np.maximum(np.abs(w[:, :3]), np.abs(ref[:, :3])).astype(np.float32))
    assert (np.abs(w[:, :3] - ref[:, :3]) <= ulp).all() and np.array_equal(w[:, 3], ref[:, 3])
    cov = g.wait_pose_covariance(0, 0)
    assert cov["scan_index"] == 0 and (cov["flags"] & api.COV_VALID) and not (cov["flags"] & api.COV_NO_SOLVE), cov["flags"]
    assert np.array_equal(g.pose_log(0, 0, 1)[0][0], pose)
    g.attach_mapper(None)
    g.close(); m.close()


@pytest.mark.parametrize("export_before_first_scan", [False, True])
def test_continuation_after_export_and_import(orc, synth, export_before_first_scan):
    scans = [t[0] for t in lm.traversal(orc, synth, 1)[:8]]
    seed = lm.seeds(orc, synth)["truth"]
    g1, m1 = _handle(), _site_map(orc, synth)
    g1.attach_map_reader(m1, *lm.CELLS)
    g1.seed_stream(seed)
    first = 0 if export_before_first_scan else 1
    if not export_before_first_scan:
        g1.process_scan(scans[0], H, W)
    saved = (g1.export_stream_state(0), m1.export_state())
    assert api.parse_stream_state(saved[0])["received_map"].shape[0] == 1609
    g2, m2 = _handle(), la.Map(max_cells=96, cell_capacity=32768)
    m2.import_state(saved[1])
    g2.import_stream_state(0, saved[0])
    g2.attach_map_reader(m2, *lm.CELLS)
    assert same(g2.received_map(), g1.received_map())
    for k in range(first, first + (7 if export_before_first_scan else 6)):
        pa, ia = g1.process_scan(scans[k], H, W)
        pb, ib = g2.process_scan(scans[k], H, W)
        assert np.array_equal(pa, pb), k
        assert ia.scan_index == ib.scan_index == k, k
        assert same(g1.received_map(), g2.received_map()), k
    for g, m in ((g1, m1), (g2, m2)):
        assert m.status() == 0
        g.attach_mapper(None)
        g.close(); m.close()


def test_sixteen_lockstep_streams_read_one_map(orc, synth):
    S, n = 16, 8
    tr = lm.traversal(orc, synth, 1)[:n]
    scans = [t[0] for t in tr]

    def run(disturb):
        g, m = _handle(S, pose_log_capacity=n + 4), _site_map(orc, synth)
        for s in range(S):
            g.attach_map_reader(m, *lm.CELLS, stream=s)
        assert g.modes()["map_readers"] == "16" and g.modes()["n_streams"] == "16"
        before = m.export_state()
        g.alloc_resident(n)
        for s in range(S):
            for k in range(n):
                g.upload_scan(s, k, scans[k])
        for k in range(n - 1):
            if disturb and k == 4:
                g.seed_stream(tr[4][2], stream=5)
            g.process_resident(k, H * W, H, W, readback=True)
        # a subset step: the odd streams sit it out
        sitting = list(range(1, S, 2))
        recv_before = [g.received_map(stream=s) for s in sitting]
        g.process_resident_subset(n - 1, list(range(0, S, 2)), H * W, H, W, readback=True)
        for s, rb in zip(sitting, recv_before):
            assert rb.shape[0] == 1609 and same(rb, g.received_map(stream=s)), s
        logs = [g.pose_log(s, 0, (n - 1 - (4 if (disturb and s == 5) else 0)) + (1 - s % 2))[0] for s in range(S)]
        recv = [g.received_map(stream=s) for s in range(S)]
        assert m.export_state() == before and m.status() == 0
        for s in range(S):
            g.attach_mapper(None, stream=s)
        assert "map_readers" not in g.modes()
        g.close(); m.close()
        return logs, recv

    logs, recv = run(False)
    for s in range(1, S):      # streams fed equal data give equal bits
        assert np.array_equal(logs[s][:n - 1], logs[0][:n - 1]), s
        assert same(recv[s], recv[s % 2]), s
    one = _one_stream_reader_run(orc, synth, n)
    for k in range(n):         # ... and stream 0 is the one-stream handle's run within the cross-shape bars
        assert _pose_close(logs[0][k], one[k][0], POSE_TOL_T, POSE_TOL_R), k
    assert same(recv[0], one[n - 1][1])
    dlogs, drecv = run(True)
    for s in range(S):
        if s == 5:
            assert dlogs[5].shape[0] == 3 and not np.array_equal(dlogs[5], logs[5][4:])      # its scan 4 was its first, from the seed
            continue
        assert np.array_equal(dlogs[s], logs[s]) and same(drecv[s], recv[s]), s


def test_per_stream_launches_give_the_rows_kernels_bits(orc, synth, monkeypatch):
    """LIODOM_MAP_ROWS=0 (and extents the LDS plan cannot hold) send a reader through k_map_local_plan + k_map_gather, stream by
    stream: the same received maps and poses as through k_map_local_rows, to the bit — on a lock-step handle with a subset step."""
    S, n = 16, 5
    scans = [t[0] for t in lm.traversal(orc, synth, 1)[:n]]

    def run(rows, cells):
        monkeypatch.setenv("LIODOM_MAP_ROWS", "1" if rows else "0")
        g, m = _handle(S, pose_log_capacity=n + 4), _site_map(orc, synth)
        for s in range(S):
            g.attach_map_reader(m, *cells, stream=s)
        assert g.modes()["map_rows"] == ("1" if rows else "0")
        g.alloc_resident(n)
        for s in range(S):
            for k in range(n):
                g.upload_scan(s, k, scans[(k + s) % n])
        for k in range(n - 1):
            g.process_resident(k, H * W, H, W, readback=True)
        g.process_resident_subset(n - 1, [1, 2, 7, 15], H * W, H, W, readback=True)
        out = [(g.pose_log(s, 0, n - 1 + (1 if s in (1, 2, 7, 15) else 0))[0], g.received_map(stream=s)) for s in range(S)]
        assert m.status() == 0
        for s in range(S):
            g.attach_mapper(None, stream=s)
        g.close(); m.close()
        return out

    a, b = run(True, lm.CELLS), run(False, lm.CELLS)
    for s in range(S):
        assert np.array_equal(a[s][0], b[s][0]) and same(a[s][1], b[s][1]) and a[s][1].shape[0] > 0, s
    # 16 / 1 visits 33 x 33 + 3 keys: over the plan's cap whatever the switch says; 15 / 1 is the largest square it holds
    c, d = run(True, (16, 1)), run(True, (15, 1))
    for s in range(S):
        assert np.array_equal(c[s][0], d[s][0]) and same(c[s][1], d[s][1]), s


def _batch_poses(orc, synth):
    base = [T_of(t[2]) for t in lm.traversal(orc, synth, 1)[:3]]
    out = list(base)
    for t in ((-35.3, -12.7, -3.2), (39.6, 0.2, 0.0), (40.4, -0.2, 0.9), (-0.4, -0.6, 0.3), (-40.2, 19.9, 49.7), (0.9, 39.99, -0.99), (79.5, -80.5, 24.6),
              (-39.999, -40.001, 50.2)):
        T = base[1].copy()
        T[:, 3] = t
        out.append(T)
    out.append(out[3].copy())      # equal poses in two rows
    return out


@pytest.mark.parametrize("cells", [(2, 1), (0, 0), (1, 2)])
def test_local_batch_against_the_loop_and_the_oracle(orc, synth, cells):
    m, mo = _site_map(orc, synth), lm.site_map(orc, synth)
    poses = _batch_poses(orc, synth)
    many = [poses[i % len(poses)] for i in range(33)]
    for rows in (poses[:1], many):
        got = m.get_local_batch(np.array(rows), *cells)
        assert len(got) == len(rows)
        for i, T in enumerate(rows):
            assert same(got[i], m.get_local(T, *cells)) and same(got[i], mo.local(T, *cells)), (cells, i)
    sizes = [c.shape[0] for c in got]
    assert max(sizes) > 0 and (cells != (0, 0) or any(same(c[:c.shape[0] // 2], c[c.shape[0] // 2:]) and c.shape[0] > 0 for c in got))   # 0 / 0: the centre cell twice
    # one point short: LIODOM_ERR_CAPACITY, the sizes reported
    with pytest.raises(la.LiodomError) as err:
        m.get_local_batch(np.array(many), *cells, cap_per_row=max(sizes) - 1)
    assert err.value.code == api.ERR_CAPACITY and list(err.value.sizes) == sizes
    assert len(m.get_local_batch(np.array(many), *cells, cap_per_row=max(sizes))) == 33
    assert m.status() == 0
    m.close()


def test_local_batch_empty_map_and_the_fallback_over_the_plan_cap(orc, synth):
    empty = la.Map(**CAPS)
    poses = _batch_poses(orc, synth)
    assert [c.shape[0] for c in empty.get_local_batch(np.array(poses), 2, 1)] == [0] * len(poses)
    empty.close()
    # 33 x 33 + 3 keys: more than the LDS plan of k_map_local_rows holds (1024): the two old launches, row by row
    m, mo = _site_map(orc, synth), lm.site_map(orc, synth)
    got = m.get_local_batch(np.array(poses[:4]), 16, 1)
    for i, T in enumerate(poses[:4]):
        assert got[i].shape[0] > 0 and same(got[i], m.get_local(T, 16, 1)) and same(got[i], mo.local(T, 16, 1)), i
    # 31 x 31 + 3 = 964 keys: the largest square the plan holds
    got = m.get_local_batch(np.array(poses[:4]), 15, 1)
    for i, T in enumerate(poses[:4]):
        assert same(got[i], m.get_local(T, 15, 1)) and same(got[i], mo.local(T, 15, 1)), i
    assert m.status() == 0
    m.close()


def test_errors_leave_handle_and_map_untouched(orc, synth):
    seed = lm.seeds(orc, synth)["truth"]
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    # mapping = 0
    g0 = _handle(mapping=0, recv_capacity=0)
    assert g0.L.liodom_seed_stream(g0.h, 0, dp(seed)) == api.ERR_UNSUPPORTED
    m = _site_map(orc, synth)
    assert g0.L.liodom_attach_map_reader(g0.h, 0, m.h, 2, 1) == api.ERR_UNSUPPORTED
    g0.close()
    g = _handle(2)
    g.attach_map_reader(m, *lm.CELLS, stream=0)
    g.process_scan(lm.traversal(orc, synth, 1)[0][0], H, W)
    state, mstate = g.export_stream_state(0), m.export_state()
    bad = seed.copy(); bad[5] = np.nan
    assert g.L.liodom_seed_stream(g.h, 0, dp(bad)) == api.ERR_INVALID_ARG
    bad = seed.copy(); bad[:4] *= 1.001
    assert g.L.liodom_seed_stream(g.h, 0, dp(bad)) == api.ERR_INVALID_ARG
    assert g.L.liodom_seed_stream(g.h, 2, dp(seed)) == api.ERR_INVALID_ARG
    # a map is read or written, not both — in either order
    assert g.L.liodom_attach_mapper(g.h, 1, m.h, 2, 1) == api.ERR_INVALID_ARG
    assert g.modes()["map_readers"] == "1"
    w = la.Map(**CAPS)
    g.attach_mapper(w, 2, 1, stream=1)
    assert g.L.liodom_attach_map_reader(g.h, 0, w.h, 2, 1) == api.ERR_INVALID_ARG
    assert g.L.liodom_attach_map_reader(g.h, 0, m.h, -1, 1) == api.ERR_INVALID_ARG
    assert g.modes()["map_readers"] == "1"
    assert g.export_stream_state(0) == state and m.export_state() == mstate and w.num_cells() == 0
    # still attached as before: a reader keeps import / reset out, and the writer writes
    with pytest.raises(la.LiodomError) as err:
        m.reset()
    assert err.value.code == api.ERR_BUSY
    g.attach_mapper(None, stream=0); g.attach_mapper(None, stream=1)
    g.close(); w.close()
    # a local map larger than recv_capacity at the seed
    gs = _handle(recv_capacity=1000)
    gs.attach_map_reader(m, *lm.CELLS)
    state = gs.export_stream_state(0)
    assert gs.L.liodom_seed_stream(gs.h, 0, dp(seed)) == api.ERR_CAPACITY
    assert gs.export_stream_state(0) == state and m.export_state() == mstate and m.status() == 0
    gs.attach_mapper(None)
    gs.close(); m.close()


def test_replay_harness_localises_in_a_saved_map(orc, synth, tmp_path):
    """liodom_replay mapping=true map_state_in=FILE localize=1 seed_pose=..: the host mirror (LaserOdometer::attachMapReader and
    seed) gives the poses of the Python handle, and the map it prints at the end is the one it was given."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (run __graft_entry__.build())"
    n = 6
    scans = [t[0] for t in lm.traversal(orc, synth, 1)[:n]]
    seed = lm.seeds(orc, synth)["perturbed"]
    g, m = _handle(), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    g.seed_stream(seed)
    rows = [T_of(g.process_scan(x, H, W)[0]).reshape(12) for x in scans]
    g.attach_mapper(None)
    g.close()
    blob = m.export_state()
    m.close()
    scan_dir, out_dir, state = tmp_path / "scans", tmp_path / "out", tmp_path / "site.map"
    scan_dir.mkdir(); out_dir.mkdir()
    state.write_bytes(blob)
    for k, x in enumerate(scans):
        x.astype(np.float32).tofile(str(scan_dir / ("%06d.bin" % k)))
    r = subprocess.run([exe, str(scan_dir), str(out_dir) + "/", "scan_lines=%d" % H, "scan_regions=%d" % R, "edges_per_region=%d" % EPR,
                        "prev_frames=%d" % P, "mapping=true", "map_state_in=%s" % state, "map_state_out=%s" % (tmp_path / "after.map"), "localize=1",
                        "seed_pose=" + ",".join("%.17g" % v for v in seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.loadtxt(str(out_dir / "poses.txt")).reshape(-1, 12)
    assert np.allclose(got, np.array(rows), rtol=2e-5, atol=2e-6)
    found = re.search(r"map: (\d+) points in (\d+) cells", r.stdout)
    assert found and (int(found.group(1)), int(found.group(2))) == (2640, 29)
    assert (tmp_path / "after.map").read_bytes() == blob
    # without a saved map there is nothing to localise in
    r = subprocess.run([exe, str(scan_dir), str(out_dir) + "/", "scan_lines=%d" % H, "mapping=true", "localize=1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "map_state_in" in r.stderr
