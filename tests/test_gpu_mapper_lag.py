"""The lagged mapper (liodom_attach_mapper_ex with lag = 1): what leaves the sliding window enters the attached map, bit for bit;
the loop solves where the synchronous replay degenerates; other streams, sat-out steps and checkpoints are not disturbed; and
lag = 0 through the new entry point is liodom_attach_mapper."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
from mapper_lag_common import (EPR, H, K, P, POSE_TOL_R, POSE_TOL_T, R, W, T_of, map_part_correspondences, oracle_lagged_run, rot_angle,
                               same, scans_of)

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)


def _handle(n_streams=1, **cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(n_streams=n_streams, max_points=H * W, max_width=W, recv_capacity=1 << 16, **cfg))


def test_lagged_mapper_is_the_window_overflow_bit_for_bit(synth):
    g, mA, mB = _handle(), la.Map(**CAPS), la.Map(**CAPS)
    g.attach_mapper(mA, 2, 1, lag=1)
    assert g.modes()["mapper_lag"] == "1" and g.modes()["early_rebuild"] == "0" and g.modes()["chain"] == "0"
    n_edges = []
    for j, x in enumerate(scans_of(synth)):
        w, nf = g.window()
        leaving = w[:n_edges[j - P]].copy() if nf == P else None      # the oldest frame the window shows before the step
        assert (leaving is not None) == (j >= P)
        pose, info = g.process_scan(x, H, W)
        n_edges.append(info.n_edges)
        if leaving is None:
            assert g.received_map().shape[0] == 0 and mA.num_cells() == 0, j
            continue
        assert leaving.shape[0] > 100
        mB.update(leaving, np.eye(4)[:3])
        assert same(mB.get_local(T_of(pose), 2, 1), g.received_map()), j
        assert same(mB.all(), mA.all()) and mB.num_cells() == mA.num_cells(), j
        # ... and nothing of it is in the window the next scan searches
        w_after, _ = g.window()
        assert same(w_after[:n_edges[j - P + 1]], w[leaving.shape[0]:leaving.shape[0] + n_edges[j - P + 1]]), j
    assert mA.status() == 0 and mA.num_cells() > 0 and mA.all().shape[0] > 1000
    g.attach_mapper(None)
    assert "mapper_lag" not in g.modes()
    g.close(); mA.close(); mB.close()


def test_lagged_mapper_against_the_oracle(orc, synth):
    run = oracle_lagged_run(orc, synth)
    g, m = _handle(), la.Map(**CAPS)
    g.attach_mapper(m, 2, 1, lag=1)
    used_map = 0
    for j, x in enumerate(scans_of(synth)):
        n_window = g.window()[0].shape[0]
        pose, info = g.process_scan(x, H, W)
        rec = run[j]
        assert np.linalg.norm(pose[4:] - rec["pose"][4:]) <= POSE_TOL_T and rot_angle(pose[:4], rec["pose"][:4]) <= POSE_TOL_R, j
        if j == 0:
            continue
        assert [info.lm[i].termination for i in (0, 1)] == rec["term"], j
        assert [info.lm[i].iterations for i in (0, 1)] == rec["iters"], j
        if j >= P:
            assert 5 not in [info.lm[i].termination for i in (0, 1)], j
        assert n_window == rec["n_window"], j
        for it in (0, 1):
            vo, ao, _ = rec["corr"][it]
            vg, ag, _ = g.correspondences(it)
            assert vo.shape == vg.shape, (j, it)
            diff = int((vo != vg).sum()) + int(((ao != ag) & (vo == 1) & (vg == 1)).sum())
            assert diff <= 3, (j, it, diff)
            if j > P:
                used_map += int((ag[vg == 1] >= n_window).sum())
    assert used_map > 50, used_map
    assert sum(map_part_correspondences(r) for r in run) > 50
    assert m.status() == 0
    g.attach_mapper(None)
    g.close(); m.close()


def test_lag_leaves_other_streams_and_sat_out_steps_alone(synth):
    """Stream 0 lagged, stream 1 without a mapper; a subset step that lists stream 1 only."""
    n = 9
    scans = [scans_of(synth, s, n) for s in range(2)]
    steps = [("all", k) for k in range(6)] + [("one", 6), ("all", 7), ("all", 8)]

    def run(with_mapper):
        g = _handle(2, pose_log_capacity=n + 4)
        m = la.Map(**CAPS) if with_mapper else None
        if m is not None:
            g.attach_mapper(m, 2, 1, stream=0, lag=1)
        g.alloc_resident(n)
        for s in range(2):
            for k in range(n):
                g.upload_scan(s, k, scans[s][k])
        checked = False
        for kind, slot in steps:
            if kind == "all":
                g.process_resident(slot, H * W, H, W, readback=True)
                continue
            before = (m.export_state(), g.received_map(stream=0), g.window(stream=0)[0]) if m is not None else None
            g.process_resident_subset(slot, [1], H * W, H, W, readback=True)
            if m is not None:
                assert before[0] == m.export_state() and same(before[1], g.received_map(stream=0)) and same(before[2], g.window(stream=0)[0])
                assert len(before[1]) > 0 and m.num_cells() > 0
                checked = True
        logs = [g.pose_log(s, 0, n_s)[0] for s, n_s in ((0, n - 1), (1, n))]
        recv1 = g.received_map(stream=1)
        cells = m.num_cells() if m is not None else 0
        if m is not None:
            assert checked and m.status() == 0
            g.attach_mapper(None, stream=0)
            m.close()
        g.close()
        return logs, recv1, cells

    (log0, log1, ), recv1, cells = run(True)
    (ref0, ref1, ), ref_recv1, _ = run(False)
    assert np.array_equal(log1, ref1) and recv1.shape[0] == 0 and ref_recv1.shape[0] == 0
    assert cells > 0 and not np.array_equal(log0, ref0)      # stream 0 did search its map


def test_checkpoint_resumes_a_lagged_run(synth):
    scans = scans_of(synth)
    g1, m1 = _handle(), la.Map(**CAPS)
    g1.attach_mapper(m1, 2, 1, lag=1)
    full, saved = [], None
    for k in range(K):
        p, _ = g1.process_scan(scans[k], H, W)
        full.append((p.copy(), g1.received_map()))
        if k == 8:
            saved = (g1.export_stream_state(0), m1.export_state())
    assert len(full[8][1]) > 0 and m1.status() == 0
    g1.attach_mapper(None)
    g1.close(); m1.close()
    g2, m2 = _handle(), la.Map(max_cells=96, cell_capacity=32768)
    m2.import_state(saved[1])
    g2.import_stream_state(0, saved[0])
    g2.attach_mapper(m2, 2, 1, lag=1)
    assert same(g2.received_map(), full[8][1])
    for k in range(9, K):
        p, _ = g2.process_scan(scans[k], H, W)
        assert np.array_equal(p, full[k][0]), k
        assert same(g2.received_map(), full[k][1]), k
    assert m2.status() == 0
    g2.attach_mapper(None)
    g2.close(); m2.close()


def test_lag_zero_is_attach_mapper(synth):
    scans = scans_of(synth, count=6)
    out = []
    for ex in (False, True):
        g, m = _handle(), la.Map(**CAPS)
        if ex:
            o = api.MapperOptions()
            g.L.liodom_mapper_options_default(C.byref(o))
            g._check(g.L.liodom_attach_mapper_ex(g.h, 0, m.h, C.byref(o)))
        else:
            g._check(g.L.liodom_attach_mapper(g.h, 0, m.h, 2, 1))
        assert "mapper_lag" not in g.modes()
        out.append([(g.process_scan(x, H, W)[0].copy(), g.received_map()) for x in scans])
        assert m.num_cells() > 0 and len(out[-1][-1][1]) > 0
        g._check(g.L.liodom_attach_mapper_ex(g.h, 0, None, None))
        g.close(); m.close()
    for (pa, ra), (pb, rb) in zip(*out):
        assert np.array_equal(pa, pb) and same(ra, rb)


def test_replay_harness_runs_the_lagged_mapper(synth, tmp_path):
    """liodom_replay mapping=true mapper_lag=1 map_prune_period=..: the host mirror (LaserOdometer::attachMapper with options)
    gives the poses of the Python handle with the same options, and the tool prints the final cell count."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (run __graft_entry__.build())"
    n = 8
    scans = scans_of(synth, count=n)
    opts = dict(lag=1, prune_period=3, keep_cells_xy=2, keep_cells_z=1)
    g, m = _handle(), la.Map(20.0, 25.0, 0.4, **CAPS)
    g.attach_mapper(m, 2, 1, **opts)
    rows = [T_of(g.process_scan(x, H, W)[0]).reshape(12) for x in scans]
    cells, points = m.num_cells(), m.all().shape[0]
    g.attach_mapper(None)
    g.close(); m.close()
    scan_dir, out_dir = tmp_path / "scans", tmp_path / "out"
    scan_dir.mkdir(); out_dir.mkdir()
    for k, x in enumerate(scans):
        x.astype(np.float32).tofile(str(scan_dir / ("%06d.bin" % k)))
    r = subprocess.run([exe, str(scan_dir), str(out_dir) + "/", "scan_lines=%d" % H, "scan_regions=%d" % R, "edges_per_region=%d" % EPR,
                        "prev_frames=%d" % P, "mapping=true", "voxel_xysize=20", "voxel_zsize=25", "mapper_lag=1", "map_prune_period=3",
                        "map_keep_xy=2", "map_keep_z=1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.loadtxt(str(out_dir / "poses.txt")).reshape(-1, 12)
    assert np.allclose(got, np.array(rows), rtol=2e-5, atol=2e-6)
    found = re.search(r"map: (\d+) points in (\d+) cells", r.stdout)
    assert found and (int(found.group(1)), int(found.group(2))) == (points, cells) and cells > 0
    assert np.fromfile(str(out_dir / "map.bin"), dtype=np.float32).reshape(-1, 4).shape[0] == points
