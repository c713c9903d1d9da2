"""getLocalMap on the device at its limits, on the designed worlds of tests/local_map_model.py: k_map_local_plan + k_map_gather
(liodom_map_get_local, attached mappers, LIODOM_MAP_ROWS=0) and k_map_local_rows (map readers, liodom_map_get_local_batch).

Every output is a copy, so every comparison is bit for bit: against the NumPy restatement (local_map_model.local), which
tests/test_local_map_model.py holds bit-equal to the CPU oracle, and against the oracle itself (orc.Map.local).
  host calls   twelve poses and four extents on `counts`, one at a time, all at once and over 33 rows; the largest extent the LDS
               plan of k_map_local_rows admits and the next one on a map of 2.5 x 1.5 m cells; LIODOM_ERR_CAPACITY below the size
  step path    a local map larger than recv_capacity: the first recv_capacity points in visit order, n_recv = recv_capacity, the
               sticky LIODOM_MAP_RESULT_OVERFLOW — for capacities that cut at 1, 256, 257, an entry's end, inside either copy of
               the centre cell and around the size; readers alone, four readers in lock step with a subset step, a writer; and
               five scans of the localising traversal that solve against exactly the truncated cloud
  plan limits  more than 4096 found cells; the planners' loop guard at 65536 iterations
Every handle and map is sized to its world.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import local_map_model as lmm
import localize_model as lm
from mapper_lag_common import EPR, H, P, POSE_TOL_R, POSE_TOL_T, R, W, T_of, rot_angle, same, scans_of

pytestmark = pytest.mark.gpu

OVERFLOW = 64          # LIODOM_MAP_RESULT_OVERFLOW


def device_map(name):
    """The world on the device, in a map sized to it."""
    w = lmm.world(name)
    m = la.Map(*w["sizes"], **w["caps"])
    m.import_state(lmm.blob(w))
    assert m.num_cells() == len(w["state"]["keys"]) and m.status() == 0
    return m


def handle(n_streams=1, recv_capacity=1 << 16, **cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(n_streams=n_streams, max_points=H * W, max_width=W, recv_capacity=recv_capacity, **cfg))


def expected(name, pose7, cells):
    w = lmm.world(name)
    return lmm.local(w["state"], T_of(pose7), w["sizes"], *cells)


# ---------------------------------------------------------------------------------------------
# host calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", lmm.COUNTS_EXTENTS)
def test_host_calls_on_counts(orc, cells):
    w, m, mo = lmm.world("counts"), device_map("counts"), lmm.oracle_map(orc, "counts")
    poses = lmm.COUNTS_POSES
    want = [lmm.local(w["state"], T, w["sizes"], *cells) for T in poses]
    for i, T in enumerate(poses):
        assert same(want[i], mo.local(T, *cells)), (cells, i)
        assert same(m.get_local(T, *cells), want[i]), (cells, i)
    got = m.get_local_batch(np.array(poses), *cells)
    assert len(got) == len(poses)
    for i in range(len(poses)):
        assert same(got[i], want[i]), (cells, i)
    got = m.get_local_batch(np.array([poses[i % len(poses)] for i in range(33)]), *cells)
    assert len(got) == 33
    for i in range(33):
        assert same(got[i], want[i % len(poses)]), (cells, i)
    assert want[0].shape[0] > 0 and want[10].shape[0] == 0 and m.status() == 0
    m.close()


def test_host_calls_at_the_edge_of_the_rows_plan(orc):
    """Sizes (2.5, 1.5): the largest cells_xy map_rows_fit admits goes through k_map_local_rows, the next one through the two old
    launches, row by row; the answer is the same on either path, and status 0 says that no plan was cut."""
    w, m, mo = lmm.world("frac"), device_map("frac"), lmm.oracle_map(orc, "frac")
    c, cz = lmm.frac_cells_xy(), lmm.FRAC_CELLS_Z
    assert lmm.rows_fit(w["sizes"], c, cz) and not lmm.rows_fit(w["sizes"], c + 1, cz)
    for cxy in (c, c + 1):
        want = [lmm.local(w["state"], T, w["sizes"], cxy, cz) for T in lmm.FRAC_POSES]
        got = m.get_local_batch(np.array(lmm.FRAC_POSES), cxy, cz)
        for i, T in enumerate(lmm.FRAC_POSES):
            assert same(want[i], mo.local(T, cxy, cz)), (cxy, i)
            assert same(got[i], want[i]) and same(m.get_local(T, cxy, cz), want[i]), (cxy, i)
        assert max(x.shape[0] for x in want) >= 100
    assert m.status() == 0
    m.close()


@pytest.mark.parametrize("cells", [(3, 0), (0, 0)])
def test_host_calls_below_the_size_report_capacity(cells):
    w, m = lmm.world("counts"), device_map("counts")
    poses = [lmm.COUNTS_POSES[0], lmm.COUNTS_POSES[9], lmm.COUNTS_POSES[10]]
    want = [lmm.local(w["state"], T, w["sizes"], *cells) for T in poses]
    totals = [x.shape[0] for x in want]
    assert min(totals) == 0 and totals[0] > 1 and totals[1] > 1
    fill = np.float32(-7.5)
    T0 = np.ascontiguousarray(poses[0], np.float64).reshape(12)
    Tn = np.ascontiguousarray(np.array(poses), np.float64).reshape(-1)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    total = totals[0]
    for cap in (0, 1, total - 1, total):
        buf = np.full((max(cap, 1), 4), fill, np.float32)
        n = C.c_int64(-1)
        rc = m._L.liodom_map_get_local(m.h, dp(T0), cells[0], cells[1], fp(buf), cap, C.byref(n))
        assert n.value == total, cap
        if cap < total:
            assert rc == api.ERR_CAPACITY and (buf == fill).all(), cap
        else:
            assert rc == 0 and same(buf, want[0]), cap
        assert m.status() == 0, cap
    total = max(totals)          # of the batch: its largest row
    for cap in (0, 1, total - 1, total):
        buf = np.full((len(poses), max(cap, 1), 4), fill, np.float32)
        sizes = np.full(len(poses), -1, np.int64)
        rc = m._L.liodom_map_get_local_batch(m.h, dp(Tn), len(poses), cells[0], cells[1], fp(buf), cap, sizes.ctypes.data_as(C.POINTER(C.c_int64)))
        assert list(sizes) == totals, cap
        if cap < total:
            assert rc == api.ERR_CAPACITY and (buf == fill).all(), cap
        else:
            assert rc == 0, cap
            for i in range(len(poses)):
                assert same(buf[i, :totals[i]], want[i]) and (buf[i, totals[i]:] == fill).all(), (cap, i)
        assert m.status() == 0, cap
    m.close()


# ---------------------------------------------------------------------------------------------
# the step path at recv_capacity
# ---------------------------------------------------------------------------------------------
FAR = np.array([0.0, 0.0, 0.0, 1.0, 1000.0, -1000.0, 0.0])      # nothing of `counts` around it


def reader_run(synth, cap, rows, monkeypatch):
    """One reader of `counts` on a handle of recv_capacity = cap: the scan at the origin, then a scan from a seed far away, whose
    local map is empty and fits.  -> per scan (pose, received map, map status)."""
    monkeypatch.setenv("LIODOM_MAP_ROWS", "1" if rows else "0")
    scans = scans_of(synth, count=2)
    g, m = handle(recv_capacity=cap), device_map("counts")
    g.attach_map_reader(m, *lmm.STEP_EXTENTS)
    assert g.modes()["map_rows"] == ("1" if rows else "0")
    out = []
    pose, _ = g.process_scan(scans[0], H, W)
    out.append((pose.copy(), g.received_map(), m.status()))
    g.seed_stream(FAR)
    assert g.received_map().shape[0] == 0
    pose, _ = g.process_scan(scans[1], H, W)
    out.append((pose.copy(), g.received_map(), m.status()))
    g.attach_mapper(None)
    g.close(); m.close()
    return out


@pytest.mark.parametrize("which", lmm.STEP_CAP_NAMES)
def test_reader_step_truncates_at_recv_capacity(synth, monkeypatch, which):
    cap = lmm.step_caps(lmm.world("counts"))[which]
    runs = [reader_run(synth, cap, rows, monkeypatch) for rows in (True, False)]
    for rows, run in zip((True, False), runs):
        pose, recv, status = run[0]
        want = expected("counts", pose, lmm.STEP_EXTENTS)
        total = want.shape[0]
        print("%s rows=%d: cap %d, total %d, received %d, status %d" % (which, rows, cap, total, recv.shape[0], status))
        assert np.array_equal(pose[4:], np.zeros(3)) and total == lmm.step_caps(lmm.world("counts"))["total"]
        assert recv.shape[0] == min(cap, total) and same(recv, want[:cap]), (which, rows)
        assert bool(status & OVERFLOW) == (total > cap) and (status & ~OVERFLOW) == 0, (which, rows, status)
        # a later step that fits leaves the bit as it is
        pose1, recv1, status1 = run[1]
        want1 = expected("counts", pose1, lmm.STEP_EXTENTS)
        assert want1.shape[0] <= cap and same(recv1, want1) and status1 == status, (which, rows, status1)
    for a, b in zip(*runs):
        assert np.array_equal(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2], which


def test_lockstep_readers_on_both_sides_of_the_capacity(synth, monkeypatch):
    """Four streams read `counts` in lock step with recv_capacity = the size of stream 0's local map; streams 1 - 3 start from
    imported states at other poses.  Then a subset step of two streams (the kList instantiation of k_map_local_rows)."""
    monkeypatch.setenv("LIODOM_MAP_ROWS", "1")
    w = lmm.world("counts")
    cap = lmm.lockstep_cap(w)
    S = 4
    cells = [lmm.LOCKSTEP_EXTENTS, lmm.STEP_EXTENTS, lmm.STEP_EXTENTS, lmm.STEP_EXTENTS]
    starts = [None, lmm.COUNTS_POSES[1], lmm.COUNTS_POSES[10], lmm.COUNTS_POSES[9]]
    src = handle(recv_capacity=16)
    g, m = handle(S, recv_capacity=cap), device_map("counts")
    for s in range(1, S):
        src.seed_stream(np.concatenate([[0.0, 0.0, 0.0, 1.0], starts[s][:, 3]]))
        g.import_stream_state(s, src.export_stream_state(0))
    src.close()
    for s in range(S):
        g.attach_map_reader(m, *cells[s], stream=s)
    assert g.modes()["map_rows"] == "1" and g.modes()["map_readers"] == "4"
    scans = scans_of(synth, count=2)
    g.alloc_resident(2)
    for s in range(S):
        for k in range(2):
            g.upload_scan(s, k, scans[k])
    poses, _ = g.process_resident(0, H * W, H, W, readback=True)
    recv = [g.received_map(stream=s) for s in range(S)]
    totals = []
    for s in range(S):
        want = expected("counts", poses[s], cells[s])
        totals.append(want.shape[0])
        assert same(recv[s], want[:cap]), s
    print("lock step: cap %d, totals %s" % (cap, totals))
    assert totals[0] == cap and totals[1] > cap and totals[2] == 0 and totals[3] > cap and min(t for t in totals if t) <= cap
    assert m.status() == OVERFLOW
    poses2, _ = g.process_resident_subset(1, [0, 2], H * W, H, W, readback=True)
    for s in (1, 3):
        assert recv[s].shape[0] == cap and same(g.received_map(stream=s), recv[s]), s
    for i, s in enumerate((0, 2)):
        assert same(g.received_map(stream=s), expected("counts", poses2[i], cells[s])[:cap]), s
    assert m.status() == OVERFLOW
    for s in range(S):
        g.attach_mapper(None, stream=s)
    g.close(); m.close()


def test_writer_step_truncates_at_recv_capacity(orc, synth):
    """liodom_attach_mapper with a recv_capacity between the map's size around the pose after scan 0 and after scan 1.  The oracle
    map is updated with the oracle's own edges and poses (the synchronous replay: every pose is the prediction, bit for bit)."""
    po = orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, knn_mode=1, mapping=1)
    od, mo = orc.Odometer(po), orc.Map()
    scans = scans_of(synth, count=2)
    want = []
    for x in scans:
        e = orc.extract(po, x, H, W)["edges"]
        pose, _ = od.step(e)
        mo.update(e, T_of(pose))
        want.append(mo.local(T_of(pose), 2, 1))
        assert same(want[-1], od.received_map())
    od.close()
    n0, n1 = want[0].shape[0], want[1].shape[0]
    cap = (n0 + n1) // 2
    print("writer: %d points after scan 0, %d after scan 1, recv_capacity %d" % (n0, n1, cap))
    assert 0 < n0 < cap < n1
    g, mg = handle(recv_capacity=cap), la.Map(max_cells=64, cell_capacity=4096)
    g.attach_mapper(mg, 2, 1)
    g.process_scan(scans[0], H, W)
    assert same(g.received_map(), want[0]) and mg.status() == 0
    g.process_scan(scans[1], H, W)
    recv = g.received_map()
    assert recv.shape[0] == cap and same(recv, want[1][:cap])
    assert mg.status() == OVERFLOW
    g.attach_mapper(None)
    g.close(); mg.close()


def _corr_equal(got, want):
    (vg, ag, bg), (vo, ao, bo) = got, want
    ok = vg == 1
    return vg.shape == vo.shape and np.array_equal(vg, vo) and np.array_equal(ag[ok], ao[ok]) and np.array_equal(bg[ok], bo[ok])


def test_scans_after_the_truncation_solve_against_the_truncated_cloud(orc, synth):
    """The site map and the localising traversal of tests/localize_model.py, unseeded, with recv_capacity = 1000 below the local
    map's 1609 points: every scan searches window ++ the first 1000 points, n_recv == recv_capacity.  The oracle odometer is fed
    exactly that cloud."""
    cap, n = 1000, 5
    mo = lm.site_map(orc, synth)
    m = la.Map(max_cells=32, cell_capacity=4096)
    for e, T in lm.site_updates(orc, synth):
        m.update(e, T)
    assert same(m.all(), mo.all()) and m.status() == 0
    g = handle(recv_capacity=cap)
    g.attach_map_reader(m, *lm.CELLS)
    od = orc.Odometer(lm.params(orc))
    for j, (x, e, _) in enumerate(lm.traversal(orc, synth, 1)[:n]):
        n_window, recv = g.window()[0].shape[0], g.received_map()
        assert same(recv, od.received_map()) and recv.shape[0] == (cap if j else 0) and n_window == od.window().shape[0], j
        pose_o, info_o = od.step(e)
        pose_g, info_g = g.process_scan(x, H, W)
        full = mo.local(T_of(pose_o), *lm.CELLS)
        if j == 0:
            assert full.shape[0] == 1609
        assert full.shape[0] > cap, j
        od.set_received_map(full[:cap])
        print("scan %d: dt %.3e dr %.3e" % (j, np.linalg.norm(pose_g[4:] - pose_o[4:]), rot_angle(pose_g[:4], pose_o[:4])))
        assert np.linalg.norm(pose_g[4:] - pose_o[4:]) <= POSE_TOL_T and rot_angle(pose_g[:4], pose_o[:4]) <= POSE_TOL_R, j
        assert info_g.status == 0, (j, info_g.status)
        if j == 0:
            continue
        assert info_g.map_points == info_o.map_points, (j, info_g.map_points, info_o.map_points)
        assert [info_g.lm[i].termination for i in (0, 1)] == [info_o.lm[i].termination for i in (0, 1)], j
        assert [info_g.lm[i].iterations for i in (0, 1)] == [info_o.lm[i].iterations for i in (0, 1)], j
        for it in (0, 1):
            got = g.correspondences(it)
            assert _corr_equal(got, od.last_corr(it)), (j, it)
            assert int((got[1][got[0] == 1] >= n_window).sum()) > 0, (j, it)      # the truncated map is in use
    assert m.status() == OVERFLOW
    g.attach_mapper(None)
    g.close(); m.close(); od.close()


# ---------------------------------------------------------------------------------------------
# the plan's limits
# ---------------------------------------------------------------------------------------------
def test_more_found_cells_than_the_plan_holds(orc):
    """4201 found cells: the plan keeps the first 4096 in visit order and raises LIODOM_MAP_RESULT_OVERFLOW; 4096: all of them."""
    w, m = lmm.world("ones"), device_map("ones")
    T = lmm.ones_pose()
    got = m.get_local(T, 40, 0)
    want, over = lmm.local_device(w["state"], T, w["sizes"], 40, 0)
    assert over and want.shape[0] == lmm.ENTRIES_MAX and same(want, lmm.oracle_map(orc, "ones").local(T, 40, 0)[:lmm.ENTRIES_MAX])
    assert same(got, want) and m.status() == OVERFLOW
    m.close()
    w, m = lmm.world("ones-65x63"), device_map("ones-65x63")
    T = lmm.ones_pose(65, 63)
    got = m.get_local(T, 40, 0)
    assert got.shape[0] == lmm.ENTRIES_MAX and same(got, lmm.oracle_map(orc, "ones-65x63").local(T, 40, 0)) and m.status() == 0
    m.close()


def test_a_visit_cut_by_the_loop_guard_is_reported(orc):
    """cells_xy = 127 on 1 m cells stays under the planners' guard of 65536 loop iterations: the oracle's answer, status 0.
    cells_xy = 128 does not: the visit is cut where local_map_model.visit_cut says, and LIODOM_MAP_RESULT_OVERFLOW is raised
    (sticky = 0 or not: these are host calls)."""
    w, m, mo = lmm.world("guard"), device_map("guard"), lmm.oracle_map(orc, "guard")
    T = lmm.GUARD_POSE
    got = m.get_local(T, 127, 0)
    assert got.shape[0] == 17 and same(got, mo.local(T, 127, 0)) and m.status() == 0
    got = m.get_local(T, 128, 0)
    full = mo.local(T, 128, 0)
    want, over = lmm.local_device(w["state"], T, w["sizes"], 128, 0)
    assert over and want.shape[0] == full.shape[0] - 13 and same(want, full[:want.shape[0]])
    assert m.status() == OVERFLOW, "a visit cut by the loop guard left status %d" % m.status()
    assert same(got, want)
    # the batch call takes the same two launches for such an extent
    assert same(m.get_local_batch(np.array([T]), 128, 0)[0], want)
    m.close()
