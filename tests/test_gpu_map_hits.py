"""Per-scan map-hit records on the device: liodom_map_hit_rows (k_map_hit_rows, the batch form), liodom_set_map_hits /
liodom_get_map_hit_log (the step path and its kept occupancy) and Liodom.localize_scan.  Every count is compared for equality with
liodom_map_score_poses at the record's own matrix and, on the designed maps, with the NumPy model (tests/reloc_model.py).

Shapes.  k_map_hit_rows gives a row one 256-thread workgroup whose four waves stride the rounds of 64 edges: the boundaries are
0 | 1 | 63 | 64 | 65 edges (a wave's round) and 255 | 256 | 257 | 513 (the workgroup's round, a third round with one edge).  A launch
has one workgroup per row and no chunking: 1, 3, 4 and 5 rows with unequal counts."""
import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import localize_model as lm
import map_hits_model as mh
import reloc_model as rm
from mapper_lag_common import EPR, H, P, R, W, T_of, rot_angle

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)
SMALL = dict(max_cells=16, cell_capacity=256, max_update_points=1024, max_modified_cells=16)
ROW_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 513]
V, NR, NS = api.HIT_VALID, api.HIT_NO_READER, api.HIT_NO_SOLVE
_SITE = {}


def _handle(n_streams=1, mapping=1, **cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=mapping),
                     la.make_config(n_streams=n_streams, max_points=H * W, max_width=W, recv_capacity=1 << 16, **cfg))


def _site_blob(orc, synth):
    if "blob" not in _SITE:
        m = la.Map(**CAPS)
        for e, T in lm.site_updates(orc, synth):
            m.update(e, T)
        assert m.num_cells() == 29 and m.status() == 0
        _SITE["blob"] = m.export_state()
        m.close()
    return _SITE["blob"]


def _site_map(orc, synth, blob=None):
    m = la.Map(**CAPS)
    m.import_state(_site_blob(orc, synth) if blob is None else blob)
    return m


def _tiled(edges, n):
    return np.tile(edges, (-(-max(n, 1) // edges.shape[0]), 1))[:n].copy()


def _code(err):
    return int(str(err.value).split("error ")[1].split(":")[0])


def _rows_equal_score_poses_and_model(m, edges, T4, radius, counts):
    """hit_rows of len(counts) rows (row i: the first counts[i] of the tiled edges, shifted a little per row, under T4[i % 4])
    against score_poses row by row and against the model."""
    occ = rm.Occupancy(api.parse_map_state(m.export_state()))
    clouds, T = [], []
    for i, n in enumerate(counts):
        c = _tiled(edges, n)
        c[:, :3] += np.float32(0.05 * (i % 3))      # (rows differ in more than their length; NaN / inf stay what they are)
        clouds.append(c)
        T.append(T4[i % T4.shape[0]])
    T = np.array(T)
    got = m.hit_rows(clouds, T, radius=radius)
    assert got.dtype == np.int32 and got.shape == (len(counts), 2)
    for i, c in enumerate(clouds):
        want = m.score_poses(c, T[i:i + 1], radius=radius)[0]
        assert tuple(got[i]) == tuple(want), (i, counts[i], radius)
        assert tuple(got[i]) == tuple(occ.hits(c, T[i:i + 1], radius=radius)[0]), (i, counts[i], radius)
    return got


@pytest.mark.parametrize("radius", [0, 1])
def test_designed_rows(radius):
    m = la.Map(**SMALL)
    m.update(rm.DESIGNED_MAP)
    assert m.num_cells() == rm.DESIGNED_CELLS and m.status() == 0
    before = m.export_state()
    edges, want = rm.designed_edges()
    T4 = rm.designed_candidates()
    # the designed edges themselves, one row per candidate: the identity's known counts, the far candidate's zeros
    got = m.hit_rows([edges] * 4, T4, radius=radius)
    assert tuple(got[0]) == want[radius] and tuple(got[1]) == (0, 0)
    assert np.array_equal(got, m.score_poses(edges, T4, radius=radius))
    # NaN, inf and 2e6 edges miss, edge by edge, as they do in score_poses
    bad = np.array([i for i, (p, _, _) in enumerate(rm.DESIGNED_EDGES) if not np.isfinite(p).all() or max(np.abs(p)) >= 1e6])
    assert bad.shape[0] == 4
    assert not m.hit_rows([edges[i:i + 1] for i in bad], np.tile(T4[0], (bad.shape[0], 1)), radius=radius).any()
    # every round boundary in one call, then 1, 3, 4 and 5 rows with unequal counts
    got = _rows_equal_score_poses_and_model(m, edges, T4, radius, ROW_COUNTS)
    assert got[0].tolist() == [0, 0] and got[:, 0].max() > 0
    for counts in ([257], [65, 0, 513], [1, 256, 64, 63], [513, 1, 0, 255, 65]):
        _rows_equal_score_poses_and_model(m, edges, T4, radius, counts)
    # nothing to do is no error
    assert m.hit_rows([], np.zeros((0, 12)), radius=radius).shape == (0, 2)
    assert not m.hit_rows([edges[:0]] * 3, np.tile(T4[0], (3, 1)), radius=radius).any()
    assert m.status() == 0 and m.export_state() == before
    m.close()


@pytest.mark.parametrize("radius", [0, 1])
def test_designed_rows_on_the_first_and_last_word_of_a_cells_bitmap(radius):
    blob, edges, want, _ = rm.crafted_state_blob()
    m = la.Map(**SMALL)
    m.import_state(blob)
    I = np.eye(4)[:3].reshape(1, 12)
    assert tuple(m.hit_rows([edges], I, radius=radius)[0]) == want[radius]
    _rows_equal_score_poses_and_model(m, edges, np.concatenate([I, rm.designed_candidates()[2:3]]), radius, ROW_COUNTS)
    assert m.status() == 0 and m.export_state() == blob
    m.close()


def test_hit_rows_argument_rules():
    m = la.Map(**SMALL)
    m.update(rm.DESIGNED_MAP)
    edges, _ = rm.designed_edges()
    I = np.eye(4)[:3].reshape(1, 12)
    for radius in (-1, 2):
        with pytest.raises(la.LiodomError) as err:
            m.hit_rows([edges], I, radius=radius)
        assert err.value.code == api.ERR_INVALID_ARG
    with pytest.raises(la.LiodomError) as err:      # a row longer than max_update_points, as score_poses refuses it
        m.hit_rows([_tiled(edges, SMALL["max_update_points"] + 1)], I)
    assert err.value.code == api.ERR_INVALID_ARG
    assert m.hit_rows([_tiled(edges, SMALL["max_update_points"])], I).shape == (1, 2)
    m.close()


def _check_record(rec, info, pose, edges, m, radius, flags):
    assert int(rec["flags"]) == flags and int(rec["radius"]) == radius
    assert int(rec["scan_index"]) == info.scan_index and int(rec["n_edges"]) == info.n_edges == edges.shape[0]
    assert not rec["reserved"].any()
    want = m.score_poses(edges, rec["T"].reshape(1, 12), radius=radius)[0]
    assert (int(rec["hits_r"]), int(rec["hits_0"])) == tuple(want), (info.scan_index, want)
    d = np.abs(rec["T"] - T_of(pose)).max()
    print("scan %d: hits %d %d of %d, |T - T_of(pose)| %.2e" % (info.scan_index, rec["hits_r"], rec["hits_0"], rec["n_edges"], d))
    assert d <= 1e-12


@pytest.mark.parametrize("radius", [0, 1])
def test_step_records_equal_the_host_call(orc, synth, radius):
    tr = lm.traversal(orc, synth, 1)[:5]
    g, m = _handle(), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    g.set_map_hits(radius)
    assert g.modes()["map_hits"] == "1"
    before = m.export_state()
    for k, (x, _, _) in enumerate(tr):      # unseeded: the first scan does not solve
        pose, info = g.process_scan(x, H, W)
        rec = g.map_hits(k, 1)[0]
        _check_record(rec, info, pose, g.get_edges()["edges"], m, radius, (V | NS) if k == 0 else V)
    log = g.map_hits(0, len(tr) + 1)
    assert [int(f) for f in log["flags"]] == [V | NS] + [V] * (len(tr) - 1) + [0]
    assert log["scan_index"][:len(tr)].tolist() == list(range(len(tr)))
    # seeded at the truth: the first scan solves, and it lies in the map
    g.seed_stream(tr[0][2])
    assert g.modes()["map_hits"] == "1"
    for k, (x, _, _) in enumerate(tr[:2]):
        pose, info = g.process_scan(x, H, W)
        rec = g.map_hits(k, 1)[0]
        _check_record(rec, info, pose, g.get_edges()["edges"], m, radius, V)
        assert int(rec["hits_r"]) > info.n_edges // 2
    assert m.export_state() == before and m.status() == 0
    g.attach_mapper(None)
    g.close(); m.close()


def test_poses_do_not_change(orc, synth):
    tr = lm.traversal(orc, synth, 1)[:6]

    def run(radius):
        g, m = _handle(), _site_map(orc, synth)
        g.attach_map_reader(m, *lm.CELLS)
        if radius is not None:
            g.set_map_hits(radius)
        out = []
        for x, _, _ in tr:
            pose, info = g.process_scan(x, H, W)
            out.append((pose.tobytes(), bytes(info), g.received_map().tobytes()))
        assert ("map_hits" in g.modes()) == (radius is not None)
        g.attach_mapper(None)
        g.close(); m.close()
        return out

    off = run(None)
    assert run(1) == off and run(0) == off


def test_lockstep_and_subsets(orc, synth):
    """Streams 0, 1: readers of map A with radius 0 and 1; 2: a reader of map B; 3: a writing mapper; 4: nothing."""
    S, n = 5, 4
    scans = [t[0] for t in lm.traversal(orc, synth, 1)[:n]]
    g = _handle(S, pose_log_capacity=8)
    A, B, Cw = _site_map(orc, synth), _site_map(orc, synth), la.Map(**CAPS)
    B.prune(T_of(lm.traversal(orc, synth, 1)[0][2]), keep_xy=0, keep_z=0)      # B is not A
    assert 0 < B.num_cells() < A.num_cells()
    g.attach_map_reader(A, *lm.CELLS, stream=0)
    g.attach_map_reader(A, *lm.CELLS, stream=1)
    g.attach_map_reader(B, *lm.CELLS, stream=2)
    g.attach_mapper(Cw, stream=3)
    radius = [0, 1, 1, 1, 0]
    for s in range(S):
        g.set_map_hits(radius[s], stream=s)
    assert g.modes()["map_hits"] == "5"
    states = (A.export_state(), B.export_state())
    g.alloc_resident(n)
    for s in range(S):
        for k in range(n):
            g.upload_scan(s, k, scans[k])
    maps = {0: A, 1: A, 2: B}

    def check(streams, poses, infos, k_of):
        for i, s in enumerate(streams):
            rec = g.map_hits(k_of[s], 1, stream=s)[0]
            if s in maps:
                _check_record(rec, infos[i], poses[i], g.get_edges(stream=s)["edges"], maps[s], radius[s], (V | NS) if k_of[s] == 0 else V)
            else:
                assert int(rec["flags"]) == (NR | (NS if k_of[s] == 0 else 0)) and int(rec["scan_index"]) == k_of[s] == infos[i].scan_index
                assert (int(rec["hits_r"]), int(rec["hits_0"]), int(rec["n_edges"])) == (0, 0, 0) and int(rec["radius"]) == radius[s]
                assert np.abs(rec["T"] - T_of(poses[i])).max() <= 1e-12

    for k in range(3):
        poses, infos = g.process_resident(k, H * W, H, W)
        check(range(S), poses, infos, {s: k for s in range(S)})
    # a subset step: stream 1 sits it out
    kept = g.map_hits(0, 8, stream=1).tobytes()
    active = [0, 2, 3, 4]
    poses, infos = g.process_resident_subset(3, active, H * W, H, W)
    check(active, poses, infos, {s: 3 for s in active})
    assert g.map_hits(0, 8, stream=1).tobytes() == kept and int(g.map_hits(3, 1, stream=1)[0]["flags"]) == 0
    # radius 0 and 1 on one map, one pose: the counts differ only in hits_r
    r0, r1 = g.map_hits(2, 1, stream=0)[0], g.map_hits(2, 1, stream=1)[0]
    assert np.array_equal(r0["T"], r1["T"]) and int(r0["hits_0"]) == int(r1["hits_0"]) == int(r0["hits_r"]) < int(r1["hits_r"])
    assert (A.export_state(), B.export_state()) == states and A.status() == 0 and B.status() == 0
    for s in range(4):
        g.attach_mapper(None, stream=s)
    g.close(); A.close(); B.close(); Cw.close()


def _missing_edges(occ, edges, T, want):
    """Indices of the first `want` edges that hit nothing (radius 1) under T, from the model."""
    out = []
    for i in range(edges.shape[0]):
        if occ.hits(edges[i:i + 1], T.reshape(1, 12), radius=1)[0, 0] == 0:
            out.append(i)
            if len(out) == want:
                break
    return np.array(out, int)


def test_the_kept_occupancy_is_invalidated(orc, synth, capfd, monkeypatch):
    """Between steps the map is changed from the host — update, evict, merge_state, prune —: the next record equals score_poses on the
    changed map and differs from what the occupancy of the map before the change gives.  Without a change, a step builds nothing."""
    tr = lm.traversal(orc, synth, 1)[:7]
    g, m = _handle(), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    g.set_map_hits(1)
    g.seed_stream(tr[0][2])

    def step(k):
        pose, info = g.process_scan(tr[k][0], H, W)
        return g.map_hits(k, 1)[0], g.get_edges()["edges"]

    def builds():
        return capfd.readouterr().err.count("liodom map_hits occupancy")

    # the first step builds the occupancy, the second one, with nothing changed in between, does not
    monkeypatch.setenv("LIODOM_MAP_STATE_TIMING", "1")
    capfd.readouterr()
    rec0, e0 = step(0)
    assert builds() == 1
    rec1, e1 = step(1)
    assert builds() == 0
    monkeypatch.delenv("LIODOM_MAP_STATE_TIMING")
    # (score_poses, rebuilding as it always did, agrees with both — and only now touches the map's buffer)
    for rec, e in ((rec0, e0), (rec1, e1)):
        assert (int(rec["hits_r"]), int(rec["hits_0"])) == tuple(m.score_poses(e, rec["T"].reshape(1, 12))[0])

    def changed_then_step(k, change):
        """Applies `change` to the map, steps scan k; returns the record's counts, score_poses on the changed map and score_poses
        on a copy of the map as it was before the change: the stale occupancy's answer."""
        old = _site_map(orc, synth, blob=m.export_state())
        change()
        rec, e = step(k)
        got = (int(rec["hits_r"]), int(rec["hits_0"]))
        T = rec["T"].reshape(1, 12)
        new, stale = tuple(m.score_poses(e, T)[0]), tuple(old.score_poses(e, T)[0])
        old.close()
        print("scan %d: record %s, changed map %s, map before the change %s" % (k, got, new, stale))
        assert int(rec["flags"]) == V
        return got, new, stale

    # update: points on leaves that scan 2's edges probe and find empty (the model says which), placed under scan 2's ground truth
    occ = rm.Occupancy(api.parse_map_state(m.export_state()))
    T2 = T_of(tr[2][2])
    miss = _missing_edges(occ, tr[2][1], T2, 24)
    assert miss.shape[0] >= 8
    pts = np.concatenate([(tr[2][1][miss, :3].astype(np.float64) @ T2[:, :3].T + T2[:, 3]).astype(np.float32), np.ones((miss.shape[0], 1), np.float32)], axis=1)
    got, new, stale = changed_then_step(2, lambda: m.update(pts))
    assert got == new and got != stale and got[0] > stale[0]
    # evict everything but the pose's own cell, then merge the tile back: the cells come back under other ids
    T3 = T_of(tr[2][2])
    tile = {}
    got, new, stale = changed_then_step(3, lambda: tile.update(blob=m.evict(T3, keep_xy=0, keep_z=0)[0]))
    assert got == new and got != stale and got[0] < stale[0]
    got, new, stale = changed_then_step(4, lambda: m.merge_state(tile["blob"]))
    assert got == new and got != stale and got[0] > stale[0]
    # prune
    got, new, stale = changed_then_step(5, lambda: m.prune(T3, keep_xy=0, keep_z=0))
    assert got == new and got != stale and got[0] < stale[0]
    g.attach_mapper(None)
    g.close(); m.close()


def test_log_index_and_lifecycle(orc, synth):
    tr = lm.traversal(orc, synth, 1)[:6]
    scans = [t[0] for t in tr]
    cap = 4
    g, m = _handle(pose_log_capacity=cap), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    # never enabled: unsupported, nothing in the modes; switching off what was never on is no error and allocates nothing
    with pytest.raises(la.LiodomError) as err:
        g.map_hits(0, 1)
    assert _code(err) == api.ERR_UNSUPPORTED and "map_hits" not in g.modes()
    g.set_map_hits(-1)
    with pytest.raises(la.LiodomError) as err:
        g.map_hits(0, 1)
    assert _code(err) == api.ERR_UNSUPPORTED
    for bad in ((2, 0), (-2, 0), (1, 1), (1, -1)):
        with pytest.raises(la.LiodomError) as err:
            g.set_map_hits(bad[0], stream=bad[1])
        assert _code(err) == api.ERR_INVALID_ARG and "map_hits" not in g.modes()
    g.set_map_hits(1)
    # across the capacity: scans 4 and 5 get no record, as they get no pose-log entry; the range errors are the pose log's
    for x in scans:
        g.process_scan(x, H, W)
    log = g.map_hits(0, cap)
    assert log["scan_index"].tolist() == [0, 1, 2, 3] and [int(f) for f in log["flags"]] == [V | NS, V, V, V]
    assert g.map_hits(cap, 0).shape[0] == 0
    for first, count in ((3, 2), (-1, 1), (0, cap + 1), (cap, 1)):
        codes = []
        for call in (lambda: g.map_hits(first, count), lambda: g.pose_log(0, first, count)):
            with pytest.raises(la.LiodomError) as err:
                call()
            codes.append(_code(err))
        assert codes == [api.ERR_INVALID_ARG, api.ERR_INVALID_ARG], (first, count, codes)
    # reset_stream: the next scan is scan 0 again and does not solve; the setting survives
    g.reset_stream(0)
    assert g.modes()["map_hits"] == "1"
    _, info = g.process_scan(scans[0], H, W)
    rec = g.map_hits(0, 2)
    assert info.scan_index == 0 and int(rec[0]["flags"]) == (V | NS) and np.array_equal(rec[0]["T"], np.eye(4)[:3])
    assert int(rec[1]["flags"]) == V and rec[1].tobytes() == log[1].tobytes()      # (entries are overwritten, not cleared)
    # seed_stream: scan 0 again, solved
    g.seed_stream(tr[0][2])
    assert g.modes()["map_hits"] == "1"
    _, info = g.process_scan(scans[0], H, W)
    assert info.scan_index == 0 and int(g.map_hits(0, 1)[0]["flags"]) == V
    # export / import of the stream's state: the index goes back with the scan counter
    _, info = g.process_scan(scans[1], H, W)
    saved = g.export_stream_state(0)
    _, info = g.process_scan(scans[2], H, W)
    first = g.map_hits(2, 1)[0].copy()
    assert info.scan_index == 2 and int(first["flags"]) == V
    g.process_scan(scans[3], H, W)
    g.import_stream_state(0, saved)
    assert g.modes()["map_hits"] == "1"
    _, info = g.process_scan(scans[2], H, W)
    again = g.map_hits(2, 1)[0]
    assert info.scan_index == 2 and again.tobytes() == first.tobytes()
    # reset: the whole handle; then off: no further records
    g.reset()
    assert g.modes()["map_hits"] == "1"
    g.set_map_hits(-1)
    assert "map_hits" not in g.modes()
    kept = g.map_hits(0, cap).tobytes()
    g.process_scan(scans[0], H, W)
    assert g.map_hits(0, cap).tobytes() == kept
    g.attach_mapper(None)
    g.close(); m.close()
    # mapping = 0: unsupported
    g0 = _handle(mapping=0)
    with pytest.raises(la.LiodomError) as err:
        g0.set_map_hits(1)
    assert _code(err) == api.ERR_UNSUPPORTED
    g0.close()


def _kidnap_on_the_device(orc, synth, levels, seeded):
    """Liodom.localize_scan over the kidnap run of the model: one dict per scan (localize_scan's, plus the fraction)."""
    run = mh.kidnap_run(orc, synth)
    g, m = _handle(), _site_map(orc, synth)
    g.attach_map_reader(m, *lm.CELLS)
    if seeded:
        g.seed_stream([0, 0, 0, 1, 0, 0, 0])
    g.set_map_hits(mh.RADIUS)
    policy = api.TrackPolicy(run["min_fraction"], mh.LOST_AFTER)
    before, out = m.export_state(), []
    for j, (x, _, _, _) in enumerate(mh.kidnap_scans(orc, synth)):
        r = g.localize_scan(m, x, H, W, 0.1 * j, policy, levels)
        r["fraction"] = policy.fraction(r["hit"]["hits_r"], r["hit"]["hits_0"], r["hit"]["n_edges"])
        r["pose"] = r["pose"].copy()
        out.append(r)
    assert m.export_state() == before and m.status() == 0
    g.attach_mapper(None)
    g.close(); m.close()
    return out


def test_kidnap_and_recovery(orc, synth):
    run, scans = mh.kidnap_run(orc, synth), mh.kidnap_scans(orc, synth)
    want = mh.predicted_states(run["records"], run["min_fraction"])
    lost_at = want.index(api.LOST)
    assert lost_at == mh.TRACKED + mh.LOST_AFTER - 1
    got = _kidnap_on_the_device(orc, synth, mh.LEVELS, seeded=False)
    for j, r in enumerate(got):
        gt = scans[j][2]
        dt, dr = np.linalg.norm(r["pose"][4:] - gt[4:]), rot_angle(r["pose"][:4], gt[:4])
        print("scan %d (%d of the stream): %s, fraction %.3f (model %.3f), pose off by %.3f m %.4f rad" % (j, scans[j][3], r["state"], r["fraction"], run["records"][j]["fraction"], dt, dr))
        if j < lost_at:
            # before the policy's verdict the device answers what the model predicts: tracking, and after the jump below the threshold
            assert r["state"] == want[j] == api.TRACKING and r["relocalized"] is None
            assert (r["fraction"] >= run["min_fraction"]) == (j < mh.TRACKED), j
            assert int(r["hit"]["flags"]) == (V | NS if j == 0 else V) and r["info"].scan_index == j
        elif j == lost_at:
            assert r["state"] == api.LOST and r["relocalized"] is not None
            found = r["relocalized"]["pose"]
            # the relocaliser's grid residual, as tests/test_gpu_reloc_bnb.py checks it
            assert np.linalg.norm(found[4:] - gt[4:]) <= 0.15 and rot_angle(found[:4], gt[:4]) <= 0.011
            assert r["relocalized"]["fraction"] >= run["min_fraction"]
            # the same scan again, as the seeded stream's first: it solves, and it lies in the map
            assert r["info"].scan_index == 0 and int(r["hit"]["flags"]) == V and r["fraction"] >= run["min_fraction"]
            assert dt <= 0.15 and dr <= 0.011
        else:
            assert r["state"] == api.TRACKING and r["relocalized"] is None and r["fraction"] >= run["min_fraction"]
            assert r["info"].scan_index == j - lost_at and dt <= 0.15 and dr <= 0.011


def test_replay_writes_the_records_and_recovers(orc, synth, tmp_path):
    """liodom_replay localize=1 map_hits=FILE relocalize_below=..: the host mirror (LaserOdometer::setMapHits / mapHit, track_policy.h)
    writes the counts the Python handle's records hold for the same run — seeded at the identity, as the replay seeds, and searched
    over the replay's window — and recovers at the same scan."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (run __graft_entry__.build())"
    run, scans = mh.kidnap_run(orc, synth), mh.kidnap_scans(orc, synth)
    window = 4.7      # (ceil(4.7 / 0.4) = 12 steps either way: the Python run's nx, ny)
    levels = [dict(bnb=True, step_xy=0.4, step_yaw=0.02, nx=12, ny=12, nyaw=int(np.ceil(np.pi / 0.02))), mh.LEVELS[1]]
    got = _kidnap_on_the_device(orc, synth, levels, seeded=True)
    lost_at = [r["state"] for r in got].index(api.LOST)
    assert lost_at == mh.TRACKED + mh.LOST_AFTER - 1 and got[lost_at]["relocalized"] is not None
    scan_dir, out_dir, state, hits = tmp_path / "scans", tmp_path / "out", tmp_path / "site.map", tmp_path / "hits.txt"
    scan_dir.mkdir(); out_dir.mkdir()
    state.write_bytes(_site_blob(orc, synth))
    for k, (x, _, _, _) in enumerate(scans):
        x.astype(np.float32).tofile(str(scan_dir / ("%06d.bin" % k)))
    base = [exe, str(scan_dir), str(out_dir) + "/", "scan_lines=%d" % H, "scan_regions=%d" % R, "edges_per_region=%d" % EPR, "prev_frames=%d" % P,
            "mapping=true", "map_state_in=%s" % state, "localize=1"]
    r = subprocess.run(base + ["map_hits=%s" % hits, "hit_radius=%d" % mh.RADIUS, "relocalize_below=%.17g" % run["min_fraction"],
                               "lost_after=%d" % mh.LOST_AFTER, "reloc_window=%g" % window], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = np.loadtxt(str(hits), dtype=np.int64).reshape(-1, 4)
    want = np.array([[x["hit"]["scan_index"], x["hit"]["hits_r"], x["hit"]["hits_0"], x["hit"]["n_edges"]] for x in got], np.int64)
    assert np.array_equal(rows, want), (rows, want)
    assert [int(v) for v in re.findall(r"relocalized at scan (\d+)", r.stdout)] == [lost_at]
    poses = np.loadtxt(str(out_dir / "poses.txt")).reshape(-1, 12)
    assert poses.shape[0] == len(scans)                       # one row per scan: the recovered scan's last processing
    assert np.allclose(poses, np.array([T_of(x["pose"]).reshape(12) for x in got]), rtol=2e-5, atol=2e-6)
    # the options need a map that is read
    r = subprocess.run(base[:-1] + ["map_hits=%s" % hits], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "localize=1" in r.stderr
    r = subprocess.run(base + ["relocalize_below=0.4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "map_hits" in r.stderr
