"""Relocalising in a saved map on the device: liodom_map_score_poses / liodom_map_search_pose (k_map_occ_clear, k_map_occ_build,
k_map_score_poses, k_map_score_best) and Liodom.relocalize.  Every count is compared for equality with the NumPy model
(tests/reloc_model.py) built from the same map's export_state().

Shapes.  k_map_score_poses gives a candidate one wave and a workgroup four contiguous candidates; a wave walks the edges in rounds
of 64.  There is no grid chunking (the grid is ceil(n / 4) workgroups up to the 2^20 limit) and no 256-edge staging, so the
boundaries are n = 3 | 4 | 5 (a partial workgroup, a full one, one wave of a second) and n_edges = 63 | 64 | 65; 1025 candidates
keep many workgroups plus a single wave, and 255 | 256 | 257 edges stay in the list although nothing switches there."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import localize_model as lm
import reloc_model as rm
from mapper_lag_common import EPR, H, P, POSE_TOL_R, POSE_TOL_T, R, W, T_of, rot_angle

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)
SMALL = dict(max_cells=16, cell_capacity=256, max_update_points=1024, max_modified_cells=16)
GRID = dict(step_xy=0.4, step_yaw=0.05, nx=5, ny=5, nyaw=4)      # 1089 candidates, the centre at index 544
_SITE = {}


def _handle(**cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(n_streams=1, max_points=H * W, max_width=W, recv_capacity=1 << 16, **cfg))


def _site_map(orc, synth, **caps):
    if "blob" not in _SITE:
        m = la.Map(**CAPS)
        for e, T in lm.site_updates(orc, synth):
            m.update(e, T)
        assert m.num_cells() == 29 and m.status() == 0
        _SITE["blob"] = m.export_state()
        m.close()
    m = la.Map(**(caps or CAPS))
    m.import_state(_SITE["blob"])
    return m


def _site_model(orc, synth):
    if "model" not in _SITE:
        _site_map(orc, synth).close()
        _SITE["model"] = rm.Occupancy(api.parse_map_state(_SITE["blob"]))
    return _SITE["model"]


def _model(m):
    return rm.Occupancy(api.parse_map_state(m.export_state()))


def _site_candidates(orc, synth, n, scan=0):
    """n candidates around the scan's ground truth: a yaw grid, every third one tilted by a roll and a pitch as well."""
    gt = lm.traversal(orc, synth, 1)[scan][2]
    T, _, _ = rm.candidate_grid(gt, step_xy=0.4, step_yaw=0.03, nx=8, ny=8, nyaw=2)      # 1445
    T = T[np.linspace(0, T.shape[0] - 1, n).astype(int)].reshape(-1, 3, 4).copy()
    tilt = rm.rot_of_quat([0.02, -0.015, 0.0, 1.0])
    for i in range(0, n, 3):
        T[i, :, :3] = tilt @ T[i, :, :3]
    T[0] = T_of(gt)
    return T.reshape(-1, 12)


def _designed_map():
    m = la.Map(**SMALL)
    m.update(rm.DESIGNED_MAP)
    assert m.num_cells() == rm.DESIGNED_CELLS and m.status() == 0
    return m


@pytest.mark.parametrize("radius", [0, 1])
def test_designed_map(radius):
    m = _designed_map()
    before = m.export_state()
    edges, want = rm.designed_edges()
    T = rm.designed_candidates()
    got = m.score_poses(edges, T, radius=radius)
    assert got.dtype == np.int32 and got.shape == (4, 2)
    assert tuple(got[0]) == want[radius] and tuple(got[1]) == (0, 0)
    assert np.array_equal(got, _model(m).hits(edges, T, radius=radius))
    for i, (p, h0, hr) in enumerate(rm.DESIGNED_EDGES):      # edge by edge, so that a wrong case names itself
        assert tuple(m.score_poses(edges[i:i + 1], T[:1], radius=radius)[0]) == ((hr if radius else h0), h0), (i, p)
    # misses raise nothing (the key beyond +-2^20, NaN, inf, the leaf outside a grid), and nothing of the map has changed
    assert m.status() == 0 and m.export_state() == before
    m.close()


@pytest.mark.parametrize("radius", [0, 1])
def test_first_and_last_word_of_a_cells_bitmap(radius):
    blob, edges, want, _ = rm.crafted_state_blob()
    m = la.Map(**SMALL)
    m.import_state(blob)
    T = np.eye(4)[:3].reshape(1, 12)
    got = m.score_poses(edges, T, radius=radius)
    assert tuple(got[0]) == want[radius] and np.array_equal(got, _model(m).hits(edges, T, radius=radius))
    m.close()


@pytest.mark.parametrize("n_edges", [0, 1, 63, 64, 65, 255, 256, 257, 684])
def test_edge_counts(orc, synth, n_edges):
    m, occ = _site_map(orc, synth), _site_model(orc, synth)
    edges = lm.traversal(orc, synth, 1)[0][1]
    assert edges.shape[0] == 684
    e = edges[:n_edges]
    T = _site_candidates(orc, synth, 9)
    for radius in (0, 1):
        got = m.score_poses(e, T, radius=radius)
        assert np.array_equal(got, occ.hits(e, T, radius=radius)), (n_edges, radius)
        assert n_edges < 63 or got[0, 0] > n_edges // 2      # the truth is among them, and it hits
    m.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1025])
def test_candidate_counts(orc, synth, n):
    m, occ = _site_map(orc, synth), _site_model(orc, synth)
    e = lm.traversal(orc, synth, 1)[0][1][::3]      # 228 edges
    T = _site_candidates(orc, synth, n)
    got = m.score_poses(e, T, radius=1)
    assert got.shape == (n, 2) and np.array_equal(got, occ.hits(e, T, radius=1))
    assert got[:, 0].max() > 0 and (n < 5 or len(np.unique(got[:, 0])) > 2)
    m.close()


def test_the_current_slab_after_a_second_update():
    """The second update touches two of the five cells: their clouds move to the other slab (cell_buf flips), the others stay where
    they are.  The occupancy follows map_cell_cur in both kinds."""
    m = _designed_map()
    edges, _ = rm.designed_edges()
    more = np.array([[10.1, 10.1, 10.1, 1], [50.1, 5.1, 5.1, 1], [39.9, 2.1, 1.15, 1]], np.float32)      # cells (20,20,25) and (60,20,25)
    e = np.concatenate([edges, more])
    T = rm.designed_candidates()
    first = m.score_poses(e, T)
    m.update(more)
    assert m.num_cells() == rm.DESIGNED_CELLS and m.status() == 0
    got = m.score_poses(e, T)
    assert np.array_equal(got, _model(m).hits(e, T)) and got[0, 1] == first[0, 1] + 2      # (39.9, 2.1, 1.15) joined an occupied leaf
    m.close()


def test_occupancy_is_rebuilt_by_every_call(orc, synth):
    m = _site_map(orc, synth)
    tr = lm.traversal(orc, synth, 1)
    e, gt = tr[0][1], tr[0][2]
    T = _site_candidates(orc, synth, 6)

    def check(what):
        got = m.score_poses(e, T)
        assert np.array_equal(got, _model(m).hits(e, T)), what
        return got

    seen = [check("import")]
    m.update(tr[3][1], T_of(tr[3][2]))                          # more points: new leaves
    seen.append(check("update"))
    assert m.prune(T_of(gt), 0, 0) > 0                          # cells go, the survivors are renumbered
    seen.append(check("prune"))
    m.import_state(_SITE["blob"])
    seen.append(check("import_state"))
    blob, n = m.evict(T_of(gt), 0, 0)
    assert n > 0
    seen.append(check("evict"))
    assert m.merge_state(blob).sum() == n                       # ... and come back under other ids
    seen.append(check("merge_state"))
    assert np.array_equal(seen[5], seen[3]) and not np.array_equal(seen[4], seen[3]) and not np.array_equal(seen[1], seen[0])
    m.reset()
    assert not m.score_poses(e, T).any()
    m.update(tr[0][1], T_of(gt))                                # fewer cells than the occupancy has rows for
    check("update after reset")
    assert m.status() == 0
    m.close()


def test_scoring_is_read_only_also_between_a_readers_steps(orc, synth):
    tr = lm.traversal(orc, synth, 1)[:4]
    T = _site_candidates(orc, synth, 7)
    detached = _site_map(orc, synth)
    want = [detached.score_poses(e, T) for _, e, _ in tr]
    before = detached.export_state()
    assert detached.status() == 0
    detached.close()

    occ = _site_model(orc, synth)

    def run(score):
        g, m = _handle(), _site_map(orc, synth)
        g.attach_map_reader(m, *lm.CELLS)
        poses = []
        for k, (x, e, _) in enumerate(tr):
            poses.append(g.process_scan(x, H, W)[0].copy())
            if score:
                assert np.array_equal(m.score_poses(e, T), want[k]), k
                r = m.search_pose(e, tr[k][2], want_T=True, nx=1, ny=1, nyaw=1)
                assert r["n_candidates"] == 27 and r["best_index"] == rm.best_of(occ.hits(e, r["T_all"]))
        assert m.export_state() == before and m.status() == 0
        g.attach_mapper(None)
        g.close(); m.close()
        return np.array(poses)

    assert np.array_equal(run(True), run(False))


def test_site_map_search_around_the_truth(orc, synth):
    m, occ = _site_map(orc, synth), _site_model(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[0]
    r = m.search_pose(e, gt, want_T=True, want_hits=True, **GRID)
    Tm, poses, _ = rm.candidate_grid(gt, **GRID)
    assert r["n_candidates"] == 1089 and r["T_all"].shape == (1089, 3, 4)
    assert np.abs(r["T_all"].reshape(-1, 12) - Tm).max() <= 1e-12
    want = occ.hits(e, r["T_all"], radius=1)                    # the model on the matrices the device scored
    assert np.array_equal(r["hits"], want)
    assert np.array_equal(r["hits"], m.score_poses(e, r["T_all"], radius=1))
    assert r["best_index"] == rm.best_of(want) == 544
    assert (r["hits_r"], r["hits_0"]) == tuple(want[544]) and want[544, 0] + want[544, 1] == 1234
    assert np.array_equal(r["T"], r["T_all"][544]) and np.abs(r["pose"] - lm.normalised(gt)).max() <= 1e-15
    assert np.abs(r["pose"] - poses[544]).max() <= 1e-12
    m.close()


@pytest.mark.parametrize("scan", [5, 11])
def test_site_map_small_grids(orc, synth, scan):
    m, occ = _site_map(orc, synth), _site_model(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[scan]
    for radius in (0, 1):
        r = m.search_pose(e, gt, want_T=True, want_hits=True, step_xy=0.4, step_yaw=0.05, nx=2, ny=2, nyaw=1, radius=radius)
        want = occ.hits(e, r["T_all"], radius=radius)
        assert r["n_candidates"] == 75 and np.array_equal(r["hits"], want)
        assert r["best_index"] == rm.best_of(want) and (r["hits_r"], r["hits_0"]) == tuple(want[r["best_index"]])
        assert radius == 0 or r["best_index"] == 37
    m.close()


def test_ties_go_to_the_lowest_index(orc, synth):
    m = _site_map(orc, synth)
    gt = lm.traversal(orc, synth, 1)[0][2]
    r = m.search_pose(np.zeros((0, 4), np.float32), gt, want_hits=True, nz=3, step_z=0.4, nx=2)
    assert r["n_candidates"] == 35 and not r["hits"].any()
    assert (r["best_index"], r["hits_r"], r["hits_0"]) == (0, 0, 0)
    assert np.array_equal(r["pose"][4:], gt[4:] + np.array([-0.8, 0.0, -3 * 0.4]))
    # equal candidates with edges: every ix of a grid that only steps in x by a step too small to move a float coordinate
    e = lm.traversal(orc, synth, 1)[0][1]
    r = m.search_pose(e, gt, want_hits=True, nx=2, step_xy=1e-12)
    assert len(np.unique(r["hits"], axis=0)) == 1 and r["hits"][0, 0] > 0 and r["best_index"] == 0
    m.close()


LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=10, ny=10, nyaw=25), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]


def test_relocalize_seeds_the_stream(orc, synth):
    x, e, gt = lm.traversal(orc, synth, 1)[0]
    off = np.array([0.0, 0.0, np.sin(0.185), np.cos(0.185)])      # 0.37 rad about the world z axis
    centre = np.concatenate([lm.quat_mul(off, gt[:4]), gt[4:] + np.array([3.1, -2.3, 0.0])])
    m = _site_map(orc, synth)
    # the same scan after seed_stream(truth)
    g = _handle()
    g.attach_map_reader(m, *lm.CELLS)
    g.seed_stream(gt)
    want, _ = g.process_scan(x, H, W)
    g.reset_stream(0)
    state = g.export_stream_state(0)
    assert g.relocalize(m, x, H, W, centre, LEVELS, min_fraction=1.1) is None      # no fraction reaches 1.1
    assert g.export_stream_state(0) == state
    r = g.relocalize(m, x, H, W, centre, LEVELS, min_fraction=0.5)
    assert r is not None and [lv["n_candidates"] for lv in r["levels"]] == [22491, 729] and r["n_edges"] == e.shape[0]
    print("coarse %s fine %s, fraction %.3f" % (r["levels"][0]["pose"] - lm.normalised(gt), r["levels"][1]["pose"] - lm.normalised(gt), r["fraction"]))
    assert np.linalg.norm(r["pose"][4:] - gt[4:]) <= 0.15 and rot_angle(r["pose"][:4], gt[:4]) <= 0.011
    assert np.abs(api.parse_stream_state(g.export_stream_state(0))["param_t"] - r["pose"][4:]).max() == 0.0      # seeded
    got, info = g.process_scan(x, H, W)
    assert info.scan_index == 0 and info.status == 0
    print("dt %.3e dr %.3e" % (np.linalg.norm(got[4:] - want[4:]), rot_angle(got[:4], want[:4])))
    assert np.linalg.norm(got[4:] - want[4:]) <= POSE_TOL_T and rot_angle(got[:4], want[:4]) <= POSE_TOL_R
    assert m.status() == 0 and m.export_state() == _SITE["blob"]
    g.attach_mapper(None)
    g.close(); m.close()


def test_invalid_arguments_change_nothing(orc, synth):
    m = _site_map(orc, synth)
    L = m._L
    _, e, gt = lm.traversal(orc, synth, 1)[0]
    e = np.ascontiguousarray(e, np.float32)
    T = np.ascontiguousarray(_site_candidates(orc, synth, 3))
    fp, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    hits = np.full((3, 2), -7, np.int32)
    bad = api.ERR_INVALID_ARG
    assert L.liodom_map_score_poses(None, fp(e), 684, dp(T), 3, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, None, 684, dp(T), 3, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, None, 3, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, dp(T), 3, 1, None) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), -1, dp(T), 3, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, dp(T), -1, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, dp(T), 3, 2, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, dp(T), 3, -1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), m.max_update_points + 1, dp(T), 3, 1, ip(hits)) == bad
    assert L.liodom_map_score_poses(m.h, fp(e), 684, dp(T), (1 << 20) + 1, 1, ip(hits)) == bad
    assert b"liodom_map_score_poses" in L.liodom_last_error()
    assert L.liodom_map_score_poses(m.h, None, 0, None, 0, 1, None) == 0          # nothing to do is no error
    assert (hits == -7).all()
    res = api.PoseSearchResult()
    res.best_index = -7

    def search(**kw):
        return api.make_pose_search(kw.pop("centre", gt), **kw)

    assert L.liodom_map_search_pose(m.h, fp(e), 684, None, C.byref(res), None, None) == bad
    assert L.liodom_map_search_pose(m.h, fp(e), 684, C.byref(search()), None, None, None) == bad
    assert L.liodom_map_search_pose(None, fp(e), 684, C.byref(search()), C.byref(res), None, None) == bad
    assert L.liodom_map_search_pose(m.h, None, 684, C.byref(search()), C.byref(res), None, None) == bad
    nan_c, long_q = gt.copy(), gt.copy()
    nan_c[5] = np.nan
    long_q[:4] *= 1.001
    for s in (search(radius=2), search(nx=-1), search(nx=1, step_xy=0.0), search(nz=1, step_z=-0.4), search(nyaw=1, step_yaw=float("nan")),
              search(centre=nan_c), search(centre=long_q), search(nx=1 << 19), search(nx=60, ny=60, nyaw=80)):
        assert L.liodom_map_search_pose(m.h, fp(e), 684, C.byref(s), C.byref(res), None, None) == bad
        assert b"liodom_map_search_pose" in L.liodom_last_error()
    assert res.best_index == -7
    assert m.status() == 0 and m.export_state() == _SITE["blob"]
    # and the map still scores
    assert np.array_equal(m.score_poses(e, T), _site_model(orc, synth).hits(e, T))
    m.close()
