"""Branch-and-bound relocalisation on the device: liodom_map_bound_nodes (k_map_blocks_clear, k_map_blocks_build, k_map_bound_nodes)
and liodom_map_search_pose_bnb, Map.search_pose_bnb and Liodom.relocalize with a bnb level.  Every bound is compared for equality
with the NumPy model (tests/reloc_bnb_model.py) built from the same map's export_state(); every search result field for field with
liodom_map_search_pose on the same inputs, and its statistics with the model's driver.

Shapes.  k_map_bound_nodes gives a node one wave and a workgroup four contiguous nodes; a wave walks the edges in rounds of 64: the
boundaries are n = 3 | 4 | 5 and n_edges = 63 | 64 | 65.  The search switches nothing on size; its grids are ragged against every
tile size (13 x 7, 9 x 15), the measured window (21 x 21 x 51), the widest window the exhaustive call takes (129 x 129 x 51) and one
beyond it (201 x 201 x 157)."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import localize_model as lm
import reloc_bnb_model as bm
import reloc_model as rm
from mapper_lag_common import EPR, H, P, POSE_TOL_R, POSE_TOL_T, R, W, T_of, rot_angle

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)
SMALL = dict(max_cells=16, cell_capacity=256, max_update_points=1024, max_modified_cells=16)
SHAPES = [dict(nx=6, ny=3, nyaw=2), dict(nx=4, ny=7, nyaw=2)]      # 13 x 7 x 5 and 9 x 15 x 5
STEPS = [0.15, 0.4, 1.0]
DESIGNED_CENTRES = [np.array([0, 0, 0, 1, 0, 0, 0], np.float64), np.array([0, 0, np.sin(0.15), np.cos(0.15), -3.2, 1.7, 0.1])]
WINDOW = dict(step_xy=0.4, step_yaw=0.02, nx=10, ny=10, nyaw=25)      # 21 x 21 x 51 = 22 491
_SITE = {}


def _handle(**cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(n_streams=1, max_points=H * W, max_width=W, recv_capacity=1 << 16, **cfg))


def _site_map(orc, synth):
    if "blob" not in _SITE:
        m = la.Map(**CAPS)
        for e, T in lm.site_updates(orc, synth):
            m.update(e, T)
        assert m.num_cells() == 29 and m.status() == 0
        _SITE["blob"] = m.export_state()
        state = api.parse_map_state(_SITE["blob"])
        _SITE["model"] = (rm.Occupancy(state), bm.BlockSets(state))
        m.close()
    m = la.Map(**CAPS)
    m.import_state(_SITE["blob"])
    return m


def _models(m):
    state = api.parse_map_state(m.export_state())
    return rm.Occupancy(state), bm.BlockSets(state)


def _designed_map():
    m = la.Map(**SMALL)
    m.update(rm.DESIGNED_MAP)
    assert m.num_cells() == rm.DESIGNED_CELLS and m.status() == 0
    return m


def _all_nodes(wx, wy, slabs):
    K = 0
    while (1 << K) < max(wx, wy):
        K += 1
    return [(s, x0, y0, k) for k in range(K + 1) for s in range(slabs) for y0 in range(0, wy, 1 << k) for x0 in range(0, wx, 1 << k)]


def _grid_nodes(centre, radius, **grid):
    """Every node of every level of a grid: (T_lo, t_hi, the level of each)."""
    T, _, _ = rm.candidate_grid(centre, **grid)
    wx, wy = 2 * grid.get("nx", 0) + 1, 2 * grid.get("ny", 0) + 1
    nodes = _all_nodes(wx, wy, T.shape[0] // (wx * wy))
    T_lo, t_hi, _, _ = bm.node_extremes(T, wx, wy, nodes)
    return T_lo, t_hi, np.array([bm.level_of(1 << k, grid["step_xy"], 0.4, radius) for _, _, _, k in nodes])


def _check_bounds(m, blocks, edges, T_lo, t_hi, levels, radius):
    """The device's bounds of the nodes at their own levels, two levels up and at level 1, against the model's."""
    for lv in (levels, np.minimum(levels + 2, bm.LEVEL_MAX), np.ones_like(levels)):
        for h in np.unique(lv):
            at = np.nonzero(lv == h)[0]
            got = m.bound_nodes(edges, T_lo[at], t_hi[at], int(h), radius=radius)
            assert got.dtype == np.int32 and np.array_equal(got, blocks.bound(edges, T_lo[at], t_hi[at], int(h), radius)), (int(h), radius)


@pytest.mark.parametrize("radius", [0, 1])
def test_bounds_on_the_designed_map(radius):
    m = _designed_map()
    before = m.export_state()
    _, blocks = _models(m)
    edges, _ = rm.designed_edges()
    for centre in DESIGNED_CENTRES:       # tiles straddle the coarse-cell faces in x and y; the second centre lies at negative coordinates
        for step, shape in zip(STEPS, SHAPES + SHAPES[:1]):
            _check_bounds(m, blocks, edges, *_grid_nodes(centre, radius, step_xy=step, step_yaw=0.05, **shape), radius)
    # the identity node at level 2, edge by edge, so that a wrong case names itself: a one-candidate node at a fine level counts
    # what the exact score counts on this map, plus the escape (2.0e6 lies beyond the leaf limit: it counts, not knowing better)
    I = np.eye(4)[:3].reshape(1, 12)
    for i, (p, h0, hr) in enumerate(rm.DESIGNED_EDGES):
        got = tuple(m.bound_nodes(edges[i:i + 1], I, I[:, [3, 7]], 2, radius=radius)[0])
        assert got == tuple(blocks.bound(edges[i:i + 1], I, I[:, [3, 7]], 2, radius)[0]), (i, p)
        assert got[1] >= h0 and got[0] >= (hr if radius else h0) and (not np.isfinite(p).all() or p[0] < 1e6 or got == (1, 1)), (i, p, got)
    assert m.status() == 0 and m.export_state() == before
    m.close()


@pytest.mark.parametrize("radius", [0, 1])
def test_bounds_on_the_crafted_state(radius):
    blob, edges, want, _ = rm.crafted_state_blob()
    m = la.Map(**SMALL)
    m.import_state(blob)
    _, blocks = _models(m)
    I = np.eye(4)[:3].reshape(1, 12)
    for level in (1, 2, 3, 8, bm.LEVEL_MAX):
        got = m.bound_nodes(edges, I, I[:, [3, 7]], level, radius=radius)
        assert np.array_equal(got, blocks.bound(edges, I, I[:, [3, 7]], level, radius)) and got[0, 0] >= want[radius][0] and got[0, 1] >= want[radius][1]
    _check_bounds(m, blocks, edges, *_grid_nodes(DESIGNED_CENTRES[0], radius, step_xy=0.4, step_yaw=0.05, **SHAPES[0]), radius)
    m.close()


def test_escapes_count_and_non_finite_edges_do_not():
    m = _designed_map()
    _, blocks = _models(m)
    I = np.eye(4)[:3].reshape(1, 12)
    t = I[:, [3, 7]]
    e = np.array([[np.nan, 1, 1, 1], [np.inf, 1, 1, 1], [1, -np.inf, 1, 1], [1, 1, np.nan, 1],       # never count
                  [2.0e6, 0.1, 0.1, 1], [0.1, -5.0e5, 0.1, 1], [0.1, 0.1, 3.0e38, 1],               # beyond the leaf limit: count in both
                  [200.1, 200.1, 1.1, 1],                                                           # in range, no block there
                  [30.1, 30.1, 1.1, 1]], np.float32)                                                # an occupied leaf
    for radius in (0, 1):
        assert m.bound_nodes(e, I, t, 3, radius=radius).tolist() == blocks.bound(e, I, t, 3, radius).tolist() == [[4, 4]]
        for i, want in enumerate([0, 0, 0, 0, 1, 1, 1, 0, 1]):
            assert m.bound_nodes(e[i:i + 1], I, t, 3, radius=radius).tolist() == [[want, want]], i
    # a node 100 m wide at level 1: more than three blocks, every finite edge counts; non-finite extremes count as well
    assert m.bound_nodes(e, I, t + 100.0, 1).tolist() == blocks.bound(e, I, t + 100.0, 1, 1).tolist() == [[5, 5]]
    bad = np.array([[np.inf, 0.0], [np.nan, np.nan]])
    T2 = np.concatenate([I, I])
    assert m.bound_nodes(e, T2, bad, 3).tolist() == blocks.bound(e, T2, bad, 3, 1).tolist() == [[5, 5], [5, 5]]
    assert m.status() == 0
    m.close()


@pytest.mark.parametrize("n_edges", [0, 1, 63, 64, 65, 684])
def test_edge_counts(orc, synth, n_edges):
    m = _site_map(orc, synth)
    _, blocks = _SITE["model"]
    _, edges, gt = lm.traversal(orc, synth, 1)[0]
    assert edges.shape[0] == 684
    e = edges[:n_edges]
    for radius in (0, 1):
        T_lo, t_hi, levels = _grid_nodes(gt, radius, step_xy=0.4, step_yaw=0.05, nx=2, ny=1, nyaw=1)      # 5 x 3 x 3: 72 nodes
        _check_bounds(m, blocks, e, T_lo, t_hi, levels, radius)
        got = m.bound_nodes(e, T_lo[-3:], t_hi[-3:], int(levels[-1]), radius=radius)                        # the roots: the truth is in one
        assert n_edges < 63 or got.sum(axis=1).max() > n_edges
    m.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1025])
def test_node_counts(orc, synth, n):
    m = _site_map(orc, synth)
    _, blocks = _SITE["model"]
    _, edges, gt = lm.traversal(orc, synth, 1)[0]
    e = edges[::3]                                         # 228 edges
    T_lo, t_hi, levels = _grid_nodes(gt, 1, step_xy=0.4, step_yaw=0.03, nx=8, ny=8, nyaw=2)      # 17 x 17 x 5
    at = np.nonzero(levels == levels[0])[0]                # the leaves: 1445 nodes of one level
    at = at[np.linspace(0, at.shape[0] - 1, n).astype(int)]
    got = m.bound_nodes(e, T_lo[at], t_hi[at], int(levels[0]))
    assert got.shape == (n, 2) and np.array_equal(got, blocks.bound(e, T_lo[at], t_hi[at], int(levels[0]), 1))
    assert got[:, 0].max() > 0 and (n < 5 or len(np.unique(got[:, 0])) > 2)
    m.close()


def test_the_current_slab_after_a_second_update():
    m = _designed_map()
    edges, _ = rm.designed_edges()
    more = np.array([[10.1, 10.1, 10.1, 1], [50.1, 5.1, 5.1, 1], [39.9, 2.1, 1.15, 1]], np.float32)      # cells (20,20,25) and (60,20,25)
    e = np.concatenate([edges, more])
    I = np.eye(4)[:3].reshape(1, 12)
    first = m.bound_nodes(e, I, I[:, [3, 7]], 1, radius=0)
    m.update(more)
    assert m.num_cells() == rm.DESIGNED_CELLS and m.status() == 0
    _, blocks = _models(m)
    got = m.bound_nodes(e, I, I[:, [3, 7]], 1, radius=0)
    assert np.array_equal(got, blocks.bound(e, I, I[:, [3, 7]], 1, 0)) and got[0, 1] == first[0, 1] + 2      # two new blocks; one point joined an old one
    _check_bounds(m, blocks, e, *_grid_nodes(DESIGNED_CENTRES[1], 1, step_xy=0.4, step_yaw=0.05, **SHAPES[1]), 1)
    m.close()


def _same_as_exhaustive(m, e, centre, batches, models=None, **grid):
    want = m.search_pose(e, centre, **grid)
    for batch in batches:
        got = m.search_pose_bnb(e, centre, batch=batch, **grid)
        st = got.pop("stats")
        assert set(got) == set(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), (k, batch, grid, got[k], want[k])
        assert st["n_candidates"] == want["n_candidates"] and 1 <= st["candidates_scored"] <= want["n_candidates"] and st["rounds"] >= 1
        if models is not None:
            mod = bm.search_grid(models[0], models[1], e, centre, batch=batch or bm.BATCH_DEFAULT, **grid)
            assert (mod["best_index"], mod["hits_r"], mod["hits_0"]) == (got["best_index"], got["hits_r"], got["hits_0"])
            assert st == {k: mod[k] for k in st}, (batch, grid, st, mod)
    return want, st


@pytest.mark.parametrize("radius", [0, 1])
def test_search_equals_the_exhaustive_one_on_the_designed_map(radius):
    m = _designed_map()
    models = _models(m)
    edges, _ = rm.designed_edges()
    for centre in DESIGNED_CENTRES:
        for step, shape in zip(STEPS, SHAPES + SHAPES[:1]):
            _same_as_exhaustive(m, edges, centre, (1, 64, 0), models, step_xy=step, step_yaw=0.05, radius=radius, **shape)
        _same_as_exhaustive(m, edges, centre, (1, 0), models, step_xy=0.4, step_yaw=0.05, step_z=0.4, nx=2, ny=2, nyaw=1, nz=1, radius=radius)
        _same_as_exhaustive(m, edges, centre, (1, 0), models, radius=radius)                 # one candidate
        _same_as_exhaustive(m, edges, centre, (1, 3, 0), models, nyaw=3, radius=radius)      # yaw only: seven roots, all leaves
    m.close()


@pytest.mark.parametrize("scan", [0, 5, 11])
def test_search_equals_the_exhaustive_one_on_small_site_grids(orc, synth, scan):
    m = _site_map(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[scan]
    e = e[::3]
    centre = gt.copy()
    centre[4:] += (0.7, -0.45, 0.0)
    for radius, batches in ((0, (64,)), (1, (1, 0))):
        _same_as_exhaustive(m, e, centre, batches, _SITE["model"], step_xy=0.4, step_yaw=0.05, nx=5, ny=5, nyaw=4, radius=radius)      # 11 x 11 x 9
    for step, shape in zip(STEPS, SHAPES + SHAPES[:1]):
        _same_as_exhaustive(m, e, centre, (64,), _SITE["model"], step_xy=step, step_yaw=0.05, **shape)
    m.close()


@pytest.mark.parametrize("radius", [0, 1])
def test_search_equals_the_exhaustive_one_on_the_measured_window(orc, synth, radius):
    m = _site_map(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[5]
    centre = gt.copy()
    centre[4:] += (2.0, -1.2, 0.0)
    want, st = _same_as_exhaustive(m, e, centre, (1, 64, 0), radius=radius, **WINDOW)
    print("21 x 21 x 51, radius %d, default batch: %s" % (radius, st))
    assert want["n_candidates"] == 22491 and (radius == 0 or (want["best_index"], want["hits_r"] + want["hits_0"]) == (11303, 1266))
    assert st["candidates_scored"] < 22491 // 10
    m.close()


@pytest.mark.parametrize("radius", [0, 1])
def test_search_equals_the_exhaustive_one_on_its_widest_window(orc, synth, radius):
    """129 x 129 x 51 = 848 691 candidates: the widest window liodom_map_search_pose accepts, 10.0, -7.6 m off the truth."""
    m = _site_map(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[5]
    centre = gt.copy()
    centre[4:] += (10.0, -7.6, 0.0)
    want, st = _same_as_exhaustive(m, e, centre, (1, 64, 0), radius=radius, step_xy=0.4, step_yaw=0.02, nx=64, ny=64, nyaw=25)
    print("129 x 129 x 51, radius %d, default batch: %s" % (radius, st))
    assert want["n_candidates"] == 848691
    if radius:      # the truth is candidate (ix, iy, ia) = (-25, 19, 0)
        assert want["best_index"] == (25 * 129 + 19 + 64) * 129 - 25 + 64 and want["hits_r"] + want["hits_0"] == 1266
    m.close()


def test_beyond_the_exhaustive_limit(orc, synth):
    """201 x 201 x 157 = 6 342 957 candidates, +-40 m and +-1.56 rad, around a centre 10.0, -7.6 m off scan 5's truth: the truth is
    candidate (ix, iy, ia) = (-25, 19, 0) = index 3175272 and scores 1266 (the CPU model found the same)."""
    m = _site_map(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[5]
    centre = gt.copy()
    centre[4:] += (10.0, -7.6, 0.0)
    grid = dict(step_xy=0.4, step_yaw=0.02, nx=100, ny=100, nyaw=78)
    with pytest.raises(la.LiodomError):
        m.search_pose(e, centre, **grid)
    for batch in (256, 0):
        r = m.search_pose_bnb(e, centre, batch=batch, **grid)
        print("201 x 201 x 157, batch %d: %s" % (batch, r["stats"]))
        assert r["n_candidates"] == r["stats"]["n_candidates"] == 6342957 and r["best_index"] == 3175272 and r["hits_r"] + r["hits_0"] == 1266
        assert np.abs(r["pose"] - lm.normalised(gt)).max() <= 1e-12 and np.abs(r["T"] - T_of(gt)).max() <= 1e-12
        assert tuple(m.score_poses(e, r["T"].reshape(1, 12))[0]) == (r["hits_r"], r["hits_0"])
        assert r["stats"]["candidates_scored"] < 10000 and r["stats"]["levels_built"] >= 4
    assert m.status() == 0 and m.export_state() == _SITE["blob"]
    m.close()


def test_no_edges_and_no_map(orc, synth):
    m = _site_map(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[0]
    want = m.search_pose(np.zeros((0, 4), np.float32), gt, nz=3, step_z=0.4, nx=2)
    got = m.search_pose_bnb(np.zeros((0, 4), np.float32), gt, nz=3, step_z=0.4, nx=2)
    assert got.pop("stats") == dict(n_candidates=35, nodes_bounded=0, candidates_scored=0, rounds=0, levels_built=0)
    assert all(np.array_equal(got[k], want[k]) for k in want) and got["best_index"] == 0
    # equal candidates with edges: a step too small to move a float coordinate
    _same_as_exhaustive(m, e, gt, (1, 0), nx=2, step_xy=1e-12)
    m.reset()
    want, got = m.search_pose(e, gt, **WINDOW), m.search_pose_bnb(e, gt, **WINDOW)
    assert got.pop("stats")["rounds"] == 0 and all(np.array_equal(got[k], want[k]) for k in want) and (got["best_index"], got["hits_r"]) == (0, 0)
    m.close()


def test_searching_is_read_only_also_between_a_readers_steps(orc, synth):
    tr = lm.traversal(orc, synth, 1)[:4]

    def run(search):
        g, m = _handle(), _site_map(orc, synth)
        g.attach_map_reader(m, *lm.CELLS)
        poses = []
        for k, (x, e, gt) in enumerate(tr):
            poses.append(g.process_scan(x, H, W)[0].copy())
            if search:
                centre = gt.copy()
                centre[4:] += (2.0, -1.2, 0.0)
                r = m.search_pose_bnb(e, centre, **WINDOW)
                assert r["best_index"] == m.search_pose(e, centre, **WINDOW)["best_index"], k
                I = np.eye(4)[:3].reshape(1, 12)
                m.bound_nodes(e, I, I[:, [3, 7]], 4)
        assert m.export_state() == _SITE["blob"] and m.status() == 0
        g.attach_mapper(None)
        g.close(); m.close()
        return np.array(poses)

    assert np.array_equal(run(True), run(False))


def test_relocalize_over_forty_metres(orc, synth):
    x, e, gt = lm.traversal(orc, synth, 1)[0]
    off = np.array([0.0, 0.0, np.sin(0.185), np.cos(0.185)])      # 0.37 rad about the world z axis
    centre = np.concatenate([lm.quat_mul(off, gt[:4]), gt[4:] + np.array([31.1, -22.3, 0.0])])
    levels = [dict(bnb=True, step_xy=0.4, step_yaw=0.02, nx=100, ny=100, nyaw=25), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]
    m = _site_map(orc, synth)
    g = _handle()
    g.attach_map_reader(m, *lm.CELLS)
    g.seed_stream(gt)
    want, _ = g.process_scan(x, H, W)
    g.reset_stream(0)
    r = g.relocalize(m, x, H, W, centre, levels, min_fraction=0.5)
    assert r is not None and [lv["n_candidates"] for lv in r["levels"]] == [201 * 201 * 51, 729] and r["n_edges"] == e.shape[0]
    assert "stats" in r["levels"][0] and "stats" not in r["levels"][1]
    print("coarse %s %s fine %s, fraction %.3f" % (r["levels"][0]["stats"], r["levels"][0]["pose"] - lm.normalised(gt), r["levels"][1]["pose"] - lm.normalised(gt), r["fraction"]))
    assert np.linalg.norm(r["pose"][4:] - gt[4:]) <= 0.15 and rot_angle(r["pose"][:4], gt[:4]) <= 0.011
    assert np.abs(api.parse_stream_state(g.export_stream_state(0))["param_t"] - r["pose"][4:]).max() == 0.0      # seeded
    got, info = g.process_scan(x, H, W)
    assert info.scan_index == 0 and info.status == 0
    assert np.linalg.norm(got[4:] - want[4:]) <= POSE_TOL_T and rot_angle(got[:4], want[:4]) <= POSE_TOL_R
    assert m.status() == 0 and m.export_state() == _SITE["blob"]
    g.attach_mapper(None)
    g.close(); m.close()


def test_invalid_arguments_change_nothing(orc, synth):
    m = _site_map(orc, synth)
    L = m._L
    _, e, gt = lm.traversal(orc, synth, 1)[0]
    e = np.ascontiguousarray(e, np.float32)
    fp, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), \
        (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    bad = api.ERR_INVALID_ARG
    T = np.ascontiguousarray(np.tile(T_of(gt).reshape(1, 12), (3, 1)))
    t = np.ascontiguousarray(T[:, [3, 7]])
    ub = np.full((3, 2), -7, np.int32)
    for args in ((None, fp(e), 684, dp(T), dp(t), 3, 2, 1, ip(ub)), (m.h, None, 684, dp(T), dp(t), 3, 2, 1, ip(ub)), (m.h, fp(e), 684, None, dp(t), 3, 2, 1, ip(ub)),
                 (m.h, fp(e), 684, dp(T), None, 3, 2, 1, ip(ub)), (m.h, fp(e), 684, dp(T), dp(t), 3, 2, 1, None), (m.h, fp(e), -1, dp(T), dp(t), 3, 2, 1, ip(ub)),
                 (m.h, fp(e), 684, dp(T), dp(t), -1, 2, 1, ip(ub)), (m.h, fp(e), 684, dp(T), dp(t), (1 << 20) + 1, 2, 1, ip(ub)),
                 (m.h, fp(e), 684, dp(T), dp(t), 3, 0, 1, ip(ub)), (m.h, fp(e), 684, dp(T), dp(t), 3, 22, 1, ip(ub)), (m.h, fp(e), 684, dp(T), dp(t), 3, 2, 2, ip(ub)),
                 (m.h, fp(e), m.max_update_points + 1, dp(T), dp(t), 3, 2, 1, ip(ub))):
        assert L.liodom_map_bound_nodes(*args) == bad
    assert b"liodom_map_bound_nodes" in L.liodom_last_error()
    assert L.liodom_map_bound_nodes(m.h, None, 0, None, None, 0, 2, 1, None) == 0          # nothing to do is no error
    assert (ub == -7).all()
    res, st, opt = api.PoseSearchResult(), api.PoseSearchStats(), api.PoseSearchBnb()
    res.best_index = st.rounds = -7

    def search(**kw):
        return api.make_pose_search(kw.pop("centre", gt), **kw)

    def call(mh, edges, n, s, o, r, stats=C.byref(st)):
        return L.liodom_map_search_pose_bnb(mh, edges, n, s, o, r, stats)

    assert call(m.h, fp(e), 684, None, None, C.byref(res)) == bad
    assert call(m.h, fp(e), 684, C.byref(search()), None, None) == bad
    assert call(None, fp(e), 684, C.byref(search()), None, C.byref(res)) == bad
    assert call(m.h, None, 684, C.byref(search()), None, C.byref(res)) == bad
    assert call(m.h, fp(e), -1, C.byref(search()), None, C.byref(res)) == bad
    for batch in (-1, 65537):
        opt.batch = batch
        assert call(m.h, fp(e), 684, C.byref(search(nx=2)), C.byref(opt), C.byref(res)) == bad
    # the exhaustive call's error for too many edges
    rc = L.liodom_map_search_pose(m.h, fp(e), m.max_update_points + 1, C.byref(search()), C.byref(res), None, None)
    assert call(m.h, fp(e), m.max_update_points + 1, C.byref(search()), None, C.byref(res)) == rc == bad
    nan_c, long_q = gt.copy(), gt.copy()
    nan_c[5] = np.nan
    long_q[:4] *= 1.001
    for s in (search(radius=2), search(nx=-1), search(nx=1, step_xy=0.0), search(nz=1, step_z=-0.4), search(nyaw=1, step_yaw=float("nan")),
              search(centre=nan_c), search(centre=long_q), search(nx=1 << 30), search(nx=1000, ny=1000, nyaw=300), search(nx=32768, ny=32768)):
        assert call(m.h, fp(e), 684, C.byref(s), None, C.byref(res)) == bad
        assert b"liodom_map_search_pose_bnb" in L.liodom_last_error()
    assert res.best_index == -7 and st.rounds == -7
    assert m.status() == 0 and m.export_state() == _SITE["blob"]
    # and the map still searches, with and without the optional arguments
    opt.batch = 0
    assert call(m.h, fp(e), 684, C.byref(search(nx=2, ny=2)), C.byref(opt), C.byref(res), None) == 0 and res.n_candidates == 25
    assert call(m.h, fp(e), 684, C.byref(search(nx=2, ny=2)), None, C.byref(res)) == 0 and st.n_candidates == 25 and st.rounds >= 1
    m.close()
