"""The NumPy model of branch-and-bound relocalisation (tests/reloc_bnb_model.py) against the NumPy model of the exhaustive score
(tests/reloc_model.py): the bound is admissible for every node of every level, and the driver returns the exhaustive ranking's best.
CPU only; the device is held equal to this model in test_gpu_reloc_bnb.py.

The three invariants: (a) bound >= hits_r + hits_0 of every child — test_bound_is_admissible_*; (b) the search result
equals the exhaustive one — test_driver_equals_the_exhaustive_search_*; (c) the model's and the kernel's counts are equal — the GPU
tests."""
import numpy as np
import pytest

import localize_model as lm
import reloc_bnb_model as bm
import reloc_model as rm

_CACHE = {}
SHAPES = [dict(nx=6, ny=3, nyaw=2), dict(nx=4, ny=7, nyaw=2)]      # 13 x 7 x 5 and 9 x 15 x 5: ragged against every tile size
STEPS = [0.15, 0.4, 1.0]
# designed map: the identity (every designed edge at its designed place: tiles straddle the cell faces in x and y), and a yawed
# centre at negative coordinates
DESIGNED_CENTRES = [np.array([0, 0, 0, 1, 0, 0, 0], np.float64), np.array([0, 0, np.sin(0.15), np.cos(0.15), -3.2, 1.7, 0.1])]


def _designed():
    if "designed" not in _CACHE:
        state = rm.state_from_points(rm.DESIGNED_MAP)
        _CACHE["designed"] = (rm.Occupancy(state), bm.BlockSets(state))
    return _CACHE["designed"]


def _site(orc, synth):
    if "site" not in _CACHE:
        state = rm.state_from_points(lm.site_map(orc, synth).all())
        _CACHE["site"] = (rm.Occupancy(state), bm.BlockSets(state))
    return _CACHE["site"]


def _all_nodes(wx, wy, slabs):
    K = 0
    while (1 << K) < max(wx, wy):
        K += 1
    return [(s, x0, y0, k) for k in range(K + 1) for s in range(slabs) for y0 in range(0, wy, 1 << k) for x0 in range(0, wx, 1 << k)]


def _check_admissible(occ, blocks, edges, centre, radius, **grid):
    T, _, _ = rm.candidate_grid(centre, **grid)
    wx, wy = 2 * grid.get("nx", 0) + 1, 2 * grid.get("ny", 0) + 1
    exact = occ.hits(edges, T, radius=radius).astype(np.int64).reshape(-1, wy, wx, 2)
    nodes = _all_nodes(wx, wy, exact.shape[0])
    T_lo, t_hi, _, _ = bm.node_extremes(T, wx, wy, nodes)
    levels = [bm.level_of(1 << k, grid["step_xy"], 0.4, radius) for _, _, _, k in nodes]
    ub = blocks.bound(edges, T_lo, t_hi, levels, radius).astype(np.int64)
    # a looser level is admissible as well (the public call takes any), and so is the tightest one: too fine a level escapes
    ub_up = blocks.bound(edges, T_lo, t_hi, [min(h + 2, bm.LEVEL_MAX) for h in levels], radius).astype(np.int64)
    ub_1 = blocks.bound(edges, T_lo, t_hi, 1, radius).astype(np.int64)
    for i, (s, x0, y0, k) in enumerate(nodes):
        tile = exact[s, y0:y0 + (1 << k), x0:x0 + (1 << k)]
        for u in (ub[i], ub_up[i], ub_1[i]):
            assert u[0] >= tile[..., 0].max() and u[1] >= tile[..., 1].max() and u[0] >= u[1], (nodes[i], u, tile.sum(axis=-1).max())
        if k == 0 and radius == 0:
            assert ub[i, 0] == ub[i, 1]
    return ub, exact


@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("step", STEPS)
def test_bound_is_admissible_on_the_designed_map(step, radius):
    occ, blocks = _designed()
    edges, want = rm.designed_edges()
    for centre in DESIGNED_CENTRES:
        for shape in SHAPES:
            ub, exact = _check_admissible(occ, blocks, edges, centre, radius, step_xy=step, step_yaw=0.05, **shape)
        _check_admissible(occ, blocks, edges, centre, radius, step_xy=step, step_yaw=0.05, step_z=0.4, nx=2, ny=2, nyaw=1, nz=1)
    # the identity is a candidate of the identity's grids: the designed counts
    T, _, idx = rm.candidate_grid(DESIGNED_CENTRES[0], step_xy=step, step_yaw=0.05, **SHAPES[1])
    at = int(np.nonzero((idx == 0).all(axis=1))[0][0])
    assert tuple(occ.hits(edges, T[at:at + 1], radius=radius)[0]) == want[radius]


@pytest.mark.parametrize("radius", [0, 1])
@pytest.mark.parametrize("step", STEPS)
def test_bound_is_admissible_on_the_site_map(orc, synth, step, radius):
    occ, blocks = _site(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[5]
    e = e[::3]                                             # 228 edges
    centre = gt.copy()
    centre[4:] += (0.7, -0.45, 0.0)
    for shape in SHAPES:
        ub, exact = _check_admissible(occ, blocks, e, centre, radius, step_xy=step, step_yaw=0.05, **shape)
    assert ub.sum(axis=1).min() < 2 * e.shape[0]      # the bound says something: not every node keeps every edge


def test_escapes_count_and_non_finite_edges_do_not():
    occ, blocks = _designed()
    I = np.eye(4)[:3].reshape(1, 12)
    t = I[:, [3, 7]]
    e = np.array([[np.nan, 1, 1, 1], [np.inf, 1, 1, 1], [1, -np.inf, 1, 1], [1, 1, np.nan, 1],       # never count
                  [2.0e6, 0.1, 0.1, 1], [0.1, -5.0e5, 0.1, 1], [0.1, 0.1, 3.0e38, 1],               # beyond the leaf limit: count in both
                  [200.1, 200.1, 1.1, 1],                                                           # in range, no block there
                  [30.1, 30.1, 1.1, 1]], np.float32)                                                # an occupied leaf
    for radius in (0, 1):
        assert blocks.bound(e, I, t, 3, radius).tolist() == [[4, 4]]
        for i, want in enumerate([0, 0, 0, 0, 1, 1, 1, 0, 1]):
            assert blocks.bound(e[i:i + 1], I, t, 3, radius).tolist() == [[want, want]], i
    # a node 100 m wide at level 1 (blocks of 2 leaves): more than three blocks, every finite edge counts
    assert blocks.bound(e, I, t + 100.0, 1, 1).tolist() == [[5, 5]]
    # map points beyond the limit are not inserted, and an edge there escapes
    state = rm.state_from_points(np.array([[4.5e5, 0.1, 0.1, 1], [1.1, 1.1, 1.1, 1]], np.float32))
    far = bm.BlockSets(state)
    assert far.leaves.tolist() == [[2, 2, 2]]
    assert far.bound(np.array([[4.5e5, 0.1, 0.1, 1]], np.float32), I, t, 2, 1).tolist() == [[1, 1]]


def test_level_of_a_node():
    assert bm.level_of(1, 0.4, 0.4, 0) == 1 and bm.level_of(1, 0.4, 0.4, 1) == 2
    assert bm.level_of(2, 0.4, 0.4, 1) == 3 and bm.level_of(256, 0.4, 0.4, 1) == 9 and bm.level_of(256, 0.4, 0.4, 0) == 9
    assert bm.level_of(256, 0.1, 0.4, 1) == 7 and bm.level_of(1 << 31, 1.0, 0.4, 1) == bm.LEVEL_MAX
    # the span of a node's probes, in leaves, fits 2^h with a leaf to spare at either end: at most three blocks
    for w in (1, 2, 3, 8, 200):
        for step in STEPS:
            for r in (0, 1):
                assert 2.0 ** bm.level_of(w, step, 0.4, r) >= (w - 1) * step / float(np.float32(0.4)) + 2 * r + 2


def _check_driver(occ, blocks, edges, centre, batches=(1, 64, bm.BATCH_DEFAULT), **grid):
    T, _, _ = rm.candidate_grid(centre, **grid)
    want = occ.hits(edges, T, radius=grid.get("radius", 1))
    for batch in batches:
        r = bm.search_grid(occ, blocks, edges, centre, batch=batch, **grid)
        assert r["best_index"] == rm.best_of(want) and (r["hits_r"], r["hits_0"]) == tuple(want[r["best_index"]]), (batch, grid)
        assert r["n_candidates"] == T.shape[0] and 1 <= r["candidates_scored"] <= T.shape[0] and r["rounds"] >= 1
    return r, want


@pytest.mark.parametrize("radius", [0, 1])
def test_driver_equals_the_exhaustive_search_on_the_designed_map(radius):
    occ, blocks = _designed()
    edges, _ = rm.designed_edges()
    for centre in DESIGNED_CENTRES:
        for step in STEPS:
            for shape in SHAPES:
                _check_driver(occ, blocks, edges, centre, step_xy=step, step_yaw=0.05, radius=radius, **shape)
        _check_driver(occ, blocks, edges, centre, step_xy=0.4, step_yaw=0.05, step_z=0.4, nx=2, ny=2, nyaw=1, nz=1, radius=radius)
        _check_driver(occ, blocks, edges, centre, radius=radius)                  # one candidate: the root is a leaf
        _check_driver(occ, blocks, edges, centre, nyaw=3, radius=radius)          # yaw only: seven roots, all leaves


@pytest.mark.parametrize("scan", [0, 5, 11])
def test_driver_equals_the_exhaustive_search_on_the_site_map(orc, synth, scan):
    occ, blocks = _site(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[scan]
    e = e[::3]
    centre = gt.copy()
    centre[4:] += (0.7, -0.45, 0.0)
    for radius in (0, 1):
        _check_driver(occ, blocks, e, centre, step_xy=0.4, step_yaw=0.05, nx=5, ny=5, nyaw=4, radius=radius)      # 11 x 11 x 9
    for step in STEPS:
        for shape in SHAPES:
            _check_driver(occ, blocks, e, centre, batches=(64,), step_xy=step, step_yaw=0.05, **shape)


def test_ties_go_to_the_lowest_index(orc, synth):
    occ, blocks = _site(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[0]
    away = gt.copy()
    away[4:] += (1000.0, -1000.0, 0.0)                     # no edge reaches the map: every score is 0
    for batch in (1, 64):
        r = bm.search_grid(occ, blocks, e, away, batch=batch, step_xy=0.4, step_yaw=0.05, nx=3, ny=2, nyaw=1)
        assert (r["best_index"], r["hits_r"], r["hits_0"]) == (0, 0, 0)
        assert batch > 1 or r["candidates_scored"] == 1    # one node a round: the first leaf scored 0 and nothing can beat index 0
    # no edges, no map: nothing is searched
    r = bm.search_grid(occ, blocks, np.zeros((0, 4), np.float32), gt, nx=2, nz=3)
    assert (r["best_index"], r["rounds"], r["n_candidates"]) == (0, 0, 35)
    # equal candidates with edges: a step too small to move a float coordinate
    r, want = _check_driver(occ, blocks, e, gt, batches=(4,), nx=2, step_xy=1e-12)
    assert len(np.unique(want, axis=0)) == 1 and want[0, 0] > 0 and r["best_index"] == 0


def test_the_measured_window_finds_the_truth(orc, synth):
    """21 x 21 x 51 = 22 491 candidates around a centre 2.0, -1.2 m off scan 5's truth: the truth is candidate
    (ix, iy, ia) = (-5, 3, 0) = index 11303, and its score is 1266."""
    occ, blocks = _site(orc, synth)
    _, e, gt = lm.traversal(orc, synth, 1)[5]
    centre = gt.copy()
    centre[4:] += (2.0, -1.2, 0.0)
    r = bm.search_grid(occ, blocks, e, centre, batch=256, step_xy=0.4, step_yaw=0.02, nx=10, ny=10, nyaw=25)
    print(r)
    assert r["n_candidates"] == 22491 and r["best_index"] == 11303 and r["hits_r"] + r["hits_0"] == 1266
    assert r["candidates_scored"] < 22491 // 20
