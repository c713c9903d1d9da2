"""Covariances of the pose graph and the loop gate on the GPU (liodom_graph_solve_columns / _covariance / _gate_edges; the kernels
in kernels_graph.h) against tests/graph_cov_model.py, on its designed graphs: chains of 2, 5, 64, 65 nodes, rings of 1024,
1025 and 1030 (a thread of the solving workgroup first owns two nodes at 1025), a ring of 12 with two loops, a hub of degree 40,
two components of which one has no fixed node, and a ring with Geman-McClure weights and a switched-off edge.  The bounds are the
model's (drift_allowance, block_bound, gate_bound) — none is taken from what the library returns.  The model of a graph is made
once and shared; the largest graph has 1030 nodes and at most 5 distinct query nodes: 30 workgroups."""
import numpy as np
import pytest

import graph_cov_model as gc
import graph_model as gm

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in gc.designed()}
_MODEL, _GRAPH = {}, {}


def _model(name):
    if name not in _MODEL:
        c = CASES[name]
        _MODEL[name] = gc.system(gc.lin_of(c), c["fixed"], c["edges"], c["active"])
    return _MODEL[name]


def _make(c, edges=None):
    import liodom_amd as la
    edges = c["edges"] if edges is None else edges
    g = la.PoseGraph(max_nodes=len(c["fixed"]) + 7, max_edges=len(edges) + 5)          # (capacities that are not the counts)
    g.add_nodes(c["poses"], c["fixed"])
    g.add_edges(edges)
    for kind, (name, scale) in (c["table"] or {}).items():
        g.set_loss(kind, name, scale)
    if c["active"] is not None:
        g.set_edge_active(0, c["active"])
    return g


def _graph(name):
    if name not in _GRAPH:
        _GRAPH[name] = _make(CASES[name])
    return _GRAPH[name]


def _opt(c, **more):
    return dict(max_pcg_iterations=c["max_pcg_iterations"], pcg_tolerance=c["pcg_tolerance"], **more)


@pytest.mark.parametrize("name", list(CASES))
def test_the_solve_is_a_solve(name):
    """|e_c - H x|_2 <= pcg_tolerance + d, H the model's dense matrix, d the drift allowance at the iterations the column reports."""
    c, s, g = CASES[name], _model(name), _graph(name)
    x, st = g.solve_columns(c["query"], **_opt(c))
    N = len(c["fixed"])
    assert x.shape == (len(c["query"]), 6, N, 6)
    worst = 0.0
    for k, q in enumerate(c["query"]):
        for b in range(6):
            if s["fixed"][q]:
                assert st["status"][k, b] == gc.OK and st["iterations"][k, b] == 0 and not x[k, b].any()
                continue
            if not s["anchored"][q]:
                assert st["status"][k, b] == gc.UNANCHORED and np.isnan(x[k, b]).all()
                continue
            assert st["status"][k, b] == gc.OK, (q, b, st[k, b])
            assert 1 <= st["iterations"][k, b] <= c["max_pcg_iterations"] and st["residual"][k, b] <= c["pcg_tolerance"]
            rhs = np.zeros(6 * N)
            rhs[6 * q + b] = 1.0
            res = float(np.linalg.norm(rhs - s["full"] @ x[k, b].reshape(-1)))
            d = gc.drift_allowance(s, int(st["iterations"][k, b]), float(np.linalg.norm(x[k, b])))
            worst = max(worst, res / (c["pcg_tolerance"] + d))
            assert res <= c["pcg_tolerance"] + d, (q, b, res, d, st[k, b])
            assert not x[k, b][s["fixed"]].any() and not x[k, b][~s["anchored"]].any()
    print("%s: iterations %d .. %d, worst true residual / (tolerance + d) %.3g" %
          (name, st["iterations"][st["status"] == gc.OK].min(), st["iterations"].max(), worst))


@pytest.mark.parametrize("name", list(CASES))
def test_blocks_equal_the_dense_inverse(name):
    c, s, g = CASES[name], _model(name), _graph(name)
    q = c["query"]
    rows = [r for r in q for _ in q]
    cols = [v for _ in q for v in q]
    blocks, st = g.covariance(rows, cols, **_opt(c))
    got = {}
    worst = 0.0
    for k, (r, v) in enumerate(zip(rows, cols)):
        want, wst = gc.block(s, r, v)
        assert st[k] == wst, (r, v)
        if (r, v) in got:
            assert blocks[k].tobytes() == got[(r, v)].tobytes()          # a duplicate query: equal bytes
        got[(r, v)] = blocks[k]
        if wst != gc.OK:
            assert np.isnan(blocks[k]).all()
            continue
        if s["fixed"][r] or s["fixed"][v]:
            assert not blocks[k].any()                                 # exactly 0
            continue
        xn = max(float(np.linalg.norm(gc.column(s, v, b))) for b in range(6))
        bound = gc.block_bound(s, c["pcg_tolerance"], gc.drift_allowance(s, c["max_pcg_iterations"], xn), want)
        err = float(np.linalg.norm(blocks[k] - want, 2))
        worst = max(worst, err / bound)
        assert err <= bound, (r, v, err, bound)
    for (r, v), blk in got.items():
        if gc.block(s, r, v)[1] != gc.OK or s["fixed"][r] or s["fixed"][v]:
            continue
        want = gc.block(s, r, v)[0]
        xn = max(float(np.linalg.norm(gc.column(s, n, b))) for b in range(6) for n in (r, v))
        bound = gc.block_bound(s, c["pcg_tolerance"], gc.drift_allowance(s, c["max_pcg_iterations"], xn), want)
        assert float(np.linalg.norm(blk - got[(v, r)].T, 2)) <= 2.0 * bound
    marg, mst = g.covariance(q, **_opt(c))                               # cols None: the marginals
    for k, n in enumerate(q):
        assert mst[k] == gc.block(s, n, n)[1] and marg[k].tobytes() == got[(n, n)].tobytes()
    print("%s: worst block error / bound %.3g" % (name, worst))


@pytest.mark.parametrize("name", ["chain5", "chain65", "ring1030", "ring12_two_loops", "two_components", "weighted_ring"])
def test_equal_bytes_whatever_the_batching_and_nothing_else_moves(name):
    c, g = CASES[name], _graph(name)
    poses, edges, active, lin = g.poses(), g.edges(), g.edge_active(), g.linearize()
    q = c["query"]
    x0, st0 = g.solve_columns(q, **_opt(c))
    b0, bs0 = g.covariance(q, q[::-1], **_opt(c))
    for batch in (6, 7, 0, 0):                                           # 0: automatic; twice: two calls give the same
        x, st = g.solve_columns(q, **_opt(c, batch_columns=batch))
        assert x.tobytes() == x0.tobytes() and st.tobytes() == st0.tobytes()
        b, bs = g.covariance(q, q[::-1], **_opt(c, batch_columns=batch))
        assert b.tobytes() == b0.tobytes() and bs.tobytes() == bs0.tobytes()
    assert g.poses().tobytes() == poses.tobytes() and g.edges().tobytes() == edges.tobytes() and np.array_equal(g.edge_active(), active)
    for a, b in zip(lin, g.linearize()):
        assert a.tobytes() == b.tobytes()
    h = _make(c)                                                         # an equal graph: equal bytes
    x, st = h.solve_columns(q, **_opt(c, batch_columns=1))
    assert x.tobytes() == x0.tobytes() and st.tobytes() == st0.tobytes()
    h.close()


def test_statuses():
    import liodom_amd as la
    # an unanchored node: UNANCHORED, NaN, and no column of it is launched
    c, s, g = CASES["two_components"], _model("two_components"), _graph("two_components")
    l0, c0 = g.cov_counters()
    blocks, st = g.covariance([7, 9, 7, 0], [7, 7, 9, 8], **_opt(c))
    assert list(st) == [gc.UNANCHORED] * 3 + [gc.OK] and np.isnan(blocks[:3]).all() and not blocks[3].any()
    x, cst = g.solve_columns([8], **_opt(c))
    assert (cst["status"] == gc.UNANCHORED).all() and np.isnan(x).all()
    assert g.cov_counters() == (l0, c0)
    blocks, st = g.covariance([7, 1, 2], [7, 1, 1], **_opt(c, batch_columns=4))
    assert list(st) == [gc.UNANCHORED, gc.OK, gc.OK] and g.cov_counters() == (l0 + 2, c0 + 6)          # node 1's six columns, 4 + 2
    cand = gm.api.graph_edges([1, 1], [7, 2], [gm.between(c["poses"][1], c["poses"][7]), gm.between(c["poses"][1], c["poses"][2])], gm.OMEGA)
    d2, gst = g.gate_edges(cand, **_opt(c))
    assert gst[0] == gc.UNANCHORED and np.isnan(d2[0]) and gst[1] == gc.OK and np.isfinite(d2[1])
    # an Omega of the candidate that is not positive definite
    cand["info"][1] = -cand["info"][1]
    d2, gst = g.gate_edges(cand[1:], **_opt(c))
    assert gst[0] == gc.NOT_PD and np.isnan(d2[0])
    # one iteration on the 1030-node ring
    c, g = CASES["ring1030"], _graph("ring1030")
    x, cst = g.solve_columns([515], max_pcg_iterations=1, pcg_tolerance=c["pcg_tolerance"])
    assert (cst["status"] == gc.NOT_CONVERGED).all() and (cst["iterations"] == 1).all() and np.isfinite(x).all() and x.any()
    blocks, st = g.covariance([515], max_pcg_iterations=1, pcg_tolerance=c["pcg_tolerance"])
    assert st[0] == gc.NOT_CONVERGED and np.isfinite(blocks).all()
    # a stored edge with a negative definite Omega: the solve breaks down, it does not hang
    c = CASES["chain5"]
    bad = c["edges"].copy()
    bad["info"][2] = -bad["info"][2]
    h = _make(c, bad)
    x, cst = h.solve_columns([1, 0], **_opt(c))
    assert (cst["status"][0] == gc.BREAKDOWN).all() and np.isnan(x[0]).all() and (cst["status"][1] == gc.OK).all() and not x[1].any()
    blocks, st = h.covariance([1, 3, 0], [1, 1, 1], **_opt(c))
    assert list(st) == [gc.BREAKDOWN, gc.BREAKDOWN, gc.OK] and np.isnan(blocks[:2]).all() and not blocks[2].any()
    d2, gst = h.gate_edges(gm.api.graph_edges([1], [3], [gm.between(c["poses"][1], c["poses"][3])], gm.OMEGA), **_opt(c))
    assert gst[0] == gc.BREAKDOWN and np.isnan(d2[0])
    # refusals leave everything as it is
    for call in (lambda: h.covariance([5]), lambda: h.covariance([-1]), lambda: h.solve_columns([5]), lambda: h.covariance([1], pcg_tolerance=-1.0),
                 lambda: h.covariance([1], batch_columns=-1), lambda: h.solve_columns([1], max_pcg_iterations=-1),
                 lambda: h.gate_edges(gm.api.graph_edges([1], [1], [gm.between(c["poses"][1], c["poses"][3])], gm.OMEGA)),
                 lambda: h.gate_edges(gm.api.graph_edges([1], [5], [gm.between(c["poses"][1], c["poses"][3])], gm.OMEGA))):
        with pytest.raises(la.LiodomError) as err:
            call()
        assert err.value.code == la.api.ERR_INVALID_ARG
    assert h.covariance([])[0].shape == (0, 6, 6) and h.gate_edges(bad[:0])[0].shape == (0,) and h.solve_columns([])[0].shape[0] == 0
    h.close()


def _gate_bound(s, c, poses, cand, opt):
    i, j = int(cand["i"]), int(cand["j"])
    blocks = [gc.block(s, i, i)[0], gc.block(s, i, j)[0], gc.block(s, j, j)[0]]
    xn = max([float(np.linalg.norm(gc.column(s, n, b))) for b in range(6) for n in (i, j) if not s["fixed"][n]] + [0.0])
    d = gc.drift_allowance(s, opt["max_pcg_iterations"], xn)
    bb = max(gc.block_bound(s, opt["pcg_tolerance"], d, blk) for blk in blocks)
    poses = gm.normalised(poses)
    _, st, S, e, J = gc.gate_blocks(poses[i], poses[j], gm.normalised(cand["z"])[0], cand["info"], *blocks)
    assert st == gc.OK
    return gc.gate_bound(S, e, J, bb)


def test_the_gate_equals_the_model_and_tells_the_true_loop_from_the_displaced_one():
    import liodom_amd as la
    init, fixed, odo, true, false = gc.gate_ring()
    s = gc.system(gm.linearize(init, fixed, odo), fixed, odo)
    opt = dict(max_pcg_iterations=66, pcg_tolerance=1e-8)                 # (11 free nodes: the default cap)
    xn = max(float(np.linalg.norm(gc.column(s, 11, b))) for b in range(6))
    assert gc.drift_allowance(s, 66, xn) <= 1e-9
    g = la.PoseGraph(max_nodes=16, max_edges=32)
    g.add_nodes(init, fixed)
    g.add_edges(odo)
    inner = gm.api.graph_edges([3], [9], [gm.between(init[3], init[9])], gc.GATE_INFO)
    inner["z"][0, 4:] += [0.2, -0.1, 0.05]
    cand = np.concatenate([true, false, inner])
    d2, st = g.gate_edges(cand, **opt)
    for k in range(3):
        want, wst = gc.gate(s, init, cand[k])
        bound = _gate_bound(s, None, init, cand[k], opt)
        print("candidate %d: d2 %.12g, model %.12g, bound %.3g" % (k, d2[k], want, bound))
        assert st[k] == wst == gc.OK and abs(d2[k] - want) <= bound and bound <= 1e-3 * want
    assert d2[0] < gc.CHI2_6_099 and d2[1] > 100.0
    assert g.count() == (12, 11)
    g.close()
    # with weights and a switched-off edge
    c, sw, gw = CASES["weighted_ring"], _model("weighted_ring"), _graph("weighted_ring")
    cand = gm.api.graph_edges([2], [8], [gm.between(c["poses"][2], c["poses"][8])], gm.OMEGA)
    cand["z"][0, 4:] += [0.3, 0.1, -0.2]
    d2, st = gw.gate_edges(cand, **_opt(c))
    want, wst = gc.gate(sw, c["poses"], cand[0])
    assert st[0] == wst == gc.OK and abs(d2[0] - want) <= _gate_bound(sw, c, c["poses"], cand[0], _opt(c))


def test_loop_closer_gates_its_loop_edges():
    import liodom_amd as la
    from liodom_amd import loop
    init, fixed, odo, true, false = gc.gate_ring()
    cloud = np.zeros((0, 4), np.float32)
    for gate in (gc.CHI2_6_099, None):
        db = la.Places(max_places=8, max_edges=64)
        mp = la.Map(40.0, 50.0, 0.4, max_cells=64, cell_capacity=256, max_modified_cells=64)
        lc = loop.LoopCloser(mp, db, [], min_dist=0.5, min_gap=100, max_nodes=16, max_edges=32, odometry_info=gc.GATE_INFO, loop_info=gc.GATE_INFO,
                             gate=gate)
        for p in init:
            assert lc.feed(p, cloud)["key_frame"]
        assert lc.graph.count() == (12, 11)
        Zt, Zf = gm.normalised(true["z"])[0], gm.normalised(false["z"])[0]
        if gate is None:
            assert lc.add_loop(0, 11, Zt) and lc.add_loop(0, 11, Zf)
            assert lc.graph.count() == (12, 13) and lc.loops == [(0, 11), (0, 11)] and lc.gated == []
        else:
            assert lc.add_loop(0, 11, Zt) is True
            ed = lc.graph.edges()
            assert lc.graph.count() == (12, 12) and (int(ed["i"][11]), int(ed["j"][11]), int(ed["kind"][11])) == (0, 11, 1)
            assert np.max(np.abs(ed["z"][11] - Zt)) <= 1e-15 and np.array_equal(ed["info"][11], gc.GATE_INFO)
            # (the true edge is in the graph now: the displaced one is gated against a graph that already knows the loop)
            assert lc.add_loop(0, 11, Zf) is False
            assert lc.graph.count() == (12, 12) and lc.loops == [(0, 11)]
            (place, node, d2, status), = lc.gated
            assert (place, node, status) == (0, 11, "ok") and d2 > 100.0
        lc.graph.close()
        db.close()
        mp.close()
