"""Robust losses and switched-off edges of the pose graph on the device (liodom_graph_set_loss, _set_edge_active, _edge_weights;
api.PoseGraph; loop.LoopCloser.close(loss=, reject_below=)) against their NumPy restatement (tests/graph_robust_model.py).

Bounds of the robust linearisation.  s = e^T Omega e of an edge is returned raw, and within the bound of
tests/test_gpu_pose_graph.py: ds = 1e-13 |e|^T |Omega| |e|.  rho and w are functions of s computed by graph_loss, whose own
rounding tests/test_graph_loss_host.py bounds in units of u = 2^-53 — rho 4, 6, 5 u and w 3, 4, 9 u for Huber, Cauchy and
Geman-McClure on the host; the device's log1p is within 2 ulp where the host's is within 1, which adds 2 u to Cauchy's rho: 8 u.
An error of s goes through the derivative:
  rho   within w ds + U_rho u rho                                    (rho' = w, and w only falls with s: w at s - ds covers the step)
  w     within max |dw/ds| over [s - ds, s + ds] ds + U_w u w        (graph_robust_model.dw_ds; Huber's jumps from 0 at s = c^2,
                                                                      so the larger side counts)
  node sums   a node's gradient and diagonal block are sums over its ACTIVE edges of w x (the finished quadratic entry).  The
        quadratic sums are within 1e-12 x the sum of the absolute values of their products (test_gpu_pose_graph.py); times w that
        is 1e-12 x the WEIGHTED g_abs / D_abs (the product with w adds one rounding, u, far inside).  An error dw of an edge's
        weight moves the node sum by at most dw x that edge's unweighted absolute products, so: 1e-12 x weighted g_abs / D_abs
        + sum over the node's edges of dw_e x (|J|^T |Omega| |e|, |J|^T |Omega| |J|).
After a solve the loop edges' errors are millimetres on edges metres long: e is then little more than its own rounding, and ds takes
the form test_gpu_pose_graph.py derives for its special edges — the per-edge bound on e, 1e-13 x scale (scale = 1 + |t_j - t_i| +
|t_z|), carried through the product: ds = 1e-13 |e|^T |Omega| |e| + 2e-13 scale |e|^T |Omega| 1 (`small_errors` below).
Nothing here is fitted to the device's output; the tests print the share of each bound that is used.
Poses after a solve: within 1e-4 m and 1e-4 rad of the model's dense Levenberg-Marquardt, the project's parity bound."""
import numpy as np
import pytest

import graph_model as gm
import graph_robust_model as rm
from liodom_amd import api

pytestmark = pytest.mark.gpu

OPT = dict(pcg_tolerance=1e-10, max_iterations=50)
U = 2.0 ** -53
ULP_UNITS = {"none": (0, 0), "huber": (4, 3), "cauchy": (8, 4), "geman_mcclure": (5, 9)}          # (rho, w), module docstring
GM5 = {1: ("geman_mcclure", 5.0)}


def make_graph(poses, fixed, edges, table=None, active=None, **caps):
    g = api.PoseGraph(max_nodes=caps.get("max_nodes", max(len(poses), 1)), max_edges=caps.get("max_edges", max(len(edges), 1)))
    assert g.add_nodes(poses, fixed) == 0
    if len(edges):
        g.add_edges(edges)
    for kind, (name, scale) in (table or {}).items():
        g.set_loss(kind, name, scale)
    if active is not None:
        g.set_edge_active(0, active)
    assert g.count() == (len(poses), len(edges))
    return g


def weight_bounds(lin, edges, table, active, small_errors=False):
    """(ds, drho, dw) per edge: the module docstring's bounds at the model's s."""
    E = len(edges)
    names = rm.edge_losses(edges, table)
    ds, drho, dw = np.zeros(E), np.zeros(E), np.zeros(E)
    for k in range(E):
        ae = np.abs(lin["e"][k])
        ds[k] = 1e-13 * (ae @ np.abs(edges["info"][k]) @ ae)
        if small_errors:
            ds[k] += 2e-13 * lin["scale"][k] * (ae @ np.abs(edges["info"][k]) @ np.ones(6))
        if not active[k]:
            continue
        name, c = names[k]
        s = lin["chi2"][k]
        w_lo = rm.loss(name, c, max(s - ds[k], 0.0))[1]
        slope = max(abs(rm.dw_ds(name, c, v)) for v in (max(s - ds[k], 0.0), s, s + ds[k]))
        drho[k] = w_lo * ds[k] + ULP_UNITS[name][0] * U * lin["rho"][k]
        dw[k] = slope * ds[k] + ULP_UNITS[name][1] * U * lin["w"][k]
    return ds, drho, dw


def used(d, tol):
    return float(np.max(np.where(d > 0.0, d / np.maximum(tol, 1e-300), 0.0))) if d.size else 0.0


def check_robust_linearize(poses, fixed, edges, table, active, label):
    g = make_graph(poses, fixed, edges, table, active)
    chi2, grad, D = g.linearize()
    rho, w = g.edge_weights()
    assert np.array_equal(g.edge_active(), np.asarray(active) != 0)
    g.close()
    lin = rm.linearize(poses, fixed, edges, table, active)
    ds, drho, dw = weight_bounds(lin, edges, table, lin["active"])
    g_tol, D_tol = 1e-12 * lin["g_abs"], 1e-12 * lin["D_abs"]
    for k in range(len(edges)):
        if not lin["active"][k]:
            continue
        Om, ae = np.abs(edges["info"][k]), np.abs(lin["e"][k])
        for n, J in ((int(edges["i"][k]), np.abs(lin["A"][k])), (int(edges["j"][k]), np.abs(lin["B"][k]))):
            g_tol[n] += dw[k] * (J.T @ Om @ ae)
            D_tol[n] += dw[k] * (J.T @ Om @ J)
    fx = np.asarray(fixed) != 0
    assert np.all(grad[fx] == 0.0), label
    off = ~lin["active"]
    assert np.all(rho[off] == 0.0) and np.all(w[off] == 0.0), label
    assert np.all((w >= 0.0) & (w <= 1.0)) and np.all(rho <= chi2), label
    dc, dr, dwt = np.abs(chi2 - lin["chi2"]), np.abs(rho - lin["rho"]), np.abs(w - lin["w"])
    dg, dD = np.abs(grad - lin["g"]), np.abs(D - lin["D"])
    print("%s: chi2 at %.3f of its bound, rho at %.3f, w at %.3f, gradient at %.3f, diagonal blocks at %.3f"
          % (label, used(dc, ds), used(dr, drho), used(dwt, dw), used(dg, g_tol), used(dD, D_tol)))
    assert np.all(dc <= ds), (label, "chi2")
    assert np.all(dr <= drho), (label, "rho")
    assert np.all(dwt <= dw), (label, "w")
    assert np.all(dg <= g_tol), (label, "gradient")
    assert np.all(dD <= D_tol), (label, "diagonal blocks")
    return lin


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("degree", [1, 63, 64, 65, 257])
def test_robust_linearize_a_hub(degree, side):
    """Kinds cycle over 0 .. 3 with none, Huber, Cauchy and Geman-McClure on them; every fifth edge is switched off; one scale for
    all, the square root of the median s of the active Huber edges, so that half of those sit on each branch."""
    poses, fixed, edges = gm.hub(degree, side, seed=100 + degree + side)
    edges = edges.copy()
    edges["kind"] = np.arange(degree) % 4
    active = (np.arange(degree) % 5 != 4).astype(np.int32)
    s = gm.linearize(poses, fixed, edges)["chi2"]
    huber = (edges["kind"] == 1) & (active != 0)
    c = float(np.sqrt(np.median(s[huber]))) if np.any(huber) else float(np.sqrt(np.median(s)))
    table = {0: ("none", 1.0), 1: ("huber", c), 2: ("cauchy", c), 3: ("geman_mcclure", c)}
    lin = check_robust_linearize(poses, fixed, edges, table, active, "hub of degree %d as side %d" % (degree, side))
    assert lin["degree"][0] == int(np.sum(active))
    if degree >= 63:
        share = float(np.mean(lin["w"][huber] < 1.0))
        print("    %d active Huber edges, %.2f of them past s = c^2" % (int(np.sum(huber)), share))
        assert 1.0 / 3.0 <= share <= 2.0 / 3.0
        assert np.all(lin["w"][(edges["kind"] == 0) & (active != 0)] == 1.0)
    fixed[0] = 1                                                            # ... and with the hub fixed
    check_robust_linearize(poses, fixed, edges, table, active, "fixed hub of degree %d as side %d" % (degree, side))


@pytest.mark.parametrize("n", [2, 1024, 1025])
def test_multiply_on_a_chain_cut_in_two(n):
    """Cauchy on the chain's edges and the edge (n / 2 - 1, n / 2) switched off: two segments (at n = 2 no active edge at all: the
    free node is a node without edges, y = x)."""
    poses, fixed, edges = gm.chain(n, seed=n)
    table = {0: ("cauchy", 0.3)}
    active = np.ones(len(edges), np.int32)
    cut = n // 2 - 1
    assert (int(edges["i"][cut]), int(edges["j"][cut])) == (n // 2 - 1, n // 2)
    active[cut] = 0
    g = make_graph(poses, fixed, edges, table, active)
    lin = rm.linearize(poses, fixed, edges, table, active)
    assert lin["degree"][n // 2] == (0 if n == 2 else 1) and lin["degree"][n // 2 - 1] == (0 if n == 2 else 1)
    assert n == 2 or np.all(lin["w"][active != 0] < 0.999)
    x = np.random.default_rng(n).normal(size=(n, 6))
    for lam in (0.0, 1.0):
        y = g.multiply(x, lam)
        want, y_abs = rm.multiply(lin, fixed, edges, x, lam)
        assert np.all(y[fixed != 0] == 0.0)
        worst = float(np.max(np.abs(y - want) / np.maximum(1e-12 * y_abs, 1e-300)))
        print("cut chain of %d, lambda %g: at %.3f of the bound" % (n, lam, worst))
        assert np.all(np.abs(y - want) <= 1e-12 * y_abs)
    if n == 2:
        assert np.array_equal(g.multiply(x, 0.0)[1], x[1])
    g.close()


def test_weight_one_everywhere_is_the_quadratic_path_byte_for_byte():
    """ring48 untouched against ring48 with Huber of scale 1e300 on both kinds — the robust kernels run, every w is exactly 1 —
    and set_edge_active called with all ones."""
    _, init, fixed, edges = gm.drifted_ring(48, 2, seed=48)
    runs = []
    for robust in (False, True):
        g = make_graph(init, fixed, edges)
        if robust:
            g.set_loss(0, "huber", 1e300)
            g.set_loss(1, 1, 1e300)                                        # by number
            g.set_edge_active(0, np.ones(len(edges)))
            assert g.loss(0) == ("huber", 1e300) and g.loss(1) == ("huber", 1e300) and g.loss(2) == ("none", 0.0)
        lin0 = [a.tobytes() for a in g.linearize()]
        y0 = g.multiply(np.ones((48, 6)), 0.5).tobytes()
        rep = g.optimize(**OPT)
        chi2 = g.linearize()[0]
        rho, w = g.edge_weights()
        assert np.all(w == 1.0) and np.array_equal(rho, chi2)
        runs.append((g.poses().tobytes(), rep, [a.tobytes() for a in g.linearize()], lin0, y0))
        g.close()
    assert runs[0][1]["accepted_steps"] >= 2
    for a, b in zip(runs[0], runs[1]):
        assert a == b


_REF = {}


def false_loop_reference(n_loops):
    """ring_with_false_loop(48, n_loops, 48), the model's clean solution and its robust dense solve, made once."""
    if n_loops not in _REF:
        _, init, fixed, edges, fi = rm.ring_with_false_loop(48, n_loops, 48)
        clean, _ = gm.lm(init, fixed, rm.clean(edges, fi), max_iterations=50)
        robust, rep = rm.lm(init, fixed, edges, GM5, max_iterations=50)
        _REF[n_loops] = dict(init=init, fixed=fixed, edges=edges, fi=fi, clean=clean, robust=robust, rep=rep)
    return _REF[n_loops]


@pytest.mark.parametrize("n_loops", [2, 4])
def test_the_robust_solve_equals_the_model(n_loops):
    r = false_loop_reference(n_loops)
    init, fixed, edges, fi = r["init"], r["fixed"], r["edges"], r["fi"]
    g = make_graph(init, fixed, edges, GM5)
    rep = g.optimize(**OPT)
    out = g.poses()
    chi2 = g.linearize()[0]
    rho, w = g.edge_weights()
    g.close()
    dm, dr = rm.max_distance(out, r["robust"])
    cm, cr = rm.max_distance(out, r["clean"])
    print("ring48 + false loop, %d true loops, Geman-McClure 5: %s after %d steps (%d accepted, %d PCG iterations), cost %.6g -> %.6g (model %.6g -> %.6g in %d); "
          "%.3g m / %.3g rad from the model, %.3g m / %.3g rad from clean; false weight %.3g, true >= %.4f"
          % (n_loops, rep["termination"], rep["iterations"], rep["accepted_steps"], rep["pcg_iterations"], rep["initial_cost"], rep["final_cost"],
             r["rep"]["initial_cost"], r["rep"]["final_cost"], r["rep"]["iterations"], dm, dr, cm, cr, w[fi], np.min(w[len(init) - 1:fi])))
    assert rep["termination"] in ("gradient", "cost") and r["rep"]["termination"] in ("gradient", "cost")
    assert dm <= 1e-4 and dr <= 1e-4
    assert abs(rep["final_cost"] - rm.cost(out, edges, GM5)) <= 1e-12 * rep["final_cost"]
    assert abs(rep["initial_cost"] - r["rep"]["initial_cost"]) <= 1e-12 * rep["initial_cost"]
    # the weights are the model's at the poses returned, within the linearisation's bounds
    lin = rm.linearize(out, fixed, edges, GM5)
    ds, drho, dw = weight_bounds(lin, edges, GM5, lin["active"], small_errors=True)
    print("    at the poses returned: chi2 at %.3f of its bound, rho at %.3f, w at %.3f"
          % (used(np.abs(chi2 - lin["chi2"]), ds), used(np.abs(rho - lin["rho"]), drho), used(np.abs(w - lin["w"]), dw)))
    assert np.all(np.abs(chi2 - lin["chi2"]) <= ds), "chi2"
    assert np.all(np.abs(rho - lin["rho"]) <= drho), "rho"
    assert np.all(np.abs(w - lin["w"]) <= dw), "w"
    loops = np.nonzero(edges["kind"] == 1)[0]
    assert w[fi] < 0.01 and np.all(w[[k for k in loops if k != fi]] > 0.9) and np.all(w[edges["kind"] == 0] == 1.0)
    assert np.max(np.abs(w - rm.edge_costs(r["robust"], edges, GM5)[2])) <= 1e-3          # (poses 1e-4 apart: |dw/ds| ds << 1e-3)
    # what the feature changes: the same graph with no loss
    g = make_graph(init, fixed, edges)
    g.optimize(**OPT)
    bent = g.poses()
    g.close()
    bm, br = rm.max_distance(bent, r["clean"])
    print("    with no loss: %.3g m / %.3g rad from clean" % (bm, br))
    assert bm > 1.0


def test_an_inactive_edge_is_an_absent_edge():
    r = false_loop_reference(2)
    init, fixed, edges, fi = r["init"], r["fixed"], r["edges"], r["fi"]
    active = np.ones(len(edges), np.int32)
    active[fi] = 0
    g = make_graph(init, fixed, edges, None, active)
    s0 = g.linearize()[0]
    rep = g.optimize(**OPT)
    out = g.poses()
    chi2 = g.linearize()[0]
    rho, w = g.edge_weights()
    assert len(g.edges()) == len(edges) and g.edges()[fi]["i"] == 36           # get_edges still returns it
    g.close()
    h = make_graph(init, fixed, rm.clean(edges, fi))
    rep_h = h.optimize(**OPT)
    absent = h.poses()
    h.close()
    dm, dr = rm.max_distance(out, absent)
    print("ring48, false edge switched off: %.3g m / %.3g rad from the graph without it; cost %.6g against %.6g" % (dm, dr, rep["final_cost"], rep_h["final_cost"]))
    assert dm <= 1e-4 and dr <= 1e-4 and rm.max_distance(out, r["clean"])[0] <= 1e-4
    assert abs(rep["final_cost"] - rep_h["final_cost"]) <= 1e-9 * rep_h["final_cost"]
    for poses, got in ((init, s0), (out, chi2)):                               # its chi2 stays the raw s
        lin = rm.linearize(poses, fixed, edges, None, active)
        ae = np.abs(lin["e"][fi])                                              # (an error of metres: the plain bound)
        assert lin["chi2"][fi] > 100.0 and abs(got[fi] - lin["chi2"][fi]) <= 1e-13 * (ae @ np.abs(edges["info"][fi]) @ ae)
    assert rho[fi] == 0.0 and w[fi] == 0.0 and np.all(w[active != 0] == 1.0) and np.array_equal(rho[active != 0], chi2[active != 0])
    assert abs(rep["final_cost"] - float(np.sum(rho))) <= 1e-12 * rep["final_cost"]


def test_a_node_whose_edges_are_all_inactive_stays():
    """Node 8 hangs on the chain edge (7, 8) and on nothing else, node 9 on (3, 9): with both edges off they are nodes without
    edges — no chain parent, identity block — and must not break the solve down."""
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    lone = np.stack([gm.from_axis_angle((1, 2, 3), 0.7, (5.0, 6.0, 7.0)), gm.from_axis_angle((3, 2, 1), -0.4, (-1.0, 2.0, 0.5))])
    extra = api.graph_edges([7, 3], [8, 9], [gm.between(init[7], lone[0]), gm.pose([0, 0, 0, 1], [9.0, 9.0, 9.0])], gm.OMEGA)
    poses, fx, ed = np.concatenate([init, lone]), np.concatenate([fixed, [0, 0]]), np.concatenate([edges, extra])
    active = np.ones(len(ed), np.int32)
    active[len(edges):] = 0
    g = make_graph(poses, fx, ed, {0: ("cauchy", 2.0)}, active)
    start = g.poses().copy()
    x = np.arange(60, dtype=np.float64).reshape(10, 6)
    y = g.multiply(x)
    assert np.array_equal(y[8:], x[8:])
    _, grad, D = g.linearize()
    assert np.all(grad[8:] == 0.0) and np.all(D[8:] == 0.0)
    rep = g.optimize(**OPT)
    out = g.poses()
    print("two nodes without active edges: %s after %d steps, %d accepted" % (rep["termination"], rep["iterations"], rep["accepted_steps"]))
    assert rep["termination"] in ("gradient", "cost") and rep["accepted_steps"] >= 1
    assert out[8:].tobytes() == start[8:].tobytes()
    want, _ = rm.lm(poses, fx, ed, {0: ("cauchy", 2.0)}, active, max_iterations=50)
    dm, dr = rm.max_distance(out, want)
    assert dm <= 1e-4 and dr <= 1e-4
    # every edge off: nothing to solve
    g.set_edge_active(0, np.zeros(len(ed)))
    rep = g.optimize(**OPT)
    assert (rep["iterations"], rep["termination"], rep["initial_cost"], rep["final_cost"]) == (0, "gradient", 0.0, 0.0)
    assert np.array_equal(g.poses(), out)
    g.close()


def test_two_robust_runs_on_equal_graphs_return_equal_bytes():
    r = false_loop_reference(2)
    active = np.ones(len(r["edges"]), np.int32)
    active[5] = 0
    runs = []
    for _ in range(2):
        g = make_graph(r["init"], r["fixed"], r["edges"], {0: ("huber", 0.5), 1: ("geman_mcclure", 5.0)}, active, max_nodes=64, max_edges=80)
        rep = g.optimize(**OPT)
        runs.append((g.poses().tobytes(), rep, [a.tobytes() for a in g.linearize()], [a.tobytes() for a in g.edge_weights()]))
        g.close()
    assert runs[0][1]["accepted_steps"] >= 1
    assert runs[0] == runs[1]


def test_errors_leave_the_graph_untouched_and_reset_keeps_the_losses():
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    g = make_graph(init, fixed, edges, {1: ("cauchy", 2.5)}, None, max_nodes=9, max_edges=9)
    g.set_edge_active(2, [0, 0])

    def state():
        return (g.poses().tobytes(), g.edges().tobytes(), g.edge_active().tobytes(), [g.loss(k) for k in range(16)], [a.tobytes() for a in g.edge_weights()])

    before = state()
    assert before[3][1] == ("cauchy", 2.5) and g.edge_active().tolist() == [True, True, False, False, True, True, True, True]

    def refused(call):
        with pytest.raises(api.LiodomError) as err:
            call()
        assert err.value.code == api.ERR_INVALID_ARG
        assert g.count() == (8, 8) and state() == before

    for kind in (-1, 16, 1 << 20):
        refused(lambda: g.set_loss(kind, "huber", 1.0))
        refused(lambda: g.loss(kind))
    for bad in (-1, 4, 99):
        refused(lambda: g.set_loss(1, bad, 1.0))
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        refused(lambda: g.set_loss(1, "geman_mcclure", scale))
    refused(lambda: g.set_edge_active(-1, [1]))
    refused(lambda: g.set_edge_active(7, [1, 1]))
    refused(lambda: g.set_edge_active(9, []))
    refused(lambda: g.edge_active(7, 2))
    refused(lambda: g.edge_active(-1, 1))
    g.set_edge_active(8, [])                                    # an empty range at the end is a range
    assert state() == before
    g.set_loss(3, "none", float("nan"))                         # the scale is not read for none
    assert g.loss(3) == ("none", 0.0)
    g.reset()
    assert g.count() == (0, 0) and g.loss(1) == ("cauchy", 2.5) and g.edge_active().shape == (0,)
    rho, w = g.edge_weights()
    assert rho.shape == (0,) and w.shape == (0,)
    g.add_nodes(init, fixed)
    g.add_edges(edges)
    assert np.all(g.edge_active())                              # edges are active when added
    g.close()


# ---------------------------------------------------------------------------------------------
# LoopCloser: the two-stage close on a designed ring, no scans
# ---------------------------------------------------------------------------------------------
def _closer():
    """A LoopCloser over a small real Map and Places, no search levels, fed the 48 dead-reckoned poses of
    graph_robust_model.closer_ring() — drifted_ring(48, 2, 48) at a 4 m step, min_dist 3 m: every pose is a key frame (the shortest
    step of the dead-reckoned ring is checked to be above it) — with an 8-point cloud each, the two true loops and the false one
    (12, 36, identity) added through add_loop.  On the model (tests/test_graph_robust_model.py, the rescaled ring) Geman-McClure
    with scale 5 keeps the gap on this ring: false weight 4.3e-9, true weights 0.992 and 0.984 — the scale of the 1 m ring stands."""
    import liodom_amd as la
    from liodom_amd import loop
    init, fixed, edges, loops, fi = rm.closer_ring()
    m = la.Map(12.0, 50.0, 0.4, max_cells=512, cell_capacity=4096, max_modified_cells=256)
    db = la.Places(max_places=64, max_edges=2048)
    lc = loop.LoopCloser(m, db, [], min_dist=3.0, min_gap=10, max_nodes=64, max_edges=128)
    cloud = np.zeros((8, 4), np.float32)
    cloud[:, 0] = np.arange(8) + 3.0
    cloud[:, 2] = 0.25 * np.arange(8)
    for k in range(48):
        assert lc.feed(init[k], cloud)["key_frame"]
    for place, node, Z in loops:
        lc.add_loop(place, node, Z)
    assert lc.loops == [(l[0], l[1]) for l in loops] and db.count() == 38
    return lc, m, db, init, fixed, loops


def _model_clean(lc, fixed):
    """The model's dense solve of the graph the LoopCloser holds, without its last edge (the false loop)."""
    edges = lc.graph.edges()
    clean, rep = gm.lm(lc.graph.poses(), fixed, edges[:-1], max_iterations=50)
    assert rep["termination"] in ("gradient", "cost")
    return clean


def test_the_two_stage_close_rejects_the_false_loop():
    from liodom_amd import loop
    lc, m, db, init, fixed, loops = _closer()
    with pytest.raises(ValueError):
        lc.close(reject_below=0.5)
    for bad in ((12, 12), (36, 12), (-1, 5), (5, 48)):
        with pytest.raises(ValueError):
            lc.add_loop(bad[0], bad[1], loops[-1][2])
    assert lc.graph.count() == (48, 50)
    clean = _model_clean(lc, fixed)
    out = lc.close(loss=("geman_mcclure", 5.0), reject_below=0.5, **OPT)
    assert out["applied"] and [r[:2] for r in out["rejected"]] == [(12, 36)] and [k[:2] for k in out["kept"]] == [l[:2] for l in loops[:2]]
    assert out["rejected"][0][2] < 0.01 and all(k[2] > 0.9 for k in out["kept"])
    assert lc.loops == [l[:2] for l in loops[:2]] and lc.rejected == out["rejected"]
    dm, dr = rm.max_distance(out["after"], clean)
    print("two-stage close: rejected %s, kept %s; robust solve %s after %d steps, second solve %s after %d; %.3g m / %.3g rad from the model's clean solution"
          % (out["rejected"], out["kept"], out["robust_report"]["termination"], out["robust_report"]["iterations"], out["report"]["termination"],
             out["report"]["iterations"], dm, dr))
    assert dm <= 1e-4 and dr <= 1e-4
    assert lc.graph.loss(1) == ("none", 0.0) and lc.graph.loss(0) == ("none", 0.0)
    assert lc.graph.edge_active().tolist() == [True] * 49 + [False]
    assert np.all(lc.graph.edges()["kind"][:47] == 0) and np.array_equal(lc.graph.poses(), out["after"])
    st = api.parse_place_state(db.export_state())
    assert st["count"] == 38 and np.array_equal(st["poses"], out["after"][:38]) and list(st["ids"]) == list(range(38))
    assert m.status() == 0 and 0 < m.all().shape[0] <= 48 * 8
    assert np.array_equal(np.stack(lc.key_poses), out["after"])
    # a second identical LoopCloser, closed the plain way, is bent by the false edge
    lc.graph.close(); m.close(); db.close()
    lc, m, db, init, fixed, loops = _closer()
    plain = lc.close(**OPT)
    pm_, pr_ = rm.max_distance(plain["after"], clean)
    print("plain close: %.3g m / %.3g rad from the model's clean solution" % (pm_, pr_))
    assert pm_ > 1.0 and "rejected" not in plain and lc.loops == [l[:2] for l in loops]
    lc.graph.close(); m.close(); db.close()


def test_close_applies_nothing_when_every_loop_is_rejected():
    lc, m, db, init, fixed, loops = _closer()
    m.update(np.array([[1.0, 2.0, 3.0, 0.0], [4.0, 5.0, 6.0, 0.0]], np.float32), api.pose_T34(init[0]))
    before = (m.all().tobytes(), db.export_state(), lc.graph.poses().tobytes(), lc.graph.edge_active().tobytes(), [p.tobytes() for p in lc.key_poses], list(lc.loops))
    out = lc.close(loss=("geman_mcclure", 5.0), reject_below=2.0, **OPT)          # no weight reaches 2: every loop edge is rejected
    assert out["applied"] is False and len(out["rejected"]) == 3 and out["kept"] == [] and out["report"] is None
    assert out["robust_report"]["accepted_steps"] >= 1 and np.array_equal(out["after"], out["before"])
    after = (m.all().tobytes(), db.export_state(), lc.graph.poses().tobytes(), lc.graph.edge_active().tobytes(), [p.tobytes() for p in lc.key_poses], list(lc.loops))
    assert after == before and lc.rejected == [] and lc.graph.loss(1) == ("none", 0.0)
    lc.graph.close(); m.close(); db.close()
