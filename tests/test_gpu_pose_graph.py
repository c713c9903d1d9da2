"""The pose graph on the device (liodom_graph_*; api.PoseGraph) against its NumPy restatement (tests/graph_model.py).

Bounds of the linearisation.  What the library returns are chi2 per edge and, per node, the sums of its edges' A^T Omega e and
A^T Omega A.
  node sums   within 1e-12 x the sum of the absolute values of the products they are made of (graph_model.linearize: g_abs =
              sum |J|^T |Omega| |e|, D_abs = sum |J|^T |Omega| |J|, and why products) and nothing else: eps x (degree + about 40
              operations) is <= 3e-13 at the largest degree used, 1025.
  chi2        within 1e-13 x |e|^T |Omega| |e|: 48 products and sums (1e-14) and twice the relative error of e, which on these
              graphs (|e| of the order of the scale) is the 30 eps of tests/test_graph_math_host.py: 1.3e-14.
These hold on every graph but one: the SPECIAL edges (an error that is exactly zero, translations of 100 km), where e, and with it
every term and every sum of absolute values, is nothing but the rounding of e itself, or 1e-5 of the scale.  There, and only
there, the per-edge bound on e, A and B — 1e-13 * scale, scale = 1 + |t_j - t_i| + |t_z| — is carried through each product and
added: 2e-13 scale |e|^T |Omega| 1 for chi2, 1e-13 scale (1^T |Omega| |e| + |A|^T |Omega| 1) for a gradient term,
2e-13 scale sym(|A|^T |Omega| 1 1^T) for a block term.  The test prints how much of each bound is used.
Poses after optimisation: within 1e-4 m and 1e-4 rad of the model's dense Levenberg-Marquardt, the project's parity bound."""
import numpy as np
import pytest

import graph_model as gm
from liodom_amd import api

pytestmark = pytest.mark.gpu

OPT = dict(pcg_tolerance=1e-10, max_iterations=50)


def make_graph(poses, fixed, edges, **caps):
    g = api.PoseGraph(max_nodes=caps.get("max_nodes", max(len(poses), 1)), max_edges=caps.get("max_edges", max(len(edges), 1)))
    assert g.add_nodes(poses, fixed) == 0
    if len(edges):
        g.add_edges(edges)
    assert g.count() == (len(poses), len(edges))
    return g


def check_linearize(poses, fixed, edges, label, special=False):
    g = make_graph(poses, fixed, edges)
    chi2, grad, D = g.linearize()
    g.close()
    lin = gm.linearize(poses, fixed, edges)
    E = len(edges)
    g_tol, D_tol, c_tol = 1e-12 * lin["g_abs"], 1e-12 * lin["D_abs"], np.zeros(E)
    ones = np.ones(6)
    for k in range(E):
        Om = np.abs(edges["info"][k])
        ae, s = np.abs(lin["e"][k]), lin["scale"][k]
        c_tol[k] = 1e-13 * (ae @ Om @ ae)
        if special:                      # the per-edge bound on e, A and B carried through the products (module docstring)
            c_tol[k] += 2e-13 * s * (ae @ Om @ ones)
            for n, J in ((int(edges["i"][k]), np.abs(lin["A"][k])), (int(edges["j"][k]), np.abs(lin["B"][k]))):
                g_tol[n] += 1e-13 * s * ((ones @ Om @ ae) + J.T @ Om @ ones)
                M = J.T @ Om @ np.ones((6, 6))
                D_tol[n] += 2e-13 * s * 0.5 * (M + M.T)
    fx = np.asarray(fixed) != 0
    assert np.all(grad[fx] == 0.0), label
    dg, dD, dc = np.abs(grad - lin["g"]), np.abs(D - lin["D"]), np.abs(chi2 - lin["chi2"])

    def used(d, tol):
        return float(np.max(np.where(d > 0.0, d / np.maximum(tol, 1e-300), 0.0))) if d.size else 0.0

    print("%s: chi2 at %.3f of its bound, gradient at %.3f, diagonal blocks at %.3f" % (label, used(dc, c_tol), used(dg, g_tol), used(dD, D_tol)))
    assert np.all(dc <= c_tol), (label, "chi2")
    assert np.all(dg <= g_tol), (label, "gradient")
    assert np.all(dD <= D_tol), (label, "diagonal blocks")
    return lin


def test_linearize_two_nodes_one_edge():
    rng = np.random.default_rng(1)
    poses = np.stack([gm.random_pose(rng), gm.random_pose(rng)])
    edges = api.graph_edges([0], [1], [gm.random_pose(rng, 3.0)], gm.OMEGA)
    check_linearize(poses, np.zeros(2, np.int32), edges, "one edge")
    check_linearize(poses, np.array([1, 0], np.int32), api.graph_edges([1], [0], [gm.random_pose(rng, 3.0)], gm.OMEGA), "one edge, reversed, node 0 fixed")


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("degree", [1, 63, 64, 65, 257, 1025])
def test_linearize_a_hub(degree, side):
    poses, fixed, edges = gm.hub(degree, side, seed=degree + side)          # non-diagonal Omega per edge
    lin = check_linearize(poses, fixed, edges, "hub of degree %d as side %d" % (degree, side))
    assert lin["degree"][0] == degree
    fixed[0] = 1                                                            # ... and with the hub fixed
    check_linearize(poses, fixed, edges, "fixed hub of degree %d as side %d" % (degree, side))


def test_linearize_the_special_edges():
    names, ii, jj, zs, poses = [], [], [], [], []
    for name, Xi, Xj, Z in gm.jacobian_cases():
        names.append(name)
        ii.append(len(poses)); jj.append(len(poses) + 1)
        poses += [Xi, Xj]
        zs.append(Z)
    assert any("w_negative" in n for n in names) and any("zero_error" in n for n in names) and any("100km" in n for n in names)
    rng = np.random.default_rng(9)
    M = rng.normal(size=(len(zs), 6, 6))
    info = M @ np.transpose(M, (0, 2, 1)) + np.eye(6)
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    fixed = np.zeros(len(poses), np.int32)
    fixed[::4] = 1
    check_linearize(np.stack(poses), fixed, api.graph_edges(ii, jj, np.stack(zs), info), "special edges", special=True)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025])
def test_multiply_on_chains(n):
    poses, fixed, edges = gm.chain(n, seed=n)
    if n > 4:
        fixed[n // 2] = 1
    g = make_graph(poses, fixed, edges)
    lin = gm.linearize(poses, fixed, edges)
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 6))
    for lam in (0.0, 1.0):
        y = g.multiply(x, lam)
        want, y_abs = gm.multiply(lin, fixed, edges, x, lam)
        assert np.all(y[fixed != 0] == 0.0)
        worst = float(np.max(np.abs(y - want) / np.maximum(1e-12 * y_abs, 1e-300))) if np.any(fixed == 0) else 0.0
        print("chain of %d, lambda %g: at %.3f of the bound" % (n, lam, worst))
        assert np.all(np.abs(y - want) <= 1e-12 * y_abs)
    g.close()


def _two_components():
    gt_a, init_a, fixed_a, edges_a = gm.drifted_ring(8, 1, seed=21)
    gt_b, init_b, fixed_b, edges_b = gm.drifted_ring(12, 2, seed=22)
    edges_b = edges_b.copy()
    edges_b["i"] += 8
    edges_b["j"] += 8
    return np.concatenate([init_a, init_b]), np.concatenate([fixed_a, fixed_b]), np.concatenate([edges_a, edges_b])


GRAPHS = {"ring8": lambda: gm.drifted_ring(8, 3, seed=8)[1:], "ring48": lambda: gm.drifted_ring(48, 2, seed=48)[1:],
          "ring257": lambda: gm.drifted_ring(257, 1, seed=257)[1:], "two_components": _two_components}
_REF = {}


def reference(name):
    """The graph and the model's dense solution, made once."""
    if name not in _REF:
        poses, fixed, edges = GRAPHS[name]()
        out, rep = gm.lm(poses, fixed, edges, max_iterations=50)
        _REF[name] = (poses, fixed, edges, out, rep)
    return _REF[name]


@pytest.mark.parametrize("name", list(GRAPHS))
def test_optimize_equals_the_dense_solve(name):
    """Rings of 8, 48 and 257 key frames and two components, pcg_tolerance 1e-10, max_iterations 50.  ring257 is the case that
    needs the preconditioner to work along the chain: with plain block-Jacobi every solve but the first runs into the cap of
    6 x free nodes iterations and 50 steps end 3.1e-3 m from the model (tools/pose_graph_cost.py measures both)."""
    poses, fixed, edges, want, want_rep = reference(name)
    g = make_graph(poses, fixed, edges)
    start = g.poses().copy()
    rep = g.optimize(**OPT)
    out = g.poses()
    g.close()
    assert np.max(np.abs(start - gm.normalised(poses))) <= 4e-16          # taken in with the quaternion divided by its norm
    dist = [gm.pose_distance(a, b) for a, b in zip(out, want)]
    print("%s: %s after %d steps (%d accepted, %d PCG iterations), chi2 %.6g -> %.6g (model %.6g -> %.6g in %d); worst %.3g m, %.3g rad from the model"
          % (name, rep["termination"], rep["iterations"], rep["accepted_steps"], rep["pcg_iterations"], rep["initial_cost"], rep["final_cost"],
             want_rep["initial_cost"], want_rep["final_cost"], want_rep["iterations"], max(d[0] for d in dist), max(d[1] for d in dist)))
    assert rep["termination"] in ("gradient", "cost") and want_rep["termination"] in ("gradient", "cost")
    assert max(d[0] for d in dist) <= 1e-4 and max(d[1] for d in dist) <= 1e-4
    assert abs(rep["final_cost"] - gm.chi2(out, edges)) <= 1e-12 * rep["final_cost"]
    assert abs(rep["initial_cost"] - want_rep["initial_cost"]) <= 1e-12 * rep["initial_cost"]
    assert rep["final_cost"] < rep["initial_cost"] and rep["accepted_steps"] >= 1
    assert np.array_equal(out[fixed != 0], start[fixed != 0])
    assert np.max(np.abs(np.linalg.norm(out[:, :4], axis=1) - 1.0)) <= 4e-16


def _permuted_ring():
    """ring48 with its nodes in a seeded random order (node 0 stays): hardly an edge joins n - 1 to n, the solve's preconditioner
    has no chain to work along and is block-Jacobi."""
    poses, fixed, edges = gm.drifted_ring(48, 2, seed=48)[1:]
    order = np.concatenate([[0], 1 + np.random.default_rng(4).permutation(47)])          # new index -> old index
    new_of = np.argsort(order)
    edges = edges.copy()
    edges["i"], edges["j"] = new_of[edges["i"]], new_of[edges["j"]]
    return poses[order], fixed[order], edges


def _segmented_ring():
    """ring48 with a second fixed node in the middle and one odometry edge turned round (j, i, Z^-1): the chain has three segments."""
    poses, fixed, edges = gm.drifted_ring(48, 2, seed=48)[1:]
    fixed, edges = fixed.copy(), edges.copy()
    fixed[20] = 1
    i, j = int(edges["i"][30]), int(edges["j"][30])
    edges["i"][30], edges["j"][30], edges["z"][30] = j, i, gm.inverse(gm.normalised(edges["z"][30])[0])
    return poses, fixed, edges


GRAPHS["permuted_ring48"] = _permuted_ring
GRAPHS["segmented_ring48"] = _segmented_ring


@pytest.mark.parametrize("name", ["permuted_ring48", "segmented_ring48"])
def test_optimize_where_the_chain_is_broken(name):
    poses, fixed, edges, want, want_rep = reference(name)
    if name == "permuted_ring48":
        assert int(np.sum(edges["j"] == edges["i"] + 1)) <= 3
    g = make_graph(poses, fixed, edges)
    start = g.poses().copy()
    rep = g.optimize(**OPT)
    out = g.poses()
    g.close()
    dist = [gm.pose_distance(a, b) for a, b in zip(out, want)]
    print("%s: %s after %d steps, %d PCG iterations; worst %.3g m, %.3g rad from the model" % (name, rep["termination"], rep["iterations"], rep["pcg_iterations"], max(d[0] for d in dist), max(d[1] for d in dist)))
    assert rep["termination"] in ("gradient", "cost") and max(d[0] for d in dist) <= 1e-4 and max(d[1] for d in dist) <= 1e-4
    assert abs(rep["final_cost"] - gm.chi2(out, edges)) <= 1e-12 * rep["final_cost"]
    assert np.array_equal(out[fixed != 0], start[fixed != 0])


def test_chi2_never_rises_over_accepted_steps():
    """The report has no cost per step, so the steps are taken one call at a time: each call tries one step from lambda = 1e-4,
    and its final cost is held to its initial cost and the next call's initial cost to it.  What happens between the steps of
    ONE call — lambda / 10 after an accept, the linearisation at the accepted poses — is checked through the first and last
    cost of test_optimize_equals_the_dense_solve and its step count, which equals the dense solve's."""
    poses, fixed, edges, _, _ = reference("ring48")
    g = make_graph(poses, fixed, edges)
    costs, accepted = [], 0
    for _ in range(12):
        rep = g.optimize(pcg_tolerance=1e-10, max_iterations=1)
        if not costs:
            costs.append(rep["initial_cost"])
        assert rep["initial_cost"] == costs[-1]            # a call starts at the cost the last one left
        assert rep["final_cost"] <= rep["initial_cost"]
        assert (rep["final_cost"] < rep["initial_cost"]) == (rep["accepted_steps"] == 1)
        accepted += rep["accepted_steps"]
        costs.append(rep["final_cost"])
        if rep["termination"] != "max_iterations":
            break
    g.close()
    print("ring48, one step per call: chi2 " + " ".join("%.6g" % c for c in costs))
    assert accepted >= 2 and costs[-1] < 1e-2 * costs[0]


def test_an_optimal_graph_takes_no_step():
    gt, _, fixed, edges = gm.drifted_ring(24, 1, seed=5)
    edges = edges.copy()
    edges["z"] = np.stack([gm.between(gt[int(i)], gt[int(j)]) for i, j in zip(edges["i"], edges["j"])])
    g = make_graph(gt, fixed, edges)
    start = g.poses().copy()
    rep = g.optimize(**OPT)
    assert rep["accepted_steps"] == 0 and rep["iterations"] == 0 and rep["termination"] == "gradient" and rep["max_gradient"] <= 1e-9
    assert np.array_equal(g.poses(), start)
    g.close()


def test_a_graph_without_a_free_node_returns_at_once_and_one_without_a_fixed_node_is_refused():
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    g = make_graph(init, np.ones(8, np.int32), edges)
    start = g.poses().copy()
    rep = g.optimize(**OPT)
    assert (rep["iterations"], rep["accepted_steps"], rep["pcg_iterations"], rep["termination"]) == (0, 0, 0, "gradient")
    assert rep["initial_cost"] == rep["final_cost"] > 0.0 and np.array_equal(g.poses(), start)
    g.set_fixed(0, np.zeros(8, np.int32))
    with pytest.raises(api.LiodomError) as err:
        g.optimize(**OPT)
    assert err.value.code == api.ERR_INVALID_ARG and np.array_equal(g.poses(), start)
    g.close()


def test_an_indefinite_information_matrix_breaks_down_and_leaves_the_poses():
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    edges = edges.copy()
    edges["info"] = -gm.OMEGA
    g = make_graph(init, fixed, edges)
    start = g.poses().copy()
    rep = g.optimize(**OPT)
    assert rep["termination"] == "breakdown" and rep["accepted_steps"] == 0
    assert np.array_equal(g.poses(), start)
    g.close()


def test_a_free_node_without_edges_stays():
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    lone = gm.from_axis_angle((1, 2, 3), 0.7, (5.0, 6.0, 7.0))
    poses = np.concatenate([init, lone[None]])
    g = make_graph(poses, np.concatenate([fixed, [0]]), edges)
    start = g.poses().copy()
    y = g.multiply(np.arange(54, dtype=np.float64).reshape(9, 6))
    assert np.array_equal(y[8], np.arange(48, 54, dtype=np.float64))
    rep = g.optimize(**OPT)
    assert rep["termination"] in ("gradient", "cost") and rep["accepted_steps"] >= 1
    assert np.array_equal(g.poses()[8], start[8]) and np.max(np.abs(start[8] - lone)) <= 4e-16
    g.close()


def test_two_runs_on_equal_graphs_return_equal_bytes():
    poses, fixed, edges, _, _ = reference("ring48")
    runs = []
    for _ in range(2):
        g = make_graph(poses, fixed, edges, max_nodes=64, max_edges=80)
        rep = g.optimize(**OPT)
        runs.append((g.poses().tobytes(), rep, [a.tobytes() for a in g.linearize()]))
        g.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]


def test_errors_leave_the_graph_untouched():
    _, init, fixed, edges = gm.drifted_ring(8, 1, seed=2)
    g = make_graph(init, fixed, edges, max_nodes=9, max_edges=9)
    before = (g.poses().copy(), g.edges().copy())

    def refused(code, call):
        with pytest.raises(api.LiodomError) as err:
            call()
        assert err.value.code == code
        assert g.count() == (8, 8) and np.array_equal(g.poses(), before[0]) and g.edges().tobytes() == before[1].tobytes()

    refused(api.ERR_CAPACITY, lambda: g.add_nodes(init[:2]))
    refused(api.ERR_CAPACITY, lambda: g.add_edges(edges[:2]))
    bad = edges[:1].copy(); bad["j"] = 8
    refused(api.ERR_INVALID_ARG, lambda: g.add_edges(bad))
    bad = edges[:1].copy(); bad["j"] = bad["i"]
    refused(api.ERR_INVALID_ARG, lambda: g.add_edges(bad))
    bad = edges[:1].copy(); bad["info"][0, 1, 2] = 1.0
    refused(api.ERR_INVALID_ARG, lambda: g.add_edges(bad))
    bad = edges[:1].copy(); bad["z"][0, 3] += 1e-3
    refused(api.ERR_INVALID_ARG, lambda: g.add_edges(bad))
    bad = edges[:1].copy(); bad["reserved"] = 1
    refused(api.ERR_INVALID_ARG, lambda: g.add_edges(bad))
    nanpose = init[:1].copy(); nanpose[0, 5] = np.nan
    refused(api.ERR_INVALID_ARG, lambda: g.add_nodes(nanpose))
    refused(api.ERR_INVALID_ARG, lambda: g.set_poses(7, init[:2]))
    refused(api.ERR_INVALID_ARG, lambda: g.set_poses(0, nanpose))
    refused(api.ERR_INVALID_ARG, lambda: g.optimize(pcg_tolerance=-1.0))
    assert np.max(np.abs(g.edges()["z"] - gm.normalised(edges["z"]))) <= 4e-16 and np.array_equal(g.edges()["i"], edges["i"])
    g.reset()
    assert g.count() == (0, 0)
    g.close()


# ---------------------------------------------------------------------------------------------
# end to end: the circle (tests/place_model.py) driven once and a fifth around, the loop found and closed
# ---------------------------------------------------------------------------------------------
SITE_SZ, SITE_CELLS = (12.0, 50.0, 0.4), (3, 1)
LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=8, ny=8, nyaw=7), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]


def test_the_loop_of_the_circle_is_found_and_closed(orc, synth):
    import time
    import liodom_amd as la
    import place_model as pm
    from liodom_amd import loop
    run = pm.circle(orc, synth)
    H, W = pm.H, pm.W_SCAN
    gt = np.stack([gm.pose(p[:4], p[4:]) for p in run["gt"]])
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, mapping=1, max_range=pm.MAX_RANGE),
                  la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))
    m = la.Map(*SITE_SZ, max_cells=512, cell_capacity=4096, max_modified_cells=256)
    db = la.Places(max_places=64, max_edges=2048)
    lc = loop.LoopCloser(m, db, LEVELS, min_dist=4.0, min_gap=10, k=2, min_fraction=0.3, max_nodes=128, max_edges=512)
    t0 = time.time()
    odo, key_scans, found = [], [], []
    for k in range(len(run["scans"]) - 1):                      # scans 0 .. 223; the last one is kept for after the re-seed
        pose, info = g.process_scan(run["scans"][k], H, W)
        assert info.status == 0
        pose = gm.compose(gt[0], gm.pose(pose[:4], pose[4:]))   # the odometry starts at the identity
        odo.append(pose)
        edges = g.get_edges()["edges"]
        if k < pm.N_SITE_SCANS:
            m.update(edges, api.pose_T34(pose))                 # the site map: scans 0 .. 187 at the odometry's poses
        r = lc.feed(pose, edges)
        if r["key_frame"]:
            key_scans.append(k)
        found += r["loops"]
    assert m.status() == 0
    n_keys = len(key_scans)
    print("circle: %d key frames, %d places, %d loop edges: %s (%.1f s)" % (n_keys, db.count(), len(found), [(l["place"], l["node"], round(l["fraction"], 2)) for l in found], time.time() - t0))
    assert len(found) >= 1
    for l in found:                                             # a loop edge joins the second lap to the first
        assert key_scans[l["node"]] >= pm.N_SITE_SCANS - 8 and l["node"] - l["place"] >= 10
    gt_keys = gt[key_scans]

    def errors(poses):
        d = np.linalg.norm(np.asarray(poses)[:, 4:] - gt_keys[:, 4:], axis=1)
        return float(np.sqrt(np.mean(d * d))), float(d[-1]), float(np.max(d))

    out = lc.close(handle=g, reader_cells=SITE_CELLS, pcg_tolerance=1e-10, max_iterations=50)
    before, after = errors(out["before"]), errors(out["after"])
    rep = out["report"]
    print("circle: rms %.2f -> %.2f m, last key frame %.2f -> %.2f m, worst %.2f -> %.2f m; %s after %d steps, %d PCG iterations, chi2 %.4g -> %.4g"
          % (before[0], after[0], before[1], after[1], before[2], after[2], rep["termination"], rep["iterations"], rep["pcg_iterations"],
             rep["initial_cost"], rep["final_cost"]))
    assert after[0] < before[0] and after[1] < before[1]
    assert np.max(np.abs(out["before"] - np.stack([odo[k] for k in key_scans]))) <= 4e-16
    # the database's poses are the corrected ones, everything else of it as it was
    st = api.parse_place_state(db.export_state())
    assert st["count"] == n_keys - 10 and np.array_equal(st["poses"], out["after"][:n_keys - 10]) and list(st["ids"]) == list(range(n_keys - 10))
    # the map holds the key frames' clouds and nothing else
    assert m.status() == 0 and 0 < m.all().shape[0] <= sum(c.shape[0] for c in lc.clouds)
    # the stream goes on from the corrected pose, reading the rebuilt map
    assert np.array_equal(api.parse_stream_state(g.export_stream_state(0))["param_t"], out["pose"][4:])
    k = len(run["scans"]) - 1
    pose, info = g.process_scan(run["scans"][k], H, W)
    assert info.status == 0 and info.scan_index == 0
    d_seed, d_odo = np.linalg.norm(out["pose"][4:] - gt[k - 1][4:]), np.linalg.norm(odo[-1][4:] - gt[k - 1][4:])
    print("circle: the pose the stream is seeded with is %.2f m off the truth (the odometry's was %.2f m); the next scan ends %.2f m off"
          % (d_seed, d_odo, np.linalg.norm(pose[4:] - gt[k][4:])))
    g.attach_mapper(None)
    g.close(); m.close(); db.close(); lc.graph.close()


def test_close_refuses_a_place_database_it_does_not_own():
    import liodom_amd as la
    from liodom_amd import loop
    cloud = np.zeros((8, 4), np.float32)
    cloud[:, 0] = np.arange(8) + 3.0
    db = la.Places(max_places=8, max_edges=64)
    db.add(cloud, gm.from_axis_angle((0, 0, 1), 0.0, (50.0, 0.0, 0.0)), id=7)          # somebody else's place
    lc = loop.LoopCloser(None, db, [], min_dist=4.0, min_gap=1, max_nodes=8, max_edges=8)
    for k in range(3):
        assert lc.feed(gm.from_axis_angle((0, 0, 1), 0.0, (5.0 * k, 0.0, 0.0)), cloud)["key_frame"]
    before = (db.export_state(), lc.graph.poses().copy())
    with pytest.raises(ValueError):
        lc.close()
    assert db.export_state() == before[0] and np.array_equal(lc.graph.poses(), before[1])
    lc.graph.close(); db.close()
