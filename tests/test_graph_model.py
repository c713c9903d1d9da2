"""The pose graph's NumPy restatement (tests/graph_model.py) against what does not depend on it: its analytic Jacobians against
central differences, its dense Levenberg-Marquardt on a drifted ring, and the correction of the CPU oracle's drift on the project's
circle with ideal loop edges.  No GPU, no library call."""
import math

import numpy as np
import pytest

import graph_model as gm
import place_model as pm


@pytest.mark.parametrize("name,Xi,Xj,Z", gm.jacobian_cases(), ids=[c[0] for c in gm.jacobian_cases()])
def test_the_jacobians_are_the_derivatives(name, Xi, Xj, Z):
    """Central differences at h = 1e-6: truncation ~ h^2, rounding ~ eps / h * scale; the bound 1e-7 * scale is three decades above
    both."""
    e, A, B = gm.edge_jacobians(Xi, Xj, Z)
    An, Bn = gm.numeric_jacobians(Xi, Xj, Z, 1e-6)
    bound = 1e-7 * gm.edge_scale(Xi, Xj, Z)
    worst = max(float(np.max(np.abs(A - An))), float(np.max(np.abs(B - Bn))))
    print("%s: worst |analytic - numeric| %.3g, bound %.3g" % (name, worst, bound))
    assert worst <= bound
    if "w_negative" in name:
        assert gm.compose(gm.inverse(Z), gm.between(Xi, Xj))[3] < 0.0
    if "zero_error" in name:
        assert np.max(np.abs(e)) <= 1e-15 * gm.edge_scale(Xi, Xj, Z) * 10


def test_the_error_is_the_half_angle_and_the_offset():
    Xi = gm.from_axis_angle((0, 0, 1), 0.3, (1.0, 2.0, 3.0))
    d = gm.from_axis_angle((0, 1, 0), 0.2, (0.5, -0.25, 0.125))
    Xj = gm.compose(Xi, d)
    e = gm.edge_error(Xi, Xj, gm.pose([0, 0, 0, 1], [0, 0, 0]))
    assert np.allclose(e, [0.0, math.sin(0.1), 0.0, 0.5, -0.25, 0.125], rtol=0, atol=1e-15)
    assert np.allclose(gm.edge_error(Xi, Xj, d), 0.0, rtol=0, atol=1e-15)


def test_the_dense_lm_converges_on_the_drifted_ring():
    gt, init, fixed, edges = gm.drifted_ring(48, 1, seed=3)
    out, rep = gm.lm(init, fixed, edges, max_iterations=50)
    assert rep["termination"] in ("gradient", "cost") and rep["accepted_steps"] >= 2
    assert rep["final_cost"] < 1e-2 * rep["initial_cost"]
    assert all(b <= a for a, b in zip(rep["costs"], rep["costs"][1:]))
    assert abs(gm.chi2(out, edges) - rep["final_cost"]) <= 1e-12 * rep["final_cost"]
    before = np.sqrt(np.mean(np.sum((init[:, 4:] - gt[:, 4:]) ** 2, axis=1)))
    after = np.sqrt(np.mean(np.sum((out[:, 4:] - gt[:, 4:]) ** 2, axis=1)))
    print("ring of 48: rms %.3f m -> %.3f m, %d steps" % (before, after, rep["iterations"]))
    assert after < before
    assert np.array_equal(out[0], gm.normalised(init)[0])          # the fixed node
    # the solution is a stationary point of the dense problem: a second run from it takes no step
    _, again = gm.lm(out, fixed, edges, max_iterations=50, gradient_tolerance=1e-6)
    assert again["accepted_steps"] == 0 and again["termination"] == "gradient"


def test_multiply_is_the_dense_product():
    poses, fixed, edges = gm.chain(9, seed=5)
    fixed[4] = 1
    lin = gm.linearize(poses, fixed, edges)
    Hm, g = gm.dense(lin, edges)
    rng = np.random.default_rng(2)
    x = rng.normal(size=(9, 6))
    free = np.repeat(fixed == 0, 6)
    for lam in (0.0, 1.0):
        y, y_abs = gm.multiply(lin, fixed, edges, x, lam)
        Hd = Hm + lam * np.diag(np.diag(Hm))
        want = np.zeros(54)
        want[free] = Hd[np.ix_(free, free)] @ x.reshape(-1)[free]
        assert np.max(np.abs(y.reshape(-1) - want)) <= 1e-12 * np.max(y_abs)
        assert np.all(y[fixed != 0] == 0.0)


def circle_graph(orc, synth, step=4):
    """The CPU oracle's odometry over the project's circle as a graph: key frames every `step` scans, odometry edges from the
    oracle's poses, ideal loop edges from the key frames of the second lap to those one lap (188 scans) earlier, node 0 fixed ->
    (gt [K, 7], init [K, 7], fixed, edges)."""
    run = pm.circle(orc, synth)
    po = pm.circle_params(orc)
    od = orc.Odometer(po)
    odo = []
    for k in range(len(run["edges"])):
        p, _ = od.step(run["edges"][k])
        odo.append(gm.compose(gm.pose(run["gt"][0][:4], run["gt"][0][4:]), gm.pose(p[:4], p[4:])))
    keys = list(range(0, len(odo), step))
    gt = np.stack([gm.pose(run["gt"][k][:4], run["gt"][k][4:]) for k in keys])
    init = np.stack([odo[k] for k in keys])
    ii, jj, zs, kinds = [], [], [], []
    for a in range(len(keys) - 1):
        ii.append(a); jj.append(a + 1); zs.append(gm.between(init[a], init[a + 1])); kinds.append(0)
    for a, k in enumerate(keys):
        if k >= pm.N_SITE_SCANS:
            b = keys.index(k - pm.N_SITE_SCANS)
            ii.append(b); jj.append(a); zs.append(gm.between(gt[b], gt[a])); kinds.append(1)
    edges = gm.api.graph_edges(ii, jj, np.stack(zs), gm.OMEGA)
    edges["kind"] = kinds
    fixed = np.zeros(len(keys), np.int32)
    fixed[0] = 1
    return gt, init, fixed, edges


def translation_errors(poses, gt):
    d = np.linalg.norm(np.asarray(poses)[:, 4:] - gt[:, 4:], axis=1)
    return float(np.sqrt(np.mean(d * d))), float(d[-1]), float(np.max(d))


def test_ideal_loop_edges_correct_the_oracles_drift_on_the_circle(orc, synth):
    gt, init, fixed, edges = circle_graph(orc, synth)
    assert int(np.sum(edges["kind"] == 1)) == 10
    before = translation_errors(init, gt)
    out, rep = gm.lm(init, fixed, edges, max_iterations=50)
    after = translation_errors(out, gt)
    print("circle: rms %.2f -> %.2f m, last key frame %.2f -> %.2f m, worst %.2f -> %.2f m, %d LM iterations (%s)"
          % (before[0], after[0], before[1], after[1], before[2], after[2], rep["iterations"], rep["termination"]))
    assert after[0] < before[0] and after[1] < before[1]
