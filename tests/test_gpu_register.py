"""liodom_map_register_poses (k_map_local_rows -> k_map_register_grid -> k_map_register) on an MI355X against tests/register_model.py:
the issue's convergence table, designed clouds (tests/designed_register.py), batches, the read-only guarantee on the three kinds
of map, every refusal, and LoopCloser.refine_loop on the real map.

Bounds.  passes, termination, matches, local_points and the correspondences are equal.  The pose is held to 1e-8, the bound
test_gpu_localize.py holds the seeded first scan to (the correspondences are asserted equal, so both sides solve the same
problems; the sums differ in order only).  information is held to 1e-8 of its norm against sum rho' J^T J from the oracle's
autodiff Jacobians, final_cost is bit-equal to the solve's trace and sigma2 = 2 final_cost / (3 C - 6) to 1e-15: the bounds
test_gpu_pose_covariance.py holds the same fields to.  final_cost against the model's: 1e-6 relative — the two poses differ by up
to 1e-8 and the cost's gradient is of the size of the cost over a metre at most."""
import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import designed_register as dr
import localize_model as lm
import register_model as rm
from mapper_lag_common import EPR, H, P, R, W, same

pytestmark = pytest.mark.gpu

CAPS = dict(max_cells=128, cell_capacity=16384)
TIGHT = dict(stop_translation=1e-6, stop_rotation=1e-7)      # the thresholds of the issue's table
SMALL_WS = dict(local_capacity=2048)                          # (the site's rows hold 1609 points)
ERR_INVALID_ARG, ERR_CAPACITY = -1, -3
_SITE = {}


def _site_map(orc, synth, **caps):
    if "blob" not in _SITE:
        m = la.Map(**CAPS)
        for e, T in lm.site_updates(orc, synth):
            m.update(e, T)
        assert same(m.all(), lm.site_map(orc, synth).all()) and m.status() == 0
        _SITE["blob"] = m.export_state()
        m.close()
    m = la.Map(**(caps or CAPS))
    m.import_state(_SITE["blob"])
    return m


def _designed_map(points):
    m = la.Map(**dr.MAP_SIZES, **dr.MAP_CAPS)
    m.update(points)
    assert m.status() == 0
    return m


def _bytes(r):
    keys = sorted(k for k in r if k != "last_lm")
    return b"".join(np.asarray(r[k]).tobytes() for k in keys) + b"".join(np.asarray(r["last_lm"][k]).tobytes() for k in sorted(r["last_lm"]))


def _check(orc, got, want, what, min_range=3.0, max_range=75.0):
    print(what, "termination", got["termination"], "passes", got["passes"], "matches", got["matches"], "moves", got["last_move_t"], got["last_move_r"])
    assert (got["termination"], got["passes"], got["matches"], got["local_points"]) == \
        (want["termination"], want["passes"], want["matches"], want["local_points"]), what
    assert np.array_equal(got["corr"], want["corr"]), (what, int(np.sum(np.any(got["corr"] != want["corr"], axis=1))))
    sign = 1.0 if np.dot(got["pose"][:4], want["pose"][:4]) >= 0 else -1.0
    dq, dt = np.abs(got["pose"][:4] - sign * want["pose"][:4]).max(), np.abs(got["pose"][4:] - want["pose"][4:]).max()
    print(what, "pose difference", dq, dt)
    assert max(dq, dt) <= 1e-8, (what, dq, dt)
    assert got["n_residuals"] == want["n_residuals"], what
    if want["termination"] in (rm.CONVERGED, rm.MAX_PASSES):
        assert abs(got["last_move_t"] - want["last_move_t"]) <= 2e-8 and abs(got["last_move_r"] - want["last_move_r"]) <= 2e-8, what
        assert (got["last_lm"]["termination"], got["last_lm"]["iterations"], got["last_lm"]["accepted"]) == want["last_lm"], what
        Hg, Hr = got["information"], want["information"]
        assert np.array_equal(Hg, Hg.T), what
        print(what, "information difference", np.linalg.norm(Hg - Hr) / np.linalg.norm(Hr), "cost", got["final_cost"], want["final_cost"])
        assert np.linalg.norm(Hg - Hr) <= 1e-8 * np.linalg.norm(Hr), what
        assert np.float64(got["final_cost"]).view(np.uint64) == np.float64(got["last_lm"]["final_cost"]).view(np.uint64), what
        assert abs(got["final_cost"] - want["final_cost"]) <= 1e-6 * want["final_cost"], what
        n = got["n_residuals"]
        assert got["sigma2"] == pytest.approx(2.0 * got["final_cost"] / (3 * n - 6), rel=1e-15), what
        assert got["cov_flags"] == api.COV_VALID, (what, got["cov_flags"])
    else:
        assert np.isnan(got["information"]).all() and np.isnan(got["sigma2"]) and got["final_cost"] == 0.0, what
        assert got["cov_flags"] == (api.COV_EVAL_FAILURE if want["termination"] == rm.EVAL_FAILURE else api.COV_NO_SOLVE), what
        if want["termination"] != rm.EVAL_FAILURE:
            assert got["last_lm"] == dict(iterations=0, accepted=0, termination=0, initial_cost=0.0, final_cost=0.0), what


TABLE = [(0, None), (0, "A"), (0, "B"), (5, None), (5, "A"), (5, "B"), (10, "A")]
STARTS = dict(A=rm.START_A, B=rm.START_B)


def test_the_convergence_table_against_the_model(orc, synth):
    m = _site_map(orc, synth)
    before = m.export_state()
    for scan, name in TABLE:
        want = rm.site_case(orc, synth, scan, STARTS.get(name), **TIGHT)
        got = m.register_poses(want["edges"], [want["start"]], want_corr=True, **TIGHT, **SMALL_WS)[0]
        assert same(m.get_local(api.pose_T34(want["start"]), *lm.CELLS), want["local"])
        _check(orc, got, want, "scan %d from %s" % (scan, name or "the truth"))
    assert rm.site_case(orc, synth, 10, rm.START_A, **TIGHT)["termination"] == rm.MAX_PASSES
    assert m.export_state() == before and m.status() == 0
    m.close()


@pytest.mark.parametrize("max_passes", [1, 2, 10])
def test_pass_counts_against_the_model(orc, synth, max_passes):
    m = _site_map(orc, synth)
    want = rm.site_case(orc, synth, 0, rm.START_A, max_passes=max_passes, **TIGHT)
    got = m.register_poses(want["edges"], [want["start"]], want_corr=True, max_passes=max_passes, **TIGHT, **SMALL_WS)[0]
    _check(orc, got, want, "max_passes %d" % max_passes)
    assert got["passes"] == min(max_passes, 8)
    m.close()


def test_default_workspace_and_default_options(orc, synth):
    """The defaults: 65536 points per row, stops 1e-4 / 1e-5."""
    m = _site_map(orc, synth)
    want = rm.site_case(orc, synth, 5, rm.START_B)
    got = m.register_poses(want["edges"], [want["start"]], want_corr=True)[0]
    _check(orc, got, want, "defaults")
    m.close()


@pytest.mark.parametrize("n_edges", dr.COUNTS)
def test_designed_world_by_edge_count(orc, n_edges):
    w = dr.world()
    m = _designed_map(w["map"])
    edges = w["edges"][:n_edges]
    local = m.get_local(None, 2, 1)
    assert local.shape[0] == w["map"].shape[0]
    want = rm.register(orc, None, edges, dr.IDENTITY, local=local)
    got = m.register_poses(edges, [dr.IDENTITY], want_corr=True, local_capacity=4096)[0]
    _check(orc, got, want, "n_edges %d" % n_edges)
    assert want["termination"] == (rm.FEW_MATCHES if n_edges < 6 else rm.CONVERGED)
    m.close()


def test_designed_neighbourhoods(orc):
    k = dr.knn()
    m = _designed_map(k["map"])
    local = m.get_local(None, 2, 1)
    assert local.shape[0] == k["map"].shape[0]
    want = rm.register(orc, None, k["edges"], dr.IDENTITY, local=local, max_passes=1)
    got = m.register_poses(k["edges"], [dr.IDENTITY], want_corr=True, max_passes=1, local_capacity=4096)[0]
    _check(orc, got, want, "neighbourhoods")
    for name, e in k["special"].items():
        print(name, got["corr"][e])
        if k["expect"][name] is not None:
            assert (got["corr"][e, 0] >= 0) == k["expect"][name], name
    m.close()


@pytest.mark.parametrize("n", [4, 5])
def test_designed_small_maps(orc, n):
    s = dr.small(n)
    m = _designed_map(s["map"])
    local = m.get_local(None, 2, 1)
    assert local.shape[0] == n
    want = rm.register(orc, None, s["edges"], dr.IDENTITY, local=local, min_matches=100)
    got = m.register_poses(s["edges"], [dr.IDENTITY], want_corr=True, min_matches=100, local_capacity=8)[0]
    _check(orc, got, want, "map of %d points" % n)
    assert got["termination"] == rm.FEW_MATCHES and got["matches"] == (0 if n == 4 else 10)
    m.close()


def test_no_map_far_from_the_map(orc):
    w = dr.world()
    m = _designed_map(w["map"])
    want = rm.register(orc, None, w["edges"][:64], dr.FAR, local=np.zeros((0, 4), np.float32))
    got = m.register_poses(w["edges"][:64], [dr.FAR], want_corr=True, local_capacity=4096)[0]
    _check(orc, got, want, "far from the map")
    assert got["termination"] == rm.NO_MAP and got["local_points"] == 0 and (got["corr"] == -1).all()
    m.close()


def _batch_poses(orc, synth, n):
    gt = lm.traversal(orc, synth, 1)[0][2]
    rng = np.random.default_rng(5)
    return np.array([rm.displaced(gt, (rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.005, 0.005, 3))) for _ in range(n)])


def test_batches_rows_and_workspace_growth(orc, synth):
    """n = 1, 5 (the workspace grows), 2, 64 on one map: row i is the one-row call's bytes, a repeated call returns the same bytes."""
    m = _site_map(orc, synth)
    edges = lm.traversal(orc, synth, 1)[0][1]
    poses = _batch_poses(orc, synth, 64)
    single = {}

    def one(i):
        if i not in single:
            single[i] = _bytes(m.register_poses(edges, poses[i:i + 1], want_corr=True, **SMALL_WS)[0])
        return single[i]

    first = one(0)
    for n in (1, 5, 2, 64):
        rows = m.register_poses(edges, poses[:n], want_corr=True, **SMALL_WS)
        again = m.register_poses(edges, poses[:n], want_corr=True, **SMALL_WS)
        assert len(rows) == n
        for i in range(n):
            assert _bytes(rows[i]) == _bytes(again[i]), (n, i)
            assert _bytes(rows[i]) == one(i), (n, i)
    assert one(0) == first
    ends = [r["termination"] for r in m.register_poses(edges, poses, **SMALL_WS)]
    print("terminations of the 64 rows:", np.bincount(ends, minlength=5))
    m.close()


def _handle(mapping=1):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=mapping),
                     la.make_config(n_streams=1, max_points=H * W, max_width=W, recv_capacity=1 << 16))


@pytest.mark.parametrize("kind", ["detached", "reader", "mapper"])
def test_the_map_is_untouched(orc, synth, kind):
    m = _site_map(orc, synth)
    trav = lm.traversal(orc, synth, 1)
    edges, start = trav[3][1], rm.displaced(trav[3][2], rm.START_A)
    ref = _bytes(m.register_poses(edges, [start], want_corr=True, **SMALL_WS)[0]) if kind != "mapper" else None
    g = None
    if kind != "detached":
        g = _handle()
        if kind == "reader":
            g.attach_map_reader(m, *lm.CELLS)
            g.seed_stream(trav[0][2])
        else:
            g.attach_mapper(m, lag=1)
        for x, _, _ in trav[:3]:
            g.process_scan(x, H, W)
    for step in range(2):
        before, status, cells = m.export_state(), m.status(), m.num_cells()
        got = m.register_poses(edges, [start], want_corr=True, **SMALL_WS)
        assert m.export_state() == before and m.status() == status and m.num_cells() == cells, (kind, step)
        assert got[0]["termination"] in (rm.CONVERGED, rm.MAX_PASSES), kind
        if ref is not None:
            assert _bytes(got[0]) == ref, (kind, step)
        if g is not None:
            pose, info = g.process_scan(trav[3 + step][0], H, W)
            assert info.status == 0, (kind, step)
    if g is not None:
        g.attach_mapper(None)
        g.close()
    m.close()


def test_refusals_leave_the_next_call_alone(orc, synth):
    m = _site_map(orc, synth, max_cells=128, cell_capacity=16384, max_update_points=1024)
    edges = lm.traversal(orc, synth, 1)[0][1]
    poses = _batch_poses(orc, synth, 3)
    good = [_bytes(r) for r in m.register_poses(edges, poses, want_corr=True, **SMALL_WS)]
    before = m.export_state()
    bad_q, nan_pose = poses[0].copy(), poses[0].copy()
    bad_q[:4] *= 1.0 + 1e-5
    nan_pose[5] = np.nan
    cases = [
        ("n = 0", dict(poses=np.zeros((0, 7))), ERR_INVALID_ARG),
        ("n = 65", dict(poses=np.repeat(poses[:1], 65, axis=0)), ERR_INVALID_ARG),
        ("more edges than max_update_points", dict(edges=np.zeros((1025, 4), np.float32)), ERR_INVALID_ARG),
        ("NaN pose", dict(poses=[nan_pose]), ERR_INVALID_ARG),
        ("quaternion not normalised", dict(poses=[bad_q]), ERR_INVALID_ARG),
        ("reserved", dict(reserved=1), ERR_INVALID_ARG),
        ("max_passes 0", dict(max_passes=0), ERR_INVALID_ARG),
        ("max_passes 17", dict(max_passes=17), ERR_INVALID_ARG),
        ("negative cells_xy", dict(cells_xy=-1), ERR_INVALID_ARG),
        ("negative cells_z", dict(cells_z=-1), ERR_INVALID_ARG),
        ("negative stop_translation", dict(stop_translation=-1e-9), ERR_INVALID_ARG),
        ("negative stop_rotation", dict(stop_rotation=-1e-9), ERR_INVALID_ARG),
        ("NaN stop_translation", dict(stop_translation=float("nan")), ERR_INVALID_ARG),
        ("negative local_capacity", dict(local_capacity=-1), ERR_INVALID_ARG),
        ("min_matches 0", dict(min_matches=0), ERR_INVALID_ARG),
        ("row larger than local_capacity", dict(local_capacity=1608), ERR_CAPACITY),
    ]
    for what, kw, code in cases:
        kw = dict(SMALL_WS, **kw)
        e, p = kw.pop("edges", edges), kw.pop("poses", poses)
        with pytest.raises(la.LiodomError) as err:
            m.register_poses(e, p, want_corr=True, **kw)
        assert err.value.code == code, (what, err.value.code)
        if code == ERR_CAPACITY:
            assert list(err.value.sizes) == [1609, 1609, 1609], what
        assert [_bytes(r) for r in m.register_poses(edges, poses, want_corr=True, **SMALL_WS)] == good, what
    rows = m.register_poses(np.zeros((0, 4), np.float32), poses, want_corr=True, **SMALL_WS)      # n_edges = 0 is valid
    for r, p in zip(rows, poses):
        assert r["termination"] == rm.FEW_MATCHES and r["passes"] == 0 and np.array_equal(r["pose"], rm.normalised(p))
    assert m.export_state() == before and m.status() == 0
    m.close()


@pytest.mark.parametrize("scan", [0, 5])
def test_refine_loop_measures_z_on_the_real_map(orc, synth, scan):
    """LoopCloser.refine_loop from the truth displaced by start B: the measured Z composed onto the place pose is within 0.03 m of
    the truth in z (the CPU model: 0.021 and 0.001 m), where the searched pose keeps its 0.12 m; with loop_info="solve" the edge's
    information is symmetric and positive definite."""
    from liodom_amd import loop
    m = _site_map(orc, synth)
    _, edges, gt = lm.traversal(orc, synth, 1)[scan]
    place_pose = lm.traversal(orc, synth, 0)[scan][2]
    found = rm.displaced(gt, rm.START_B)
    lc = loop.LoopCloser(m, None, [], graph=object(), refine=dict(TIGHT, min_fraction=0.25, **SMALL_WS), loop_info="solve")
    Z, info, rec = lc.refine_loop(edges, place_pose, found)
    want = rm.site_case(orc, synth, scan, rm.START_B, **TIGHT)
    assert rec["termination"] == want["termination"] == rm.CONVERGED and rec["matches"] == want["matches"]
    X = loop.compose(place_pose, Z)
    print("scan %d: z error searched %.4f, refined %.4f" % (scan, abs(found[6] - gt[6]), abs(X[6] - gt[6])))
    assert abs(found[6] - gt[6]) == pytest.approx(0.12, abs=1e-12) and abs(X[6] - gt[6]) < 0.03
    assert np.abs(X[4:] - rec["pose"][4:]).max() <= 1e-12
    assert np.array_equal(info, info.T) and np.linalg.eigvalsh(info).min() > 0
    B = loop.edge_jacobian_j(place_pose, rec["pose"], Z)
    assert np.abs(B.T @ info @ B - rec["information"] / rec["sigma2"]).max() <= 1e-9 * np.abs(info).max()
    plain = loop.LoopCloser(m, None, [], graph=object(), refine=dict(TIGHT, min_fraction=0.25, **SMALL_WS))
    assert np.array_equal(plain.refine_loop(edges, place_pose, found)[1], loop.LOOP_INFO)
    thin = loop.LoopCloser(m, None, [], graph=object(), refine=dict(TIGHT, min_fraction=0.9, **SMALL_WS))
    assert thin.refine_loop(edges, place_pose, found)[0] is None      # 277 of 684 edges matched: below 0.9
    m.close()


def test_relocalize_with_refine_seeds_the_registered_pose(orc, synth):
    """Liodom.relocalize(refine=...): the searched pose (x, y, yaw of a grid; its z keeps the guess's 0.12 m) is registered and the
    stream is seeded with the registered pose; without refine the call returns what it returned before."""
    m, g = _site_map(orc, synth), _handle()
    x, edges, gt = lm.traversal(orc, synth, 1)[0]      # (the handle's extraction is bit-equal to the oracle's: test_gpu_parity)
    centre = rm.displaced(gt, rm.START_B)
    levels = [dict(step_xy=0.1, step_yaw=0.005, nx=2, ny=2, nyaw=2)]
    plain = g.relocalize(m, x, H, W, centre, levels, min_fraction=0.0)
    assert sorted(plain) == ["fraction", "hits_0", "hits_r", "levels", "n_edges", "pose"]
    assert np.array_equal(api.parse_stream_state(g.export_stream_state(0))["param_t"], plain["pose"][4:])
    r = g.relocalize(m, x, H, W, centre, levels, min_fraction=0.0, refine=dict(TIGHT, **SMALL_WS))
    assert np.array_equal(r["searched_pose"], plain["pose"]) and abs(plain["pose"][6] - gt[6]) == pytest.approx(0.12, abs=1e-12)
    want = rm.register(orc, lm.site_map(orc, synth), edges, plain["pose"], **TIGHT)
    reg = r["registration"]
    print("relocalize: searched z error %.4f, registered %.4f (%d passes, termination %d)" % (abs(plain["pose"][6] - gt[6]), abs(r["pose"][6] - gt[6]), reg["passes"], reg["termination"]))
    assert (reg["termination"], reg["passes"], reg["matches"]) == (want["termination"], want["passes"], want["matches"])
    assert reg["termination"] in (rm.CONVERGED, rm.MAX_PASSES) and np.array_equal(r["pose"], reg["pose"])
    assert np.abs(reg["pose"] - want["pose"]).max() <= 1e-8 and abs(want["pose"][6] - gt[6]) < 0.03
    assert np.array_equal(api.parse_stream_state(g.export_stream_state(0))["param_t"], reg["pose"][4:])
    g.close(); m.close()
