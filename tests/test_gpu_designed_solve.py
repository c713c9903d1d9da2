"""k_lm_solve on the designed problems of tests/designed_solves.py, through liodom_odometry_step alone: every correspondence
count at which the share / wave / register-cache arithmetic changes, designed validity masks, every end of the controller that
four iterations can reach, singular and failed evaluations, both Huber branches — on one-stream handles with 1, 2, 3, 4, 5 and
8 solving workgroups and on a 16-stream lock-step handle (first evaluation inside the solve, Q = 4).

Per case: map frames, liodom_get_local_map, the edges; then, on the GPU's OWN edges, local map and correspondences,
  0. the GPU's valid count and mask are the designed ones (no case passes by being empty);
  1. solve 0: orc.lm_solve from the identity gives the same (termination, iterations, accepted), initial_cost within 1e-12
     relative, final_cost within 1e-9 * max(final_cost, 1e-12)  (test_lm_controller_matches_oracle's bars);
  2. solve 1: the oracle, from its own solve-0 result, on the GPU's pass-1 blocks: same trace, pose within 1e-8 per coordinate
     (test_hostcheck's bar for the chained solve); cases whose normal equations have cond(H) > 1e8 (a condition of the case,
     proved in test_designed_solves.py) are exempt from the coordinate bar and held to 3;
  3. the published pose is the iterate whose cost is reported: orc.cost(pass-1 blocks, returned pose) equals lm[1].final_cost
     to 1e-12 * max(cost, COST_FLOOR), and the newest window frame is orc.transform of the edges by the returned pose to one
     float ulp per coordinate;
  4. (pose_covariance = 1) every entry of `information` within 1e-12 of the float64 sum rho' J^T J at the returned pose, scaled by
     sqrt(H_ii H_jj); n_residuals == C;
  5. a second run on the same handle after liodom_reset is bit-identical; G = 2, 3, 5 against G = 1 under the bars of 1 and 2.

COST_FLOOR = 1e-4.  The relative bar of 3 is the one of scene solves, whose costs are 1e-3 and more.  A designed case with up
to three correspondences is interpolated (final cost 1e-19 .. 1e-27, rounding noise), one with six at a millimetre of noise ends at
1e-7: there the 1.3e-14 m that float64 rounding puts on a residual formed from coordinates at 60 m is 1e-11 of the residual, and
no two correct evaluations agree to 1e-12 relative (the host-compiled controller against the oracle: 5e-12, 7e-12, and 1e-6 .. 4e-2
on the interpolated ones; their absolute differences stay below 2e-18).  Below 1e-4 the bar is therefore the absolute 1e-16.

Run with -m gpu on an MI355X; -s prints the worst difference per check."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd.api import COV_EVAL_FAILURE
import designed_solves as ds

pytestmark = pytest.mark.gpu

IC_REL, FC_REL, FC_FLOOR = 1e-12, 1e-9, 1e-12
POSE_TOL = 1e-8
COST3_REL, COST_FLOOR = 1e-12, 1e-4
H_TOL = 1e-12
SEQ_TOL_T = SEQ_TOL_R = 1e-4
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])

# handle -> (shape, streams, lm_workgroups, lm_apply_step_on_ftol, pose_covariance, modes to assert)
HANDLES = {
    "g1": (ds.SMALL, 1, 1, 0, 0, {"lm_groups": "1", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g2": (ds.SMALL, 1, 2, 0, 0, {"lm_groups": "2", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g3": (ds.SMALL, 1, 3, 0, 0, {"lm_groups": "3", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g4_ftol": (ds.SMALL, 1, 4, 1, 0, {"lm_groups": "4", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g5": (ds.SMALL, 1, 5, 0, 0, {"lm_groups": "5", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g8_cov": (ds.SMALL, 1, 8, 0, 1, {"lm_groups": "8", "n_streams": "1", "knn_instance": "256", "knn_partials": "1"}),
    "g8_alone": (ds.SMALL, 1, 8, 0, 0, {"lm_groups": "8", "n_streams": "1", "knn_instance": "256", "knn_partials": "1", "knn_overlap": "1"}),
    "big": (ds.BIG, 1, 0, 0, 0, {"lm_groups": "8", "n_streams": "1", "knn_instance": "256", "knn_partials": "1", "knn_queries": "8"}),
    "s16": (ds.SMALL, 16, 0, 0, 0, {"lm_groups": "1", "n_streams": "16", "knn_instance": "128", "knn_partials": "0", "knn_queries": "4"}),
}
SMALL_CASES = [n for n, c in ds.CASES.items() if c.shape == ds.SMALL]
LOCKSTEP_CASES = ["t_nores", "c1", "c2", "c63", "c64", "c65", "c256", "c257", "c1056", "s5", "s513", "s129",
                  "t_gtol_0_0_s1", "t_maxit_4_1", "dup", "huber32"]
STALE_COUNTS = ds.STALE_COUNTS

_handles = {}
_oracle_runs = {}
_results = {}
_worst = {}


def note(check, value, where):
    if check not in _worst or value > _worst[check][0]:
        _worst[check] = (float(value), where)


def open_handle(name):
    if name not in _handles:
        shape, S, G, apply_ftol, cov, want = HANDLES[name]
        h, r, epr = shape
        g = la.Liodom(la.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=ds.PREV_FRAMES),
                      la.make_config(n_streams=S, max_points=h * 1024, max_width=1024, lm_workgroups=G, lm_apply_step_on_ftol=apply_ftol,
                                     pose_covariance=cov))
        modes = g.modes()
        assert {k: modes[k] for k in want} == want, (name, modes)
        _handles[name] = g
    g = _handles[name]
    g.reset()
    return g


def close_handles():
    for g in _handles.values():
        g.close()
    _handles.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    close_handles()
    print("\n  designed solves, worst GPU - oracle difference per check:")
    for check in sorted(_worst):
        print("    %-34s %.3g   (%s)" % (check, _worst[check][0], _worst[check][1]))


def oracle_of(orc, name, apply_ftol):
    """The oracle's own run of the case (its counts and traces: the pinned ones when lm_apply_step_on_ftol = 0)."""
    key = (name, apply_ftol)
    if key not in _oracle_runs:
        case = ds.CASES[name]
        if apply_ftol:
            case = ds.Case(**{**case.__dict__, "apply_on_ftol": 1})
        r = ds.oracle_run(orc, case)
        if not apply_ftol:
            assert (r["matches"], r["traces"][0], r["traces"][1]) == ds.TRACES[name], name
        _oracle_runs[key] = r
    return _oracle_runs[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def ulp_distance(a, b):
    """Largest distance in float32 steps between two arrays (ordered-integer view; +0 and -0 coincide)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.max(np.abs(key(a) - key(b)))) if a.size else 0


def quat_diff(qa, qb):
    return float(min(np.abs(qa - qb).max(), np.abs(qa + qb).max()))


def feed(g, built, stream, what):
    """Map frames, the local map (must be the designed map bit for bit), the edges.  Returns what the GPU holds and reports."""
    for f in built["frames"]:
        pose, info = g.odometry_step(f, stream=stream)
        assert info.status == 0 and np.array_equal(pose, IDENT), (what, info.status, pose)
    lmap = g.local_map(stream)[0]
    assert same_bits(lmap, built["map"]), what
    return lmap


def step_and_collect(g, edges, stream, what):
    pose, info = g.odometry_step(edges, stream=stream)
    assert info.status == 0, (what, info.status)
    corr = [g.correspondences(it, stream=stream) for it in (0, 1)]
    ed = g.get_edges(stream)["edges"]
    assert same_bits(ed, edges), what
    win, _ = g.window(stream)
    return dict(pose=pose.copy(), info=info, corr=corr, edges=ed, window=win)


def info_bits(info):
    return C.string_at(C.addressof(info), C.sizeof(info))


def check_published_pose(orc, got, lmap, blocks1, what, tag):
    """Check 3 on one step: the cost of the returned pose on the pass-1 blocks is the reported final cost, and the appended
    frame is the edges under the returned pose."""
    pose, info, ed = got["pose"], got["info"], got["edges"]
    fc = info.lm[1].final_cost
    if len(blocks1) == 0:
        assert fc == 0.0, (what, fc)
    else:
        want = orc.cost(blocks1, pose[:4], pose[4:])
        if info.lm[1].termination == 5:
            assert not np.isfinite(want), what           # (a zero-length line: no cost exists at any pose)
        else:
            scale = max(want, COST_FLOOR)
            note("3 cost at the returned pose " + tag, abs(want - fc) / scale, what)
            assert abs(want - fc) <= COST3_REL * scale, (what, want, fc)
    win = got["window"]
    assert len(win) == len(lmap) + len(ed), (what, len(win), len(lmap), len(ed))
    assert same_bits(win[:len(lmap)], lmap), what
    T, _ = orc.pose_ops(pose[:4], pose[4:])
    ref = orc.transform(T, ed)
    newest = win[len(lmap):]
    d = ulp_distance(newest[:, :3], ref[:, :3])
    note("3 window frame, float ulps " + tag, d, what)
    assert d <= 1 and same_bits(newest[:, 3], ref[:, 3]), (what, d)


def h_error(orc, blocks, pose, Hd):
    Hr, _ = ds.normal_matrix(orc, blocks, pose[:4], pose[4:])
    dg = np.clip(np.diag(Hr), 0.0, None)
    scale = np.sqrt(np.outer(dg, dg))
    top = float(dg.max()) if dg.max() > 0 else 1.0
    scale = np.where(scale > 0, scale, top)              # (an entry whose row or column is exactly empty: against the largest)
    return float(np.max(np.abs(Hd - Hr) / scale))


def check_case(orc, g, hname, name, stream=0):
    """Checks 0 - 4 of one case on one handle (which the caller has reset or left with an unused stream)."""
    case = ds.CASES[name]
    _, _, _, apply_ftol, cov, _ = HANDLES[hname]
    what = "%s %s stream %d" % (hname, name, stream)
    exp = oracle_of(orc, name, apply_ftol)
    built = exp["built"]
    lmap = feed(g, built, stream, what)
    got = step_and_collect(g, built["edges"], stream, what)
    info, pose = got["info"], got["pose"]
    # 0. not empty: the designed mask, the stated counts
    v0, v1 = got["corr"][0][0], got["corr"][1][0]
    assert np.array_equal(v0.astype(bool), built["valid"]), (what, int(v0.sum()), case.C)
    assert [int(v0.sum()), int(v1.sum())] == exp["matches"] == list(info.matches) and int(v0.sum()) == case.C, (what, list(info.matches))
    blocks = [ds.blocks_of(got["edges"], lmap, *got["corr"][it]) for it in (0, 1)]
    # 1. solve 0 on identical inputs
    q0, t0, tr0 = orc.lm_solve(blocks[0], IDENT[:4], IDENT[4:], apply_on_ftol=apply_ftol)
    assert ds.trace_of(info.lm[0]) == ds.trace_of(tr0) == exp["traces"][0], (what, ds.trace_of(info.lm[0]), ds.trace_of(tr0))
    if tr0.termination in (4, 5):
        assert info.lm[0].initial_cost == tr0.initial_cost and info.lm[0].final_cost == tr0.final_cost, what
    else:
        ic, fc = info.lm[0].initial_cost, info.lm[0].final_cost
        note("1 initial cost, relative", abs(ic - tr0.initial_cost) / tr0.initial_cost, what)
        note("1 final cost / max(cost, 1e-12)", abs(fc - tr0.final_cost) / max(tr0.final_cost, FC_FLOOR), what)
        assert abs(ic - tr0.initial_cost) <= IC_REL * tr0.initial_cost, (what, ic, tr0.initial_cost)
        assert abs(fc - tr0.final_cost) <= FC_REL * max(tr0.final_cost, FC_FLOOR), (what, fc, tr0.final_cost)
    # 2. solve 1: the oracle from its own solve-0 result on the GPU's pass-1 blocks
    q1, t1, tr1 = orc.lm_solve(blocks[1], q0, t0, apply_on_ftol=apply_ftol)
    assert ds.trace_of(info.lm[1]) == ds.trace_of(tr1) == exp["traces"][1], (what, ds.trace_of(info.lm[1]), ds.trace_of(tr1))
    dq, dt = quat_diff(pose[:4], q1), float(np.abs(pose[4:] - t1).max())
    if not case.rank:
        note("2 pose, quaternion", dq, what)
        note("2 pose, translation [m]", dt, what)
        assert dq <= POSE_TOL and dt <= POSE_TOL, (what, dq, dt)
    else:
        note("2 pose of rank cases (no bar)", max(dq, dt), what)
    # 3. the published pose
    check_published_pose(orc, got, lmap, blocks[1], what, "")
    # 4. the information matrix
    if cov:
        rec = g.wait_pose_covariance(stream, info.scan_index)
        assert rec["n_residuals"] == exp["matches"][1] and rec["termination"] == info.lm[1].termination, what
        if info.lm[1].termination == 5:
            assert rec["flags"] == COV_EVAL_FAILURE, (what, rec["flags"])
        else:
            err = h_error(orc, blocks[1], pose, rec["information"])
            note("4 information matrix, scaled", err, what)
            assert err <= H_TOL, (what, err)
    return dict(pose=pose, info_bits=info_bits(info), traces=[ds.trace_of(info.lm[0]), ds.trace_of(info.lm[1])],
                costs=[(info.lm[i].initial_cost, info.lm[i].final_cost) for i in (0, 1)], window=got["window"])


def result_of(orc, hname, name):
    """Checks 0 - 4, then the same case again on the same handle after liodom_reset: bit-identical (5)."""
    key = (hname, name)
    if key not in _results:
        a = check_case(orc, open_handle(hname), hname, name)
        b = check_case(orc, open_handle(hname), hname, name)
        assert np.array_equal(a["pose"].view(np.uint64), b["pose"].view(np.uint64)) and a["info_bits"] == b["info_bits"], (hname, name)
        assert same_bits(a["window"], b["window"]), (hname, name)
        _results[key] = a
    return _results[key]


@pytest.mark.parametrize("name", SMALL_CASES)
@pytest.mark.parametrize("hname", ["g1", "g2", "g3", "g4_ftol", "g5", "g8_cov"])
def test_designed_case(orc, hname, name):
    result_of(orc, hname, name)


def test_apply_on_ftol_cases_return_the_candidate(orc):
    """lm_apply_step_on_ftol = 1: some designed cases end by function tolerance after a step (the candidate is applied without
    being accepted) and must return that candidate, others end without one; both kinds exist among the cases."""
    kinds = set()
    for name in SMALL_CASES:
        r1, r0 = oracle_of(orc, name, 1), oracle_of(orc, name, 0)
        if r1["traces"][1][0] == 2 and r1["traces"][1][1] >= 1:
            kinds.add("ftol")
            if not np.array_equal(r1["pose"], r0["pose"]):
                kinds.add("moved")
    assert kinds == {"ftol", "moved"}


@pytest.mark.parametrize("name", SMALL_CASES)
def test_workgroup_counts_agree(orc, name):
    """5.: G = 2, 3, 5 against G = 1 under the bars of 1 and 2 (the order of summation differs: not bit for bit)."""
    case = ds.CASES[name]
    ref = result_of(orc, "g1", name)
    for hname in ("g2", "g3", "g5"):
        r = result_of(orc, hname, name)
        assert r["traces"] == ref["traces"], (hname, name)
        for it in (0, 1):
            (ic, fc), (ic1, fc1) = r["costs"][it], ref["costs"][it]
            if ref["traces"][it][0] in (4, 5):
                assert (ic, fc) == (ic1, fc1) or not (np.isfinite(ic1) and np.isfinite(fc1)), (hname, name)
                continue
            if it == 0:
                note("5 initial cost G vs G = 1, relative", abs(ic - ic1) / ic1, "%s %s" % (hname, name))
                assert abs(ic - ic1) <= IC_REL * ic1, (hname, name, ic, ic1)
            assert abs(fc - fc1) <= FC_REL * max(fc1, FC_FLOOR), (hname, name, fc, fc1)
        dq, dt = quat_diff(r["pose"][:4], ref["pose"][:4]), float(np.abs(r["pose"][4:] - ref["pose"][4:]).max())
        if not case.rank:
            note("5 pose G vs G = 1", max(dq, dt), "%s %s" % (hname, name))
            assert dq <= POSE_TOL and dt <= POSE_TOL, (hname, name, dq, dt)


def test_second_round_of_the_mask_compaction(orc):
    """E = 2100 on the 8704-edge shape: 263 k_knn workgroups, 66 mask words (lm_compact_bits' second round of 64), eight of the
    72 valid edges in the 257th workgroup."""
    case = ds.CASES["big_sparse"]
    assert case.E > 2048 and ((case.E + 7) // 8 + 3) // 4 > 64
    assert int(ds.build(case)["valid"][2048:2056].sum()) == 8
    result_of(orc, "big", "big_sparse")


def test_lockstep_streams_side_by_side(orc):
    """Sixteen streams of a lock-step handle hold sixteen different cases at once (knn_partials = 0: the first evaluation happens
    inside the solve; Q = 4: bit 3 is the top bit of a mask byte); each against its own oracle, checks 0 - 3."""
    assert len(LOCKSTEP_CASES) == 16
    g = open_handle("s16")
    builts = {s: oracle_of(orc, name, 0)["built"] for s, name in enumerate(LOCKSTEP_CASES)}
    for k in range(max(len(b["frames"]) for b in builts.values())):        # the maps grow side by side
        for s, b in builts.items():
            if k < len(b["frames"]):
                pose, info = g.odometry_step(b["frames"][k], stream=s)
                assert info.status == 0 and np.array_equal(pose, IDENT), (s, k)
    lmaps = {s: g.local_map(s)[0] for s in builts}
    gots = {s: step_and_collect(g, builts[s]["edges"], s, "s16 %s" % LOCKSTEP_CASES[s]) for s in builts}
    for s, name in enumerate(LOCKSTEP_CASES):
        case, exp, got, what = ds.CASES[name], oracle_of(orc, name, 0), gots[s], "s16 %s stream %d" % (name, s)
        assert same_bits(lmaps[s], builts[s]["map"]), what
        info, pose = got["info"], got["pose"]
        v0, v1 = got["corr"][0][0], got["corr"][1][0]
        assert np.array_equal(v0.astype(bool), builts[s]["valid"]), what
        assert [int(v0.sum()), int(v1.sum())] == exp["matches"] == list(info.matches) and int(v0.sum()) == case.C, (what, list(info.matches))
        blocks = [ds.blocks_of(got["edges"], lmaps[s], *got["corr"][it]) for it in (0, 1)]
        q0, t0, tr0 = orc.lm_solve(blocks[0], IDENT[:4], IDENT[4:])
        assert ds.trace_of(info.lm[0]) == ds.trace_of(tr0) == exp["traces"][0], (what, ds.trace_of(info.lm[0]))
        if tr0.termination in (4, 5):
            assert info.lm[0].initial_cost == tr0.initial_cost and info.lm[0].final_cost == tr0.final_cost, what
        else:
            ic, fc = info.lm[0].initial_cost, info.lm[0].final_cost
            note("1 initial cost, relative (lock-step)", abs(ic - tr0.initial_cost) / tr0.initial_cost, what)
            assert abs(ic - tr0.initial_cost) <= IC_REL * tr0.initial_cost, (what, ic, tr0.initial_cost)
            assert abs(fc - tr0.final_cost) <= FC_REL * max(tr0.final_cost, FC_FLOOR), (what, fc, tr0.final_cost)
        q1, t1, tr1 = orc.lm_solve(blocks[1], q0, t0)
        assert ds.trace_of(info.lm[1]) == ds.trace_of(tr1) == exp["traces"][1], (what, ds.trace_of(info.lm[1]))
        if not case.rank:
            dq, dt = quat_diff(pose[:4], q1), float(np.abs(pose[4:] - t1).max())
            note("2 pose (lock-step)", max(dq, dt), what)
            assert dq <= POSE_TOL and dt <= POSE_TOL, (what, dq, dt)
        check_published_pose(orc, got, lmaps[s], blocks[1], what, "(lock-step)")


@pytest.mark.parametrize("hname", ["g1", "g3", "g8_cov", "s16", "g8_alone"])
def test_stale_rows_and_mask_bytes(orc, hname):
    """One handle, no reset between scans: matches and traces equal the oracle's odometer fed the same steps, pose within 1e-4,
    check 3 (and 4) on every scan.  On the lock-step handle the sequence runs on stream 9.  g8_alone: no other live handle, so
    the second kNN pass of a scan runs beside its first solve (knn_overlap = 1, asserted) and that solve hands its result over
    inside the launch — every other handle of this file shares the GPU with its neighbours and runs the passes in turn."""
    if hname == "g8_alone":
        close_handles()
    g = open_handle(hname)
    stream = 9 if hname == "s16" else 0
    cov = HANDLES[hname][4]
    steps = ds.stale_steps()
    od = orc.Odometer(ds.oracle_params(orc, ds.CASES["c1056"]))
    lmap = feed(g, steps[0], stream, hname)
    for f in steps[0]["frames"]:
        od.step(f)
    for k, b in enumerate(steps):
        what = "%s stale scan %d (C = %d)" % (hname, k, STALE_COUNTS[k])
        if k:
            lmap = g.local_map(stream)[0]
        got = step_and_collect(g, b["edges"], stream, what)
        pose_o, info_o = od.step(b["edges"])
        info, pose = got["info"], got["pose"]
        v = [got["corr"][it][0] for it in (0, 1)]
        assert np.array_equal(v[0].astype(bool), b["valid"]) and np.array_equal(v[1].astype(bool), b["valid"]), what
        assert list(info.matches) == list(info_o.matches) == [STALE_COUNTS[k]] * 2, (what, list(info.matches), list(info_o.matches))
        assert [ds.trace_of(info.lm[i]) for i in (0, 1)] == [ds.trace_of(info_o.lm[i]) for i in (0, 1)], what
        dt, dr = float(np.linalg.norm(pose[4:] - pose_o[4:])), 2.0 * quat_diff(pose[:4], pose_o[:4])
        note("stale sequence: pose vs the oracle's odometer", max(dt, dr), what)
        assert dt <= SEQ_TOL_T and dr <= SEQ_TOL_R, (what, dt, dr)
        blocks1 = ds.blocks_of(got["edges"], lmap, *got["corr"][1])
        check_published_pose(orc, got, lmap, blocks1, what, "(stale sequence)")
        if cov:
            rec = g.wait_pose_covariance(stream, info.scan_index)
            assert rec["n_residuals"] == STALE_COUNTS[k], what
            err = h_error(orc, blocks1, pose, rec["information"])
            note("4 information matrix, scaled (stale sequence)", err, what)
            assert err <= H_TOL, (what, err)
    od.close()
    if hname == "g8_alone":
        close_handles()
