"""The pose chain between the solves on the designed states of tests/designed_poses.py, CPU only.

  conditions   every case reaches the decision it is aimed at, shown on the float64 restatement (designed_poses.Chain): the
               gimbal branch, the quaternion case, the side of the trace, the tie.
  reference    the same formulas in mpmath at 50 digits, along the float64 run's decisions.  The oracle's own Odometer.step()
               from the designed state and the host-compiled header (tests/hostcheck.cc) are held to it on every case:
                 bar = BASE * scans * growth / cond,   BASE = 1e-13 (test_hostcheck.py's bar for the same functions),
               rotation entries absolute, translations relative to the largest translation of the case.
                 cond    getRPY forms its angles as atan2(y, x) of matrix entries that carry an absolute rounding error of a few
                         1e-16; the angle error is that over hypot(y, x), and hypot(y, x) = cos(pitch) outside the lock branch.
                         cond = the smallest hypot of the case (1 when it is exactly 0: atan2(0, 0) = 0 is exact).
                 growth  pose_rotation_mode 0 without the override multiplies an orthonormality defect per round trip
                          and a rounding error is such a defect: growth = the largest defect the 50-digit run
                         itself shows over the scans, over its first.  1 otherwise.
               The distance found (designed_poses.yardstick) is what the device's bars are measured in (test_gpu_designed_pose.py).
  oracle step  a step from a designed state with no match equals the composition of the oracle's free functions, bit for bit.
  mutants      transcriptions of the rules a wrong kernel would follow disagree with the oracle on the family aimed at them.
"""
import math

import numpy as np
import pytest

import designed_poses as dp

BASE = 1e-13
NAMES = list(dp.CASES)


@pytest.fixture(scope="module")
def hc():
    return dp.hostcheck_lib()


def in_range(v, lo_hi):
    return lo_hi[0] <= v <= lo_hi[1]


def test_the_edges_cannot_match():
    """A correspondence needs five window points within 1 m (d[4] < 1.0, laser_odometry.cc:324).  The edges are more than 2 m
    apart, so a ball of radius 1 m holds at most one point of a frame — rigid poses keep distances — and a window of three frames
    offers at most three; the far frame is kilometres from every designed translation."""
    e = dp.edges64()[:, :3].astype(np.float64)
    d = np.linalg.norm(e[:, None] - e[None], axis=2) + 1e9 * np.eye(64)
    assert d.min() > 2.0 and dp.PREV_FRAMES * 1 < 5
    reach = max(float(np.abs(c.odom[:, 3]).max()) for c in dp.CASES.values()) + 3.0 * dp.SCANS_CHAIN + 30.0
    assert np.linalg.norm(dp.FAR) - np.abs(e).max() * 2 > 2 * reach
    r = np.linalg.norm(e[:, :2], axis=1)
    assert r.min() >= 6.0 and r.max() <= 24.0


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    case = dp.CASES[name]
    res, trace, notes = dp.float_run(name)
    sites = {label for label, _, _ in trace}
    assert {"pose.quat", "pred.quat"} <= sites and (("imu.rpy" in sites and "new.tfquat" in sites) == bool(case.use_imu))
    for key, want in case.aim.items():
        site, _, what = key.partition(".")
        if what in ("quat", "tfquat", "rpy"):
            got = dp.decisions(trace, key)[0]
            assert got == want, (name, key, got)
        elif what == "trace":
            assert dp.facts(trace, site + ".quat")[0]["trace"] == want, (name, dp.facts(trace, site + ".quat")[0])
        elif what == "trace_ulps":
            k = dp.facts(trace, site + ".quat")[0]["trace"] / dp.EPS
            assert k == int(k) and in_range(k, want), (name, k)
        elif what == "tie":
            assert dp.facts(trace, site + ".quat")[0]["tie"] is want, name
        elif what == "m6":
            assert dp.facts(trace, site + ".rpy")[0]["m6"] == want, name
        elif what == "m6_ulps":
            k = (1.0 - abs(dp.facts(trace, site + ".rpy")[0]["m6"])) / dp.ULP1
            assert k == int(k) and in_range(k, want), (name, k)
        elif what in ("roll", "yaw"):          # the signed angle, to the bit (+pi and -pi are the two sides of atan2's cut)
            angle = notes[site + ".rpy"]["rpy".index(what[0])]
            assert angle == want and math.copysign(1.0, angle) == math.copysign(1.0, want), (name, angle.hex())
        elif what in ("pitch_gap", "roll_gap", "yaw_gap"):
            angle = abs(notes[site + ".rpy"]["rpy".index(what[0])])
            assert in_range((math.pi / 2 if what[0] == "p" else math.pi) - angle, want), (name, angle)
        elif key == "eps":
            A = case.odom[:, :3]
            defect = float(np.abs(dp.mm3(A.T, A) - np.eye(3)).max())
            assert 0.3 * want <= defect <= 3.0 * want, (name, defect)
            nq = abs(float(np.linalg.norm(res[0]["pose"][:4])) - 1.0)
            if case.mode == 1:
                assert nq <= 1e-15, (name, nq)
            elif want >= 1e-9 and not case.use_imu:
                assert nq >= 0.01 * want, (name, nq)      # linear() went through untouched: the quaternion is not a unit one
        elif key == "step":
            rel = dp.compose(np.array(dp.Chain().iso_inverse(list(case.prev_odom.reshape(12)))).reshape(3, 4), case.odom)
            angle = math.acos((np.trace(rel[:, :3]) - 1) / 2)
            assert abs(np.linalg.norm(rel[:, 3]) - want[0]) < 1e-6 and abs(angle - want[1]) < 1e-4, (name, rel)
            assert float(np.abs(case.odom[:, 3]).max()) >= 1.0e4
        elif key in ("same_as", "close_to"):
            assert want in dp.CASES
        else:
            raise AssertionError("unknown aim %r" % key)
    if case.family == "chain":
        # a full turn about z: the returned quaternion passes the 'pos' and the 'z' case (tf's getRotation too, with the override),
        # and mode 0 shows the growth
        for site in ("pose.quat", "pred.quat") + (("new.tfquat",) if case.use_imu else ()):
            assert set(dp.decisions(trace, site)) == {"pos", "z"}, (name, site)
        defect = [float(np.abs(dp.mm3(r["final"].reshape(3, 4)[:, :3].T, r["final"].reshape(3, 4)[:, :3]) - np.eye(3)).max()) for r in res]
        if case.mode == 0 and not case.use_imu:
            assert defect[0] < 1e-10 and defect[7] < 1e-10 and 1e-7 < defect[15] < 1e-6 and 1e-4 < max(defect) < 1e-2, (name, defect[0], max(defect))
        else:
            assert max(defect) < 2e-15, (name, max(defect))


def test_every_branch_is_reached_by_some_case():
    got = {}
    for name in NAMES:
        for label, value, f in dp.float_run(name)[1]:
            got.setdefault(label.split(".")[1], set()).add(value)
            if f.get("tie"):
                got.setdefault("tie", set()).add(value)
    assert got["quat"] == {"pos", "x", "y", "z"} and got["tfquat"] == {"pos", "x", "y", "z"}
    assert got["rpy"] == {"free", "lock+", "lock-"}
    assert {"x", "y"} <= got["tie"]
    sites = {(label, value) for name in NAMES for label, value, _ in dp.float_run(name)[1]}
    assert {("imu.rpy", "lock+"), ("imu.rpy", "lock-"), ("bl.rpy", "lock+"), ("bl.rpy", "lock-")} <= sites


def cond_of(name, run=None):
    """Smallest hypot(y, x) feeding an atan2 of the case's getRPY calls (see the module docstring); run(chain): another
    computation than the case's scans."""
    c = 1.0
    ch = dp.Chain()
    case = dp.CASES[name]
    seen = []
    orig = ch.tf_get_rpy

    def spy(m):
        seen.append([float(v) for v in m])
        return orig(m)
    ch.tf_get_rpy = spy
    if run is None:
        ch.run(case)
    else:
        run(ch)
    for m in seen:
        pairs = [(m[7], m[8])] if abs(m[6]) >= 1 else [(m[7], m[8]), (m[3], m[0])]
        for y, x in pairs:
            h = math.hypot(y, x)
            if h > 0.0:
                c = min(c, h)
    return c


def growth_of(name):
    case = dp.CASES[name]
    if not (case.mode == 0 and not case.use_imu and case.scans > 1):
        return 1.0
    d = [float(np.abs(dp.mm3(r["final"].reshape(3, 4)[:, :3].T, r["final"].reshape(3, 4)[:, :3]) - np.eye(3)).max()) for r in dp.mp_run(name)]
    return max(d) / d[0]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_header_against_50_digits(orc, hc, name):
    case = dp.CASES[name]
    ref, s = dp.mp_run(name), dp.scale_of(name)
    bar = BASE * case.scans * growth_of(name) / cond_of(name)
    worst = {}
    for who, got in (("oracle", dp.orc_run(orc, name)), ("header", dp.hc_run(name)), ("float64 restatement", dp.float_run(name)[0])):
        if got is None:
            continue
        worst[who] = max(dp.pose_distance(g, r, s) for g, r in zip(got, ref))
        assert worst[who] <= bar, (name, who, worst[who], bar)
    # the header's prediction and its start point for the next scan
    for g, r in zip(dp.hc_run(name), ref):
        d = np.abs(g["pred"] - r["pred"])
        d[[3, 7, 11]] /= s
        dq = min(np.abs(g["pred_q"] - r["pred_q"]).max(), np.abs(g["pred_q"] + r["pred_q"]).max())
        assert max(d.max(), dq) <= 4 * bar, (name, d.max(), dq, bar)       # (two products of three poses on top of the final pose)
    print("  %-20s bar %.2e  " % (name, bar) + "  ".join("%s %.2e" % kv for kv in worst.items()) + "  yardstick %.2e" % dp.yardstick(orc, name))
    # the new frame: the oracle's window against the header's transform_point of the same final pose, bit for bit
    o = dp.orc_run(orc, name)
    if o is not None:
        for k in (0, case.scans - 1):
            assert np.array_equal(o[k]["frame"], dp.hc_transform(o[k]["final"], dp.edges64())), name
            assert np.array_equal(o[k]["frame"], orc.transform(o[k]["final"].reshape(3, 4), dp.edges64())), name


def test_tie_and_trace_cases_on_the_free_functions(orc, hc):
    """The cases with a given start point, on what the oracle has for them: pose_ops = toRotationMatrix, then Quaterniond(Matrix3d)
    (rotation mode 0), equal to the header bit for bit (test_transform_pose_bitwise's claim) and to the restatement."""
    n = 0
    for name, case in dp.CASES.items():
        if case.start_q is None:
            continue
        n += 1
        q, t = np.array(case.start_q), dp.device_state(name)["param_t"]
        T_o, qb_o = orc.pose_ops(q, t)
        T_h, qb_h = np.zeros(12), np.zeros(4)
        hc.hc_pose_ops(dp._dp(q), dp._dp(t), dp._dp(T_h), dp._dp(qb_h))
        assert np.array_equal(T_o.reshape(12), T_h) and np.array_equal(qb_o, qb_h), name
        assert np.array_equal(qb_o, dp.float_run(name)[0][0]["pose"][:4]), name
    assert n >= 4


def test_same_orientation_same_result(orc):
    for name, case in dp.CASES.items():
        other = case.aim.get("same_as") or case.aim.get("close_to")
        if not other:
            continue
        for run in (dp.hc_run, lambda n: dp.orc_run(orc, n)):
            a, b = run(name)[0], run(other)[0]
            if "same_as" in case.aim:        # q and -q: every product in setRotation has the same sign pattern
                assert np.array_equal(a["final"], b["final"]) and np.array_equal(a["pose"], b["pose"]), name
            else:
                assert dp.pose_distance(a, b, dp.scale_of(name)) <= BASE, name


def test_the_side_of_the_cut_shows_in_the_result(orc):
    """+pi and -pi, and pi and the double before it, are told apart by the tiny entries of the final pose (designed_poses.cut_agrees):
    oracle and header agree there on every cut case, and no cut case agrees with its sibling on the other side or one step away."""
    assert len(dp.CUT_CASES) == 8
    finals = {n: dp.orc_run(orc, n)[0]["final"] for n in dp.CUT_CASES}
    for n in dp.CUT_CASES:
        assert dp.cut_agrees(dp.hc_run(n)[0]["final"], finals[n]), n
        assert dp.cut_agrees(dp.float_run(n)[0][0]["final"], finals[n]), n
    for a, b in (("gb_roll_pi", "gb_roll_mpi"), ("gb_roll_pi", "gb_roll_pi_ulp"), ("gb_roll_mpi", "gb_roll_mpi_ulp"), ("gb_roll_pi_ulp", "gb_roll_mpi_ulp"),
                 ("gb_yaw_pi", "gb_yaw_pi_ulp"), ("gb_yaw_pi_ulp", "gb_yaw_mpi_ulp"), ("gb_yaw_mpi", "gb_yaw_mpi_ulp")):
        assert not dp.cut_agrees(finals[a], finals[b]) and not dp.cut_agrees(finals[b], finals[a]), (a, b)
    # (gb_yaw_pi and gb_yaw_mpi differ in rotation mode and mounting zeros as well; their signed entries are compared directly)
    assert finals["gb_yaw_pi"][4] > 0 > finals["gb_yaw_mpi"][4]


def test_rotation_of_on_the_drift_family(orc, hc):
    import mpmath
    for name, case in dp.CASES.items():
        if case.family != "drift" or case.use_imu:
            continue
        T = np.ascontiguousarray(case.odom.reshape(12))
        g0, g1 = np.zeros(12), np.zeros(12)
        hc.hc_rotation_of(dp._dp(T), 0, dp._dp(g0))
        hc.hc_rotation_of(dp._dp(T), 1, dp._dp(g1))
        assert np.array_equal(g0, T) and np.array_equal(orc.rotation_of(case.odom, 0), case.odom), name
        with mpmath.workdps(50):
            ch = dp.Chain(mp=mpmath)
            want = np.array([float(v) for v in ch.rotation_of(ch.vec(T), 1)])
        assert np.abs(g1 - want).max() <= 5e-15 and np.abs(orc.rotation_of(case.odom, 1).reshape(12) - want).max() <= 5e-15, name
        assert np.abs(want - T).max() >= 0.1 * case.aim["eps"], name       # ... and it is not linear()


def test_oracle_step_is_the_composition_of_its_free_functions(orc):
    """Odometer.step() from a designed state, no match: predict (:148-150) in the restatement's double products, then
    orc.imu_override, Quaterniond(rotation()) through orc.publish_odom (identity mounting: its orientation output), orc.pose_ops
    (toRotationMatrix) and orc.transform — equal to the step's state, pose and new frame bit for bit."""
    n = 0
    for name, case in dp.CASES.items():
        if case.start_q is not None or case.scans > 1:
            continue
        n += 1
        o = dp.orc_run(orc, name)[0]
        ch = dp.Chain()
        pred = np.array(ch.predict(list(case.odom.reshape(12)), list(case.prev_odom.reshape(12)))).reshape(3, 4)
        if case.use_imu:
            pred = orc.imu_override(pred, np.array(case.imu_q), case.l2b, rotation_mode=case.mode)
        q = orc.publish_odom(np.eye(4)[:3], pred, 1.0, rotation_mode=case.mode)[:4]
        T, _ = orc.pose_ops(q, pred[:, 3].copy())
        pose_q = orc.publish_odom(np.eye(4)[:3], T, 1.0, rotation_mode=case.mode)[:4]
        assert np.array_equal(T.reshape(12), o["final"]), name
        assert np.array_equal(pose_q, o["pose"][:4]) and np.array_equal(T[:, 3], o["pose"][4:]), name
        assert np.array_equal(orc.transform(T, dp.edges64()), o["frame"]), name
    assert n >= 50


MUTANT_FAMILY = {"gimbal_signs": "gimbal", "tie_ge": "quat_branch", "keep_imu_yaw": "mount", "l2b_not_inverted": "mount", "ignore_mode": "drift"}


@pytest.mark.parametrize("mutation", dp.MUTATIONS)
def test_mutated_transcriptions_disagree(orc, mutation):
    """Each wrong rule, transcribed, against the oracle on the family aimed at it: it must miss by far more than any bar on at
    least one case there (and the unmutated transcription must not)."""
    fam = MUTANT_FAMILY[mutation]
    caught = []
    for name, case in dp.CASES.items():
        if case.family != fam:
            continue
        got = [dp._arr(r) for r in dp.Chain(mutate=[mutation]).run(case)]
        if case.start_q is None:
            d = max(dp.pose_distance(g, w, dp.scale_of(name)) for g, w in zip(got, dp.orc_run(orc, name)))
        else:       # (a given start point: the header stands in; the wrong candidate of a tie shows in the next start point)
            d = max(dp.pose_distance(g, w, dp.scale_of(name), with_pred=True) for g, w in zip(got, dp.hc_run(name)))
        if d > 1e-6:
            caught.append((name, d))
    print("  %s: %d of %d cases of %s" % (mutation, len(caught), sum(c.family == fam for c in dp.CASES.values()), fam), caught[:3])
    assert caught, mutation


def angle_gap(a, b, dt):
    """Largest difference of two angular twists (angles / dt) as ANGLES: a rotation of +pi and one of -pi are the same rotation,
    and which of the two atan2 returns at its cut is decided by the sign of a rounding error."""
    d = (np.asarray(a) - np.asarray(b)) * dt
    return float(np.abs((d + math.pi) % (2 * math.pi) - math.pi).max() / dt)


@pytest.mark.parametrize("name", [n for n, c in dp.CASES.items() if c.family in ("gimbal", "quat_branch") and c.start_q is None])
def test_odom_message_through_the_same_branches(orc, hc, name):
    """publishOdom runs on the host only; its twist goes through the same getRPY and its orientation through the same
    Quaterniond(rotation()).  Message of (prev = the case's odom, cur = its final pose): header against oracle at 1e-12
    (test_hostcheck.py's bar), both and the restatement against 50 digits at
    BASE / dt, the angular twist at BASE / dt / cond with cond the conditioning of the twist's own getRPY."""
    import mpmath
    case = dp.CASES[name]
    prev = np.ascontiguousarray(case.odom.reshape(12))
    cur = np.ascontiguousarray(dp.hc_run(name)[0]["final"])
    L = np.ascontiguousarray(case.l2b.reshape(12))
    msg = np.zeros(13)
    hc.hc_odom_message(dp._dp(prev), dp._dp(cur), dp._dp(L), 0.1, dp._dp(msg), case.mode)
    want = orc.publish_odom(prev.reshape(3, 4), cur.reshape(3, 4), 0.1, L.reshape(3, 4), rotation_mode=case.mode)
    cond = cond_of(name, lambda ch: ch.odom_message(list(prev), list(cur), list(L), 0.1, case.mode))      # of the twist's getRPY
    assert np.allclose(msg[:10], want[:10], atol=1e-12, rtol=0), (name, np.abs(msg - want).max())
    assert angle_gap(msg[10:], want[10:], 0.1) <= 1e-12 / cond, (name, msg[10:], want[10:], cond)
    f = dp.Chain()
    mf = np.array([float(v) for v in f.odom_message(list(prev), list(cur), list(L), 0.1, case.mode)])
    with mpmath.workdps(50):
        m = dp.Chain(mp=mpmath, pinned=f.trace)
        ref = np.array([float(v) for v in m.odom_message(m.vec(prev), m.vec(cur), m.vec(L), m.num(0.1), case.mode)])
    bar = 10 * BASE          # (/ dt = 0.1 on the twist)
    for got in (msg, want, mf):
        dq = min(np.abs(got[:4] - ref[:4]).max(), np.abs(got[:4] + ref[:4]).max())
        assert dq <= bar and np.abs(got[4:10] - ref[4:10]).max() <= bar * dp.scale_of(name), (name, dq)
        assert angle_gap(got[10:], ref[10:], 0.1) <= bar / cond, (name, got[10:], ref[10:], cond)
