"""The pose chain between the solves on the device, on the designed states of tests/designed_poses.py: k_imu_override (both
instances), iso_from_qt, finalize_scan's quat_from_pose and predict_next (plain stores and the pred_xch hand-over of chain mode),
rotation_of, transform_point of the new frame.

Getting a state in: a stream takes one far-away frame, its state is exported, the poses of the 416-byte record are replaced
(liodom_amd.api.patch_stream_state, with designed_poses.device_state: what finalize_scan would have left) and the blob is
imported; liodom_set_imu_orientation and liodom_set_laser_to_base as the case says.  Running the chain without a solve: the
step's edges are more than 2 m apart (test_designed_poses.py::test_the_edges_cannot_match), so no window of three frames offers
five neighbours within 1 m under any pose; every step asserts 0 matches and termination 4 on both solves FIRST.  Getting the
result out: pose_out, the pose log entry, the exported record (final_odom, prev_odom, odom = the prediction, param_q, param_t)
and the newest frame of liodom_get_window.

Bars (none taken from the device's output):
  use_imu = 0   every operation is an IEEE add, multiply, divide or square root, built without contraction: pose_out, the record
                and the window frame equal the host-compiled header (tests/hostcheck.cc) BIT FOR BIT, single scans and the
                32-scan chains alike.
  use_imu = 1   sin, cos, asin and atan2 come from the device's math library.  Against the oracle's own step from the same state:
                1e-13 (test_hostcheck.py's bar for imu_override; rotation entries absolute, translations relative to the case's
                largest) where the oracle's distance to the 50-digit value (designed_poses.yardstick) is below 1e-13, else
                MULT = 8 times that distance.  MULT: glibc documents at most 1 ulp for sin, cos, asin and atan2 in double on
                x86-64 (libm manual, "Errors in Math Functions"); the device library is built to the OpenCL double-precision
                bounds, at most 4 ulp for sin, cos and asin and 6 ulp for atan2.  Everything around the four calls is the same
                IEEE arithmetic on both sides, so an ill-conditioned case amplifies the device's 6 ulp exactly as it amplifies
                the host's 1: |device - oracle| <= |device - exact| + |oracle - exact| <= (6 + 1) x the host's error, rounded
                up to 8.  The chains accumulate per scan on both sides alike: the same multiple of the oracle's own drift.
                No case is exempt.  The worst ratio to the bar is printed per family under -s.
  branches      the inputs of every decision are products and sums, so the device must take the branch the conditions of
                test_designed_poses.py state: asserted where the other branch's result (the mutated transcription) lies more
                than 1000 bars away from the expected one — the lock at the IMU's call and the tie qb_tie_xy; at the base link's
                call and on qb_tie_yz both branches give the same result (check_branch).  A yaw or roll of +pi, of -pi and of
                the double before either differ by less than any bar: designed_poses.cut_agrees tells them apart.
  handles       every handle kind agrees with every other bit for bit on every case it runs (the device's library is the same
                in all of them); a second run after liodom_reset_stream is bit-identical; streams that sit a subset step out keep
                their state to the bit.

Handles (H = 16, R = 6, epr = 10, P = 3), code path asserted from liodom_get_modes: one stream (streamed rebuild; chain mode
for scans that come by ticket, the four-launch path for host-fed edges and with use_imu), 5 streams (three-kernel rebuild),
16 streams (lock-step; full steps and subset steps with a stream list over resident scans), both pose_rotation_mode values.

Run with -m gpu on an MI355X; -s prints the worst ratios."""
import numpy as np
import pytest

import liodom_amd as la
from liodom_amd.api import ERR_INVALID_ARG, parse_stream_state, patch_stream_state
import designed_poses as dp

pytestmark = pytest.mark.gpu

H, R, EPR, P = 16, 6, 10, dp.PREV_FRAMES
W = 100                      # columns of the resident / ticket scan (see coarse_scan)
BASE, MULT = 1e-13, 8.0
KINDS = {
    "one": (1, {"n_streams": "1", "early_rebuild": "1", "hash_build": "streamed"}),
    "s5": (5, {"n_streams": "5", "early_rebuild": "0", "hash_build": "global"}),
    "s16": (16, {"n_streams": "16", "early_rebuild": "0", "hash_build": "lds", "knn_instance": "128"}),
}
SINGLE = [n for n, c in dp.CASES.items() if c.scans == 1]
CHAINS = [n for n, c in dp.CASES.items() if c.scans > 1]

_handles, _base, _results, _worst = {}, {}, {}, {}


def note(family, ratio, where):
    if family not in _worst or ratio > _worst[family][0]:
        _worst[family] = (float(ratio), where)


def open_handle(kind, use_imu, mode):
    key = (kind, use_imu, mode)
    if key not in _handles:
        S, want = KINDS[kind]
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, use_imu=use_imu),
                      la.make_config(n_streams=S, max_points=H * W, max_width=W, pose_rotation_mode=mode))
        modes = g.modes()
        want = dict(want, rotation_mode=str(mode))      # (chain = 1 shows only while the handle is alone: test_chain_mode_by_ticket)
        assert {k: modes[k] for k in want} == want, (key, modes)
        _handles[key] = g
        g.reset_stream(0)
        pose, info = g.odometry_step(dp.far_frame(), stream=0)
        assert info.status == 0
        _base[key] = g.export_stream_state(0)
        assert parse_stream_state(_base[key])["n_frames"] == 1
    return _handles[key], _base[key]


def close_handles():
    for g in _handles.values():
        g.close()
    _handles.clear()
    _base.clear()


@pytest.fixture(scope="module", autouse=True)
def _module():
    yield
    close_handles()
    print("\n  designed poses, worst |device - oracle| / bar per family (use_imu = 1; use_imu = 0 is bit-equal to the header):")
    for fam in sorted(_worst):
        print("    %-14s %.3g   (%s)" % (fam, _worst[fam][0], _worst[fam][1]))


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def install(g, base, stream, name):
    case = dp.CASES[name]
    g.import_stream_state(stream, patch_stream_state(base, **dp.device_state(name)))
    if case.use_imu:
        g.set_imu(np.array(case.imu_q), stream)


def collect(g, stream, pose, info, edges, what):
    """What one finished step shows, after the assertion that both solves were empty."""
    assert list(info.matches) == [0, 0] and [info.lm[0].termination, info.lm[1].termination] == [4, 4], (what, list(info.matches), info.lm[0].termination, info.lm[1].termination)
    assert info.status == 0, (what, info.status)
    rec = parse_stream_state(g.export_stream_state(stream))
    log, _ = g.pose_log(stream, info.scan_index, 1)
    assert bits(log[0]) == bits(pose), what
    win, nf = g.window(stream)
    frame = win[-len(edges):]
    # transform_point alone: the new frame is the edges under the device's OWN final pose, bit for bit
    assert bits(frame) == bits(dp.hc_transform(rec["final_odom"], edges)), what
    assert bits(rec["final_odom"]) == bits(rec["prev_odom"]), what
    assert bits(pose[4:]) == bits(rec["final_odom"][:, 3]), what
    return dict(pose=pose.copy(), final=rec["final_odom"].reshape(12).copy(), pred=rec["odom"].reshape(12).copy(), pred_q=rec["param_q"].copy(),
                param_t=rec["param_t"].copy(), prev=rec["prev_odom"].reshape(12).copy())


def bar_of(orc, name):
    y = dp.yardstick(orc, name)
    if dp.CASES[name].scans > 1:        # a chain: the oracle's own drift over the scans, times the margin
        return MULT * y
    return BASE if y < BASE else MULT * y


def check(orc, name, got, k, what):
    """One scan's device result against the expectation of its kind."""
    case, exp = dp.CASES[name], dp.hc_run(name)[k]
    if not case.use_imu:
        for key, want in (("pose", exp["pose"]), ("final", exp["final"]), ("prev", exp["record"]["prev_odom"]), ("pred", exp["record"]["odom"]),
                          ("pred_q", exp["record"]["param_q"]), ("param_t", exp["record"]["param_t"])):
            assert bits(got[key]) == bits(want), (what, key, got[key], want)
        return
    o, s, bar = dp.orc_run(orc, name)[k], dp.scale_of(name), bar_of(orc, name)
    d = dp.pose_distance(got, o, s)
    note(case.family, d / bar, what)
    assert d <= bar, (what, d, bar)
    if name in dp.CUT_CASES:      # the side of atan2's cut, and pi against the double before it: invisible at 1e-13, see cut_agrees
        assert dp.cut_agrees(got["final"], o["final"]), (what, got["final"], o["final"])
    # the prediction left for the next scan (the oracle forms it at the start of its next step: the header stands in, at 4 bars —
    # two more products of three poses)
    dpred = dp.pose_distance(dict(final=got["pred"], pose=np.concatenate([got["pred_q"], got["param_t"]])),
                             dict(final=exp["record"]["odom"], pose=np.concatenate([exp["record"]["param_q"], exp["record"]["param_t"]])), s)
    assert dpred <= 4 * bar, (what, dpred, bar)


def check_branch(orc, name, got, what):
    """Lock cases at the IMU's call and the tie case whose candidates differ (qb_tie_xy): the other branch is far away, so being
    within the bar IS having taken the stated branch.  Not so for the lock at the base link's call (gb_bl_lock_*, mt_on_its_side)
    and for qb_tie_yz: only bl_yaw is used of that getRPY and both lock signs give yaw 0, and the tied pair of qb_tie_yz gives
    the same quaternion from either candidate — there the two branches agree and the result cannot tell which was taken."""
    case = dp.CASES[name]
    mutation = None
    if any(v in ("lock+", "lock-") for k, v in case.aim.items() if k.endswith(".rpy")) and "imu.rpy" in case.aim:
        mutation = "gimbal_signs"
    elif name == "qb_tie_xy":       # (qb_tie_yz is symmetric in its tied pair: both candidates give the same quaternion)
        mutation = "tie_ge"
    if mutation is None:
        return 0
    alt = dp._arr(dp.Chain(mutate=[mutation]).run(case)[0])
    exp = dp.hc_run(name)[0]
    gap = dp.pose_distance(alt, exp, dp.scale_of(name), with_pred=True)
    bar = bar_of(orc, name)
    assert gap > 1000 * bar, (what, gap)
    mine = dict(got, pred=got["pred"], pred_q=got["pred_q"])
    assert dp.pose_distance(mine, exp, dp.scale_of(name), with_pred=True) <= 4 * bar, what
    return 1


def run_host_fed(orc, kind, name, stream):
    """The case on handle `kind`, stream `stream`, through liodom_odometry_step.  Returns the per-scan results it checked."""
    case = dp.CASES[name]
    g, base = open_handle(kind, case.use_imu, case.mode)
    g.set_laser_to_base(case.l2b)
    install(g, base, stream, name)
    e, out = dp.edges64(), []
    for k in range(case.scans):
        what = "%s stream %d %s scan %d" % (kind, stream, name, k)
        pose, info = g.odometry_step(e, stream=stream)
        if k in (0, 1, case.scans // 2, case.scans - 1):
            got = collect(g, stream, pose, info, e, what)
            check(orc, name, got, k, what)
            out.append(got)
        else:
            assert list(info.matches) == [0, 0] and info.lm[1].termination == 4 and info.status == 0, what
            if not case.use_imu:
                assert bits(pose) == bits(dp.hc_run(name)[k]["pose"]), what
    _results.setdefault(name, {})[kind] = out
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_single_scans(orc, kind):
    """Every single-scan case on every handle kind, cases rotating over the handle's streams so that a stream's neighbours hold
    other cases; lock and tie cases additionally against the other branch."""
    S = KINDS[kind][0]
    n_branch = 0
    for i, name in enumerate(SINGLE):
        got = run_host_fed(orc, kind, name, (5 * i + 3) % S)
        n_branch += check_branch(orc, name, got[0], "%s %s" % (kind, name))
    assert n_branch >= 4
    # q and -q are the same orientation: every product of setRotation has the same sign pattern, so the DEVICE's two results are
    # the same bits (each was held to the oracle above; this holds them to each other)
    n_same = 0
    for name, case in dp.CASES.items():
        if "same_as" in case.aim:
            a, b = _results[name][kind][0], _results[case.aim["same_as"]][kind][0]
            for key in a:
                assert bits(a[key]) == bits(b[key]), (kind, name, key)
            n_same += 1
    assert n_same >= 1


@pytest.mark.parametrize("kind", list(KINDS))
def test_chains(orc, kind):
    S = KINDS[kind][0]
    for i, name in enumerate(CHAINS):
        run_host_fed(orc, kind, name, (7 * i + 2) % S)


def test_handles_agree_bit_for_bit(orc):
    n = 0
    for name in SINGLE + CHAINS:
        for kind in KINDS:        # (what the tests above collected; run here when this test runs on its own)
            if kind not in _results.get(name, {}):
                run_host_fed(orc, kind, name, 0)
        by_kind = _results[name]
        kinds = sorted(by_kind)
        for other in kinds[1:]:
            for a, b in zip(by_kind[kinds[0]], by_kind[other]):
                for key in a:
                    assert bits(a[key]) == bits(b[key]), (name, kinds[0], other, key)
                n += 1
    assert n >= 2 * len(SINGLE), "run the whole module: this test compares what the others collected"


def test_second_run_after_reset_stream_is_identical(orc):
    for kind, name, stream in (("one", "gb_pitch_p_1e8", 0), ("s16", "mt_rot_03", 11), ("s5", "ch_m0", 4)):
        first = run_host_fed(orc, kind, name, stream)
        case = dp.CASES[name]
        g, _ = open_handle(kind, case.use_imu, case.mode)
        g.reset_stream(stream)
        pose, info = g.odometry_step(dp.far_frame(), stream=stream)
        assert np.array_equal(pose, [0, 0, 0, 1, 0, 0, 0])
        again = run_host_fed(orc, kind, name, stream)
        for a, b in zip(first, again):
            for key in a:
                assert bits(a[key]) == bits(b[key]), (kind, name, key)


def test_set_imu_orientation_refuses_what_poisons_the_stream(orc):
    """A zero or non-finite quaternion: LIODOM_ERR_INVALID_ARG, the stored orientation unchanged, and the next step equal to a
    run without the call.  (Before the check the copy went through, tf's setRotation divided by zero and the stream's odom was
    NaN for good, with no status bit.)"""
    name = "iq_q"
    case = dp.CASES[name]
    want = run_host_fed(orc, "one", name, 0)[0]
    g, base = open_handle("one", 1, case.mode)
    install(g, base, 0, name)
    for bad in ([0.0, 0.0, 0.0, 0.0], [np.nan, 0.0, 0.0, 1.0], [0.0, np.inf, 0.0, 1.0], [0.0, 0.0, -np.inf, 0.0], [1e-170, 0.0, 0.0, 1e-170]):
        q = np.array(bad)
        assert g.L.liodom_set_imu_orientation(g.h, 0, q.ctypes.data_as(la.api.C.POINTER(la.api.C.c_double))) == ERR_INVALID_ARG, bad
        assert g.L.liodom_set_imu_orientation(g.h, 0, None) == ERR_INVALID_ARG
    assert bits(parse_stream_state(g.export_stream_state(0))["imu_q"]) == bits(np.array(case.imu_q))
    pose, info = g.odometry_step(dp.edges64(), stream=0)
    got = collect(g, 0, pose, info, dp.edges64(), "after refused orientations")
    assert np.isfinite(pose).all()
    for key in got:
        assert bits(got[key]) == bits(want[key]), key
    # non-unit quaternions stay accepted
    g.set_imu(np.array(case.imu_q) * 1e3, 0)
    g.set_imu(-np.array(case.imu_q) * 1e-3, 0)


# ---------------------------------------------------------------------------------------------
# scans that come by extraction: resident lock-step steps, subset steps, and chain mode by ticket
# ---------------------------------------------------------------------------------------------
def coarse_scan():
    """16 rings at the mid-bin elevations -15 .. 15 degrees, 100 columns, XY ranges 62 .. 72 m: neighbours on a ring are 3.9 m
    apart and neighbouring rings 2.1 m, so WHATEVER the extraction picks, its edges are more than 2 m apart and cannot match a
    window of three frames (the argument of designed_poses.edges64)."""
    x = np.zeros((H, W, 4), np.float32)
    for r in range(H):
        el = np.deg2rad(-15.0 + 2.0 * r)
        for c in range(W):
            rng = 62.0 + 10.0 * ((c * 0.6180339887498949 + r * 0.7548776662466927) % 1.0)
            az = 2.0 * np.pi * (c + 0.37 * (r % 3)) / W
            x[r, c] = (rng * np.cos(az), rng * np.sin(az), rng * np.tan(el), 1.0)
    return x.reshape(-1, 4)


def edges_apart(e):
    p = e[:, :3].astype(np.float64)
    d = np.linalg.norm(p[:, None] - p[None], axis=2) + 1e9 * np.eye(len(p))
    return len(p) >= 32 and d.min() > 2.0


LOCKSTEP16 = [n for n in SINGLE if dp.CASES[n].use_imu and dp.CASES[n].mode == 1 and np.array_equal(dp.CASES[n].l2b, dp.I34)][:16]


def test_lockstep_step_and_subset_step_over_resident_scans(orc):
    """Sixteen different override cases in the sixteen streams of ONE lock-step step (k_imu_override<false>), then — from the same
    states — a subset step with a stream list (k_imu_override<true>): the listed streams give the full step's results bit for bit,
    the streams that sit out keep their exported state to the bit."""
    assert len(LOCKSTEP16) == 16
    g, base = open_handle("s16", 1, 1)
    g.set_laser_to_base(dp.I34)
    scan = coarse_scan()
    g.alloc_resident(1)
    for s in range(16):
        g.upload_scan(s, 0, scan)

    def install_all():
        for s, name in enumerate(LOCKSTEP16):
            install(g, base, s, name)
        return [g.export_stream_state(s) for s in range(16)]

    install_all()
    poses, infos = g.process_resident(0, H * W, H, W)
    full = {}
    for s, name in enumerate(LOCKSTEP16):
        e = g.get_edges(s)["edges"]
        assert edges_apart(e), (s, len(e))
        what = "lock-step step, stream %d %s" % (s, name)
        full[s] = collect(g, s, poses[s], infos[s], e, what)
        check(orc, name, full[s], 0, what)
        check_branch(orc, name, full[s], what)
        host_fed = _results.get(name, {}).get("s16")
        if host_fed:      # the same case fed by liodom_odometry_step on whichever stream: same bits
            for key in ("pose", "final", "pred", "pred_q", "param_t"):
                assert bits(full[s][key]) == bits(host_fed[0][key]), (what, key)
    before = install_all()
    listed = [1, 4, 5, 9, 15]
    poses, infos = g.process_resident_subset(0, listed, H * W, H, W)
    assert int(g.modes().get("subset_steps", "0")) >= 1
    for i, s in enumerate(listed):
        what = "subset step, stream %d %s" % (s, LOCKSTEP16[s])
        got = collect(g, s, poses[i], infos[i], g.get_edges(s)["edges"], what)
        for key in got:
            assert bits(got[key]) == bits(full[s][key]), (what, key)
    for s in range(16):
        if s not in listed:
            assert g.export_stream_state(s) == before[s], s


@pytest.mark.parametrize("mode", [1, 0])
def test_chain_mode_by_ticket(orc, mode):
    """One stream, use_imu = 0, scans by ticket: after the warm-up scans the handle runs chain mode — the prediction travels to the
    next scan's first pass as pred_xch granules, its speculative copy formed beside the last evaluation — for the rest of the
    32-scan chain.  Chain mode needs the GPU to itself: every other handle of the module is closed first.  Poses and the final
    record equal the header bit for bit, and liodom_get_modes shows that chain-mode workgroups ran."""
    close_handles()
    name = "ch_m%d" % mode
    case = dp.CASES[name]
    g, base = open_handle("one", 0, mode)
    assert g.modes()["chain"] == "1", g.modes()
    install(g, base, 0, name)
    scan = coarse_scan()
    exp = dp.hc_run(name)
    for k in range(case.scans):
        t = g.extract_edges_device(scan, H, W)
        assert t is not None
        pose, info = g.odometry_step_device(t)
        what = "chain mode %s scan %d" % (name, k)
        assert list(info.matches) == [0, 0] and [info.lm[0].termination, info.lm[1].termination] == [4, 4] and info.status == 0, what
        assert bits(pose) == bits(exp[k]["pose"]), (what, pose, exp[k]["pose"])
    e = g.get_edges(0)["edges"]
    assert edges_apart(e)
    got = collect(g, 0, pose, info, e, name + " by ticket")
    check(orc, name, got, case.scans - 1, name + " by ticket")
    # every scan behind the warm-up ran in chain mode: chain_done counts the first-pass workgroups launched in chain mode since the
    # import (knn_grid of them per scan); the first kOvWarmScans = 2 scans of a restarted stream (step_plan.h) run every launch on
    # one stream.  A handle that drops out of chain mode on the way falls short.
    modes = g.modes()
    chain_scans = int(modes["chain_done"].split("/")[0]) / int(modes["knn_grid"].split("/")[0])
    print("\n  %s: %g of %d scans in chain mode" % (name, chain_scans, case.scans))
    assert chain_scans == case.scans - 2, modes
    close_handles()
