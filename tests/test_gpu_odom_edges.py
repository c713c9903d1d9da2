"""Odometry edges from the scans' own covariances on an MI355X: k_odom_edges through liodom_chain_odometry_edges (the public form,
on designed records) and liodom_get_odometry_edges (the handle form, on a stream's own logs).

The public form is held to the host-compiled header (tests/odom_edge_host.cc: liodom_math.h's leaf functions run lane by lane in
the kernel's order) BYTE FOR BYTE — interval lengths at the lane-stride boundaries, batches of 1, 2 and 65 overlapping
intervals, gaps, every flag.  The handle form is held to the public form fed with what pose_log() and pose_covariance_log()
return, byte for byte again."""
import gc
import json
import os

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api

import handle_matrix as hm
import odom_edge_host_lib as hl
import odom_edge_model as om

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, R, EPR, P = 16, 900, 6, 10, 5
K = 12                                            # synthetic scans per stream
LENGTHS = (1, 2, 63, 64, 65, 129)                 # b - a at the lane-stride boundaries
_RUN = {}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return hl.build(tmp_path_factory.mktemp("odom_edge_host"))


@pytest.fixture(scope="module")
def stream():
    poses, covs = om.designed_stream(140, seed=3)
    return poses, om.records(covs)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _equal_bytes(got, want):
    assert got.dtype == api.ODOM_EDGE_DTYPE and got.shape == want.shape
    if not np.array_equal(_bytes(got), _bytes(want)):
        for i in range(got.shape[0]):
            for name in api.ODOM_EDGE_DTYPE.names:
                assert np.array_equal(_bytes(got[name][i]), _bytes(want[name][i])), (i, name, got[name][i], want[name][i])
    assert np.array_equal(_bytes(got), _bytes(want))


# ---------------------------------------------------------------------------------------------
# the public form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(), dict(inflation=2.5, floor_rotation=1e-4, floor_translation=2e-3)], ids=["raw", "inflated_floored"])
def test_lane_stride_boundaries_equal_the_host_header(host, stream, options):
    poses, recs = stream
    for length in LENGTHS:
        for a in (0, 3, 140 - 1 - length):
            got = api.chain_odometry_edges(poses, recs, [a], [a + length], **options)
            want = hl.chain(host, poses, recs, [a], [a + length], **options)
            assert int(want["flags"][0]) == api.ODOM_EDGE_VALID and int(want["n_used"][0]) == length
            _equal_bytes(got, want)
            assert np.array_equal(got["information"][0], got["information"][0].T)


def test_batches_of_overlapping_intervals_and_their_rows(host, stream):
    poses, recs = stream
    rng = np.random.default_rng(31)
    f65 = rng.integers(0, 70, 65)
    f65[:len(LENGTHS)] = np.arange(len(LENGTHS))                          # the long ones start early: 5 + 129 < 140
    t65 = f65 + np.concatenate([np.array(LENGTHS), rng.integers(1, 70, 65 - len(LENGTHS))])
    for f, t in (([5], [70]), ([5, 20], [70, 84]), (f65, t65)):
        got = api.chain_odometry_edges(poses, recs, f, t)
        _equal_bytes(got, hl.chain(host, poses, recs, f, t))
        for i in range(len(f)):                                           # row i of a batch is the one-row call
            _equal_bytes(got[i:i + 1], api.chain_odometry_edges(poses, recs, [f[i]], [t[i]]))


def test_gaps_and_every_flag(host, stream):
    poses, recs = stream
    a, b = 10, 90
    cases = []
    for ks, how in (((a + 1,), api.COV_NO_SOLVE), ((50,), api.COV_VALID | api.COV_SINGULAR), ((b,), api.COV_EVAL_FAILURE), ((a + 64, a + 65), 0)):
        r = recs.copy()
        r["flags"][list(ks)] = how
        cases.append((poses, r, api.ODOM_EDGE_VALID | api.ODOM_EDGE_GAPS, len(ks)))
    r = recs.copy(); r["scan_index"][33] = 32; r["covariance"][34][2, 5] = np.nan
    cases.append((poses, r, api.ODOM_EDGE_VALID | api.ODOM_EDGE_GAPS, 2))
    r = recs.copy(); r["flags"][a + 1:b + 1] = api.COV_FEW_RESIDUALS
    cases.append((poses, r, api.ODOM_EDGE_NOT_PD | api.ODOM_EDGE_GAPS, b - a))
    r = recs.copy(); r["covariance"][a + 1:b + 1] = 0.0
    cases.append((poses, r, api.ODOM_EDGE_NOT_PD, 0))
    for k, col in ((a, 5), (b, 0), (47, 6)):
        p = poses.copy(); p[k, col] = np.nan
        cases.append((p, recs, api.ODOM_EDGE_NO_POSE, 0))
    p = poses.copy(); p[b, :4] = 0.0
    cases.append((p, recs, api.ODOM_EDGE_NO_POSE, 0))
    seen = set()
    for p, r, flags, n_missing in cases:
        got = api.chain_odometry_edges(p, r, [a, a, 0], [b, a + 1, 9])      # the case's interval, and two the damage may not reach
        _equal_bytes(got, hl.chain(host, p, r, [a, a, 0], [b, a + 1, 9]))
        assert int(got["flags"][0]) == flags and int(got["n_missing"][0]) == n_missing and int(got["n_used"][0]) == b - a - n_missing
        seen.add(flags)
        if flags & api.ODOM_EDGE_NO_POSE:
            assert np.isnan(got["z"][0]).all() and np.isnan(got["covariance"][0]).all() and np.isnan(got["information"][0]).all()
        elif flags & api.ODOM_EDGE_NOT_PD:
            assert np.isfinite(got["z"][0]).all() and np.isnan(got["covariance"][0]).all() and np.isnan(got["information"][0]).all()
        assert int(got["flags"][2]) == api.ODOM_EDGE_VALID
    assert seen == {3, 6, 4, 8}
    # the singular records with floors are fine
    r = recs.copy(); r["covariance"][a + 1:b + 1] = 0.0
    got = api.chain_odometry_edges(poses, r, [a], [b], floor_rotation=1e-3, floor_translation=1e-2)
    _equal_bytes(got, hl.chain(host, poses, r, [a], [b], floor_rotation=1e-3, floor_translation=1e-2))
    assert int(got["flags"][0]) == api.ODOM_EDGE_VALID


def test_refusals_of_the_public_form_leave_out_untouched(stream):
    poses, recs = stream
    m = poses.shape[0]
    out = np.zeros(2, api.ODOM_EDGE_DTYPE)
    _bytes(out)[:] = 0xA5
    before = out.copy()
    for f, t, options in (([0, 5], [3, m], {}), ([0, -1], [3, 4], {}), ([0, 4], [3, 4], {}), ([0, 6], [3, 4], {}),
                          ([0, 5], [3, 9], dict(inflation=0.0)), ([0, 5], [3, 9], dict(inflation=float("nan"))),
                          ([0, 5], [3, 9], dict(floor_rotation=-1.0)), ([0, 5], [3, 9], dict(floor_translation=float("inf"))),
                          ([0, 5], [3, 9], dict(reserved=[0, 0, 1, 0]))):
        with pytest.raises(api.LiodomError) as e:
            api.chain_odometry_edges(poses, recs, f, t, out=out, **options)
        assert e.value.code == api.ERR_INVALID_ARG
        assert np.array_equal(_bytes(out), _bytes(before))
    assert api.chain_odometry_edges(poses, recs, [], []).shape == (0,)          # n = 0
    assert api.load().liodom_chain_odometry_edges(None, None, 0, None, None, 0, None, None) == 0
    ok = api.chain_odometry_edges(poses, recs, [0, 5], [3, 9], out=out)
    assert ok is out and np.all(out["flags"] == api.ODOM_EDGE_VALID)


# ---------------------------------------------------------------------------------------------
# the handle form
# ---------------------------------------------------------------------------------------------
def _handle(n_streams=1, cov=1, **cfg):
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(n_streams=n_streams, max_points=H * W, max_width=W, pose_covariance=cov, pose_log_capacity=32, **cfg))


def _scans(synth, seed, first, count):
    cfg = synth.make_cfg(H, W, 0)
    return [synth.scan(cfg, seed, k)[0] for k in range(first, first + count)]


def _logs(g, stream, count):
    poses, infos = g.pose_log(stream, 0, count)
    assert [infos[k].scan_index for k in range(count)] == list(range(count))
    return poses, api.pose_cov_records(g.pose_covariance_log(stream, 0, count))


INTERVALS = ([0, 1, 1, 4, 0, 10, 3], [3, 2, 11, 8, 11, 11, 4])


def _check_stream(g, stream):
    poses, recs = _logs(g, stream, K)
    assert int(recs["flags"][0]) == api.COV_NO_SOLVE and np.all(recs["flags"][1:] == api.COV_VALID)
    got = g.odometry_edges(stream, *INTERVALS)
    _equal_bytes(got, api.chain_odometry_edges(poses, recs, *INTERVALS))
    # (0, 3) works: scan 0's NO_SOLVE record lies outside a + 1 .. b
    assert np.all(got["flags"] == api.ODOM_EDGE_VALID) and int(got["n_used"][0]) == 3 and int(got["n_missing"][0]) == 0
    opt = dict(inflation=4.0, floor_rotation=1e-4, floor_translation=1e-3)
    _equal_bytes(g.odometry_edges(stream, *INTERVALS, **opt), api.chain_odometry_edges(poses, recs, *INTERVALS, **opt))
    return poses, got


def _refused(g, stream, f, t, code, **options):
    out = np.zeros(len(f), api.ODOM_EDGE_DTYPE)
    _bytes(out)[:] = 0x5A
    before = out.copy()
    rc = g.L.liodom_get_odometry_edges(g.h, stream, api._ip(np.asarray(f, np.int32)), api._ip(np.asarray(t, np.int32)), len(f),
                                       api.make_odom_edge_options(**options), out.ctypes.data_as(api.C.c_void_p))
    assert rc == code, (rc, code, f, t)
    assert np.array_equal(_bytes(out), _bytes(before))


def test_one_stream_handle(synth):
    g = _handle()
    for x in _scans(synth, 7, 0, K):
        g.process_scan(x, H, W)
    poses, edges = _check_stream(g, 0)
    # the range rule: limit = the 12 scans enqueued
    for f, t in (([0], [K]), ([0, 3], [3, K]), ([3], [3]), ([4], [3]), ([-1], [3]), ([0], [40])):
        _refused(g, 0, f, t, api.ERR_INVALID_ARG)
    _refused(g, 0, [0], [3], api.ERR_INVALID_ARG, inflation=-1.0)
    _refused(g, 1, [0], [3], api.ERR_INVALID_ARG)                          # no such stream
    assert g.odometry_edges(0, [], []).shape == (0,)                       # n = 0
    # the records go into a graph, and it optimises without breakdown
    keys = [0, 3, 4, 8, 11]
    rec = g.odometry_edges(0, keys[:-1], keys[1:])
    graph = api.PoseGraph(16, 32)
    start = poses[keys].copy()
    start[1:, 4:] += np.random.default_rng(2).normal(scale=0.01, size=(4, 3))      # off the measurements by a centimetre
    graph.add_nodes(start, [1, 0, 0, 0, 0])
    graph.add_edges(api.graph_edges(range(4), range(1, 5), rec["z"], rec["information"], kind=0))
    graph.add_edges(api.graph_edges([0], [4], [om.relative_pose(om.pose_in(poses[0])[0], om.pose_in(poses[11])[0])], edges["information"][4], kind=1))
    report = graph.optimize()
    # (the measurements are consistent — every Z is a relative pose of the same log —, so the optimum has no cost left)
    assert report["termination"] != "breakdown" and report["accepted_steps"] >= 1, report
    assert report["initial_cost"] > 1.0 and report["final_cost"] <= 1e-9 * report["initial_cost"], report
    assert np.max(np.abs(graph.poses()[:, 4:] - poses[keys][:, 4:])) <= 1e-6
    graph.close()
    # a seed starts a new life of the stream: 3 more scans, and an interval reaching back past the seed is refused
    g.seed_stream(poses[K - 1])
    for x in _scans(synth, 7, K, 3):
        g.process_scan(x, H, W)
    for f, t in (([0], [3]), ([2], [5]), ([0], [11]), ([1], [3])):
        _refused(g, 0, f, t, api.ERR_INVALID_ARG)
    p3, r3 = _logs(g, 0, 3)
    _equal_bytes(g.odometry_edges(0, [0, 1, 0], [1, 2, 2]), api.chain_odometry_edges(p3, r3, [0, 1, 0], [1, 2, 2]))
    # an imported state carries its scan count on: the log below it belongs to the earlier life
    blob = g.export_stream_state(0)
    assert api.parse_stream_state(blob)["scan_counter"] == 3
    g.reset_stream(0)
    g.import_stream_state(0, blob)
    for x in _scans(synth, 7, K + 3, 3):
        g.process_scan(x, H, W)
    for f, t in (([0], [2]), ([2], [5]), ([3], [6])):
        _refused(g, 0, f, t, api.ERR_INVALID_ARG)
    p6, i6 = g.pose_log(0, 0, 6)
    r6 = api.pose_cov_records(g.pose_covariance_log(0, 0, 6))
    _equal_bytes(g.odometry_edges(0, [3, 3, 4], [4, 5, 5]), api.chain_odometry_edges(p6, r6, [3, 3, 4], [4, 5, 5]))
    g.close()


def test_stream_one_of_a_lock_step_handle(synth):
    g = _handle(n_streams=2)
    g.alloc_resident(K)
    for s, seed in ((0, 7), (1, 11)):
        for k, x in enumerate(_scans(synth, seed, 0, K)):
            g.upload_scan(s, k, x)
    for k in range(K):
        g.process_resident(k, H * W, H, W)
    p0, e0 = _check_stream(g, 0)
    p1, e1 = _check_stream(g, 1)
    assert not np.array_equal(p0, p1) and not np.array_equal(e0["information"], e1["information"])
    _refused(g, 1, [0], [K], api.ERR_INVALID_ARG)
    _refused(g, 2, [0], [3], api.ERR_INVALID_ARG)
    g.close()


def test_a_handle_without_covariance_records_is_unsupported(synth):
    g = _handle(cov=0)
    for x in _scans(synth, 7, 0, 3):
        g.process_scan(x, H, W)
    _refused(g, 0, [0], [2], api.ERR_UNSUPPORTED)
    _refused(g, 0, [], [], api.ERR_UNSUPPORTED)
    with pytest.raises(api.LiodomError) as e:
        g.odometry_edges(0, [0], [2])
    assert e.value.code == api.ERR_UNSUPPORTED
    g.close()


def test_a_handle_that_never_makes_the_call_is_the_parents(monkeypatch):
    """liodom_get_modes right after creation against the parent commit's text for the same configuration on an MI355X
    (tests/golden/odom_edges_handle_modes.json: the parent's handle_plan.h through tests/handle_plan_main.cc for a device of 256
    CUs with the k_ring_split budget of 256 workgroups every handle of tests/handle_modes_mi355x.json was recorded with, no scan
    processed, the concurrency probe passing)."""
    for k in [k for k in os.environ if k.startswith("LIODOM_")]:
        monkeypatch.delenv(k)
    with open(os.path.join(HERE, "golden", "odom_edges_handle_modes.json")) as f:
        want = json.load(f)
    gc.collect()
    for name, n_streams in (("one_stream", 1), ("two_streams", 2)):
        g = _handle(n_streams=n_streams)
        got = hm.modes_string(g)
        g.close()
        assert hm.parse_modes(got)[hm.PROBE_KEY] == hm.parse_modes(want[name])[hm.PROBE_KEY], "the concurrency probe failed (a busy GPU?)"
        assert got == want[name], [(k, v, hm.parse_modes(want[name]).get(k)) for k, v in hm.parse_modes(got).items() if hm.parse_modes(want[name]).get(k) != v]
