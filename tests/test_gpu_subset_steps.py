"""Subset steps (liodom_process_resident_subset): a lock-step handle advances the streams of a list and the others sit the step out.

Every stream runs a sequence of its own (synthetic stream 100 + s, ragged where s % 4 == 3) at the cheap 16 x 900 shape, K = P + 2
rebuild periods + 3 = 16 scans.  The reference is the same data through FULL lock-step steps of an S-stream handle
(test_gpu_lockstep_shapes.lockstep_replay: the path test_stream_count_switches_against_the_oracle holds to the oracle); a second
handle is stepped by a fixed schedule of subsets — each stream consumes its next scan whenever it is listed — and each listed
stream's Record (pose bits, n_edges, map_points, match counts, LM iterations and terminations, digests of get_edges and of both
passes' correspondences) must equal records[k_s][s] of the reference, k_s counting the stream's own scans.  S = 3 (streamed
rebuild, four-workgroup solves), 8 (three-kernel rebuild) and 16 (lock-step kernels, incremental cell hash).
  1. the schedule, bit for bit;  2. idle streams untouched (state blob, pose log, getters);  3. extraction issued ahead: right hint,
  wrong hint, NULL hint, a plain full step after a subset extraction;  4. launch economy and the full list;  5. pose_covariance,
  filter_local_map, use_imu, safe mode;  6. refusals;  7. continuous batching with idle slots sitting out.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
from test_gpu_lockstep_shapes import HB_PERIOD, Record, assert_records_equal, digest, lockstep_replay, set_env
from test_gpu_stream_counts import stream_count
from test_gpu_stream_state import _cov_bits, bits

pytestmark = pytest.mark.gpu

SMALL = (16, 900, 0, 6, 10, 5)                  # H, W, lidar_type, R, epr, P
K = SMALL[5] + 2 * HB_PERIOD + 3                # 16 scans per stream
N_SLOTS = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- data, schedule, references -------------------------------------------------------------------------------------------------
_DATA, _REF = {}, {}


def data_of(synth, S):
    if S not in _DATA:
        H, W, lt = SMALL[:3]
        cfg = synth.make_cfg(H, W, lt)
        d = [[synth.scan(cfg, 100 + s, k)[0] for k in range(K)] for s in range(S)]
        for s in range(3, S, 4):
            d[s] = [synth.ragged(x, H, W, lt, seed=100 * s + k) for k, x in enumerate(d[s])]
        _DATA[S] = d
    return _DATA[S]


def schedule(S):
    """The subsets, step by step: designed steps first, then a seeded 60 % draw per stream until every stream has had K scans."""
    third = [s for s in range(S) if s % 3 == 0]
    steps = [list(range(S)), [0], [S - 1], list(range(1, S)), list(range(0, S, 2)), list(range(1, S - 1))]
    steps += [[s for s in range(S) if s % 3 != 0]] * 5           # the streams with s % 3 == 0 sit out five steps
    steps += [third] * 5                                         # ... then every other stream does
    left = [K] * S
    for L in steps:
        for s in L:
            left[s] -= 1
    assert min(left) > 0
    rng = np.random.default_rng(20 + S)
    while any(left):
        L = [s for s in range(S) if left[s] and rng.random() < 0.6]
        for s in L:
            left[s] -= 1
        if L:
            steps.append(L)
    return steps


def contiguous(L):
    return L == list(range(L[0], L[0] + len(L)))


def check_schedule(S, sched):
    """The properties the tests rely on, from the schedule alone."""
    full = list(range(S))
    assert sched[0] == full
    for want in ([0], [S - 1], full[1:], full[::2]):
        assert want in sched, want
    assert any(contiguous(L) and L[0] > 0 and L[-1] < S - 1 for L in sched)
    out = [all(s % 3 != 0 for s in L) for L in sched]
    assert any(all(out[t:t + 5]) for t in range(len(sched) - 4))
    assert any(not contiguous(L) for L in sched) and any(len(L) == 1 for L in sched) and any(L == full for L in sched)
    assert all(L and L == sorted(set(L)) and 0 <= L[0] and L[-1] < S for L in sched)
    assert sum(len(L) for L in sched) == S * K
    for s in range(S):
        on = [t for t, L in enumerate(sched) if s in L]
        assert len(on) == K
        # an idle gap longer than the edge pipeline (3 buffers) and than a rebuild period, with steps of the stream after it
        assert max(b - a - 1 for a, b in zip(on, on[1:])) >= HB_PERIOD + 1, (s, on)


def split_of(S):
    fit = stream_count("fit")
    return "k_ring_split" if S <= fit else ("k_ring_split_lb" if S >= 16 else "k_classify + k_ring_scatter")


def reference(orc, synth, monkeypatch, S):
    """records[k][s] and the modes of S streams fed data_of(S) by full lock-step steps; computed once per S."""
    if S not in _REF:
        r = lockstep_replay(orc, SMALL, data_of(synth, S), {}, {"n_streams": str(S)}, split_of(S), monkeypatch, next_slot=True)
        _REF[S] = r.records
    return _REF[S]


def open_handle(S, params=None, **cfgkw):
    H, W, lt, R, epr, P = SMALL
    cfg = dict(n_streams=S, max_points=H * W, max_width=W, debug_buffers=1, pose_log_capacity=K + 8)
    cfg.update(cfgkw)
    return la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, **(params or {})),
                     la.make_config(**cfg))


def record_of(g, s, pose, info):
    c = [g.correspondences(it, stream=s) for it in (0, 1)]
    e = g.get_edges(s)
    return Record(pose.view(np.uint64).tobytes(), info.n_edges, info.map_points, tuple(info.matches),
                  tuple((t.iterations, t.termination) for t in info.lm),
                  digest(e["edges"].view(np.uint32), e["ring"], e["idx_in_ring"], e["src"]), tuple(digest(*ci) for ci in c))


def imu_q(s, k):
    q = np.array([0.02 * np.sin(1.0 + s + 0.7 * k), 0.02 * np.cos(2.0 + 0.3 * s * k), 0.0, 1.0])
    return q / np.linalg.norm(q)


def full_steps(g, data, imu=False):
    """K full lock-step steps (process_resident) of data on g: records[k][s]."""
    H, W = SMALL[:2]
    S = len(data)
    g.alloc_resident(N_SLOTS)
    records = []
    for k in range(K):
        for s in range(S):
            g.upload_scan(s, k % N_SLOTS, data[s][k])
            if imu:
                g.set_imu(imu_q(s, k), stream=s)
        poses, infos = g.process_resident(k % N_SLOTS, H * W, H, W, readback=True)
        assert all(i.status == 0 for i in infos)
        records.append([record_of(g, s, poses[s], infos[s]) for s in range(S)])
    return records


def wrong_list(S, L):
    """A valid list that differs from L: its complement, or L without its first entry."""
    other = [s for s in range(S) if s not in L]
    return other if other else L[1:]


def subset_steps(g, data, sched, ref, hint=None, imu=False, first_step=0, ks=None, alloc=True):
    """Steps g through sched[first_step:]: stream s consumes data[s][ks[s]] whenever it is listed; every listed stream's record must
    equal ref[ks[s]][s].  hint: None (no extraction ahead), "right" (the next step's slot and list), "wrong" (its slot, another
    list), "null" (its slot, NULL list = this step's).  The scans of a step are in resident slot step % N_SLOTS, uploaded one step
    ahead (with every readback the previous reader of that slot has completed).  Returns ks."""
    H, W = SMALL[:2]
    S = len(data)
    ks = [0] * S if ks is None else ks
    if alloc:
        g.alloc_resident(N_SLOTS)

    def upload(t, consumed=()):
        for s in (range(S) if hint in ("wrong", "null") else sched[t]):       # (such a hint may name any stream: every place holds a scan)
            g.upload_scan(s, t % N_SLOTS, data[s][min(ks[s] + (1 if s in consumed else 0), K - 1)])

    upload(first_step)
    for t in range(first_step, len(sched)):
        L = sched[t]
        nxt = sched[t + 1] if t + 1 < len(sched) else None
        if nxt is not None:
            upload(t + 1, consumed=L)
        if imu:
            for s in L:
                g.set_imu(imu_q(s, ks[s]), stream=s)
        kw = {}
        if hint and nxt is not None:
            kw = dict(next_slot=(t + 1) % N_SLOTS, next_streams={"right": nxt, "wrong": wrong_list(S, nxt), "null": None}[hint])
        poses, infos = g.process_resident_subset(t % N_SLOTS, L, H * W, H, W, readback=True, **kw)
        assert poses.shape == (len(L), 7) and len(infos) == len(L)
        for i, s in enumerate(L):
            what = ("S", S, "hint", hint, "step", t, "list", L, "stream", s, "scan", ks[s])
            assert infos[i].status == 0 and infos[i].scan_index == ks[s], (what, infos[i].status, infos[i].scan_index)
            assert_records_equal(record_of(g, s, poses[i], infos[i]), ref[ks[s]][s], what)
            ks[s] += 1
    return ks


def assert_pose_logs(g, ref, S):
    g.sync()
    for s in range(S):
        lp, li = g.pose_log(s, 0, K)
        for k in range(K):
            assert lp[k].view(np.uint64).tobytes() == ref[k][s].pose and li[k].scan_index == k, ("pose log", s, k)


# ---- 1. subset steps equal full lock-step, per stream, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 8, 16])
def test_subset_steps_equal_full_steps(orc, synth, monkeypatch, S):
    sched = schedule(S)
    check_schedule(S, sched)
    print("S = %d: %d steps, %d not contiguous, sizes %d .. %d" % (S, len(sched), sum(not contiguous(L) for L in sched),
                                                                 min(map(len, sched)), max(map(len, sched))))
    ref = reference(orc, synth, monkeypatch, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    ks = subset_steps(g, data_of(synth, S), sched, ref)
    assert ks == [K] * S
    assert_pose_logs(g, ref, S)
    m = g.modes()
    g.close()
    # (step 0 — the full list, nothing ahead — is the plain step; every other step ran over a list)
    assert int(m["subset_steps"]) == sum(len(L) < S for L in sched) > 0, m
    if S == 16:
        assert m["knn8"] == "1" and m["hash_incr"] == "1" and int(m["hash_rebuilds"]) > 0 and int(m["hash_appends"]) > 0, m


# ---- 2. idle streams are untouched -------------------------------------------------------------------------------------------------
def test_idle_streams_are_untouched(orc, synth, monkeypatch):
    S, idle, n0 = 16, [3, 8], 3
    H, W = SMALL[:2]
    ref = reference(orc, synth, monkeypatch, S)
    data = data_of(synth, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    full = list(range(S))
    ks = subset_steps(g, data, [full] * n0, ref)

    def view(s):
        g.sync()
        e = g.get_edges(s)
        lp, li = g.pose_log(s, 0, K)
        return (g.export_stream_state(s), bits(lp), [bytes(i) for i in li],
                digest(e["edges"].view(np.uint32), e["ring"], e["idx_in_ring"], e["src"]),
                [digest(*g.correspondences(it, stream=s)) for it in (0, 1)], [digest(g.knn_queries(it, stream=s)) for it in (0, 1)],
                digest(g.window(s)[0]), digest(g.local_map(s)[0]))

    before = {s: view(s) for s in idle}
    assert all(api.parse_stream_state(before[s][0])["scan_counter"] == n0 for s in idle)
    others = [s for s in full if s not in idle]
    sched = [full] * n0 + [others, others[::2], others]          # three steps (one of them scattered) that leave the two out
    ks = subset_steps(g, data, sched, ref, first_step=n0, ks=ks, alloc=False)
    for s in idle:
        after = view(s)
        for j, name in enumerate(["state blob", "pose log", "info log", "edges", "correspondences", "knn queries", "window", "local map"]):
            assert after[j] == before[s][j], ("idle stream", s, name)
    # the two step again, alone, then everybody
    sched += [idle, full]
    ks = subset_steps(g, data, sched, ref, first_step=n0 + 3, ks=ks, alloc=False)
    assert ks[idle[0]] == n0 + 2 and ks[0] == n0 + 4 and ks[others[1]] == n0 + 3
    assert int(g.modes()["subset_steps"]) == 4
    g.close()


# ---- 3. extraction issued ahead ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", ["right", "wrong", "null"])
@pytest.mark.parametrize("S", [3, 16])
def test_extraction_issued_ahead(orc, synth, monkeypatch, S, hint):
    """The schedule of test 1 with every step issuing the next step's extraction: for the list the next step names, for another
    list (the extraction is issued again), for NULL (= this step's list, right only where two steps name the same one)."""
    sched = schedule(S)
    ref = reference(orc, synth, monkeypatch, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    ks = subset_steps(g, data_of(synth, S), sched, ref, hint=hint)
    assert ks == [K] * S
    assert_pose_logs(g, ref, S)
    assert int(g.modes()["subset_steps"]) > 0
    g.close()


def test_plain_step_after_a_subset_extraction(orc, synth, monkeypatch):
    """A subset step issues slot 1's extraction ahead for three streams; the plain full step on slot 1 must extract every stream."""
    S = 16
    H, W = SMALL[:2]
    ref = reference(orc, synth, monkeypatch, S)
    data = data_of(synth, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    g.alloc_resident(N_SLOTS)
    for k in (0, 1, 2):
        for s in range(S):
            g.upload_scan(s, k, data[s][k])
    poses, infos = g.process_resident_subset(0, list(range(S)), H * W, H, W, next_slot=1, next_streams=[0, 2, 5])
    for s in range(S):
        assert_records_equal(record_of(g, s, poses[s], infos[s]), ref[0][s], ("step 0", s))
    assert int(g.modes()["subset_steps"]) == 1                     # (a full step with a list ahead does not delegate)
    poses, infos = g.process_resident(1, H * W, H, W, readback=True, next_slot=2)
    for s in range(S):
        assert infos[s].status == 0
        assert_records_equal(record_of(g, s, poses[s], infos[s]), ref[1][s], ("plain step 1", s))
    # and the other way round: the plain step issued slot 2 ahead for every stream, a subset step takes some of them
    L = [1, 4, 15]
    poses, infos = g.process_resident_subset(2, L, H * W, H, W)
    for i, s in enumerate(L):
        assert_records_equal(record_of(g, s, poses[i], infos[i]), ref[2][s], ("subset step 2", s))
    g.close()


# ---- 4. launch economy and the full list -------------------------------------------------------------------------------------------
def test_launch_economy_and_the_full_list(orc, synth, monkeypatch):
    """By kernel_stats() under set_profiling(1): a step over the scattered list [0, 2, 5, 9, 15] books no more launches than a full
    step (one sequence, not one per run of the list; the list uploads — two one-workgroup launches that carry the list in their
    arguments — are not booked, like the copies of the other entry points), and the full list through the new call books exactly
    the plain step's launches, gives its bits and is not counted as a subset step."""
    S = 16
    H, W = SMALL[:2]
    ref = reference(orc, synth, monkeypatch, S)
    data = data_of(synth, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    g.alloc_resident(K)
    for k in range(6):
        for s in range(S):
            g.upload_scan(s, k, data[s][k])
    full = list(range(S))
    g.set_profiling(1)

    def booked(step):
        g.reset_kernel_stats()
        out = step()
        return {k: n for k, (n, _) in g.kernel_stats().items() if n}, out

    def check(out, k, streams):
        poses, infos = out
        for i, s in enumerate(streams):
            assert_records_equal(record_of(g, s, poses[i], infos[i]), ref[k][s], ("step", k, "stream", s))

    for k in (0, 1):
        check(g.process_resident(k, H * W, H, W, readback=True), k, full)
    plain, out = booked(lambda: g.process_resident(2, H * W, H, W, readback=True))
    check(out, 2, full)
    # the full list through the new call: the plain step — same launches, same bits, not counted
    same, out = booked(lambda: g.process_resident_subset(3, full, H * W, H, W))
    check(out, 3, full)
    assert same == plain, (same, plain)
    assert int(g.modes()["subset_steps"]) == 0
    # a scattered list: one launch sequence, not one per run of the list
    scattered = [0, 2, 5, 9, 15]
    sub, out = booked(lambda: g.process_resident_subset(4, scattered, H * W, H, W))
    check(out, 4, scattered)
    print("launches booked: full step %s, scattered subset %s" % (plain, sub))
    assert sum(sub.values()) <= sum(plain.values()), (sub, plain)
    assert int(g.modes()["subset_steps"]) == 1
    g.set_profiling(0)
    g.close()


# ---- 5. options --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,S", [("pose_covariance", 16), ("filter_local_map", 3), ("use_imu", 8), ("safe_mode", 3)])
def test_options(orc, synth, monkeypatch, option, S):
    """The schedule of test 1 against full steps of a handle with the same option."""
    params = {"filter_local_map": {"filter_local_map": 1}, "use_imu": {"use_imu": 1}}.get(option)
    cfgkw = {"pose_covariance": 1} if option == "pose_covariance" else {}
    set_env(monkeypatch, {"LIODOM_SAFE_MODE": "1"} if option == "safe_mode" else {})
    data = data_of(synth, S)
    imu = option == "use_imu"
    g = open_handle(S, params=params, **cfgkw)
    m = g.modes()
    assert m["safe_mode"] == ("1" if option == "safe_mode" else "0") and m["filter_local_map"] == ("1" if option == "filter_local_map" else "0"), m
    ref = full_steps(g, data, imu=imu)
    g.sync()
    ref_cov = [_cov_bits(g.pose_covariance_log(s, 0, K)) for s in range(S)] if option == "pose_covariance" else None
    g.close()
    if imu:         # the override moves the result: the option is on
        plain = reference(orc, synth, monkeypatch, S)
        set_env(monkeypatch, {})
        assert any(ref[k][s].pose != plain[k][s].pose for k in range(K) for s in range(S))
    g = open_handle(S, params=params, **cfgkw)
    sched = schedule(S)
    ks = subset_steps(g, data, sched, ref, hint="right", imu=imu)
    assert ks == [K] * S
    assert_pose_logs(g, ref, S)
    if ref_cov:
        for s in range(S):
            assert _cov_bits(g.pose_covariance_log(s, 0, K)) == ref_cov[s], ("covariance log", s)
    assert int(g.modes()["subset_steps"]) > 0
    g.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(orc, synth, monkeypatch):
    S = 16
    H, W = SMALL[:2]
    ref = reference(orc, synth, monkeypatch, S)
    data = data_of(synth, S)
    set_env(monkeypatch, {})
    g = open_handle(S)
    full = list(range(S))
    ks = subset_steps(g, data, [full, [1, 4, 6]], ref)
    for s in full:
        g.upload_scan(s, 2, data[s][ks[s]])
    g.sync()
    states = [g.export_stream_state(s) for s in full]
    poses = np.zeros((S + 1, 7))
    infos = (api.StepInfo * (S + 1))()

    def call(streams, n_active, next_slot=-1, next_streams=None):
        a = np.ascontiguousarray(streams, dtype=np.int32)
        b = None if next_streams is None else np.ascontiguousarray(next_streams, dtype=np.int32)
        return g.L.liodom_process_resident_subset(g.h, 2, a.ctypes.data_as(C.POINTER(C.c_int32)), n_active, next_slot,
                                                  None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), 0 if b is None else len(b),
                                                  H * W, H, W, poses.ctypes.data_as(C.POINTER(C.c_double)), infos)

    bad = [([5, 3], 2), ([3, 3], 2), ([-1, 3], 2), ([3, S], 2), (list(range(S + 1)), S + 1), (full + [0], S + 1), ([0, 1], -1)]
    for streams, n_active in bad:
        assert call(streams, n_active) == api.ERR_INVALID_ARG, (streams, n_active)
        assert call([2, 7], 2, next_slot=1, next_streams=streams[:max(n_active, 0)] or [9, 1]) == api.ERR_INVALID_ARG, ("next", streams)
        g.sync()
        assert [g.export_stream_state(s) for s in full] == states, (streams, n_active)
    # the empty list: OK, nothing advances
    assert call([0], 0) == 0
    p0, i0 = g.process_resident_subset(2, [], H * W, H, W)
    assert p0 is None and i0 is None
    g.sync()
    assert [g.export_stream_state(s) for s in full] == states
    # the next valid step is the reference's
    L = [0, 4, 9, 15]
    p, i = g.process_resident_subset(2, L, H * W, H, W)
    for j, s in enumerate(L):
        assert i[j].status == 0 and i[j].scan_index == ks[s]
        assert_records_equal(record_of(g, s, p[j], i[j]), ref[ks[s]][s], ("after the refusals", s))
    g.close()


# ---- 7. continuous batching with idle slots sitting out ----------------------------------------------------------------------------
def test_continuous_batching_sit_out(synth, monkeypatch):
    """test_gpu_stream_state.test_continuous_batching's configuration (24 logs of 6 .. 15 scans through 16 slots): with sit_out the
    same poses to the bit, and the GPU processes exactly the scans that count."""
    set_env(monkeypatch, {})
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import batch_logs
    finally:
        sys.path.pop(0)
    H, W, lt, R, epr, P = SMALL
    S, N = 16, 24
    lo, hi = 6, P + 3 * HB_PERIOD + 2
    lengths = [lo + (i * (hi - lo)) // (N - 1) for i in range(N)]
    lengths = [lengths[(7 * i) % N] for i in range(N)]
    cfg = synth.make_cfg(H, W, 0)
    logs = [[synth.scan(cfg, 100 + i, k)[0] for k in range(lengths[i])] for i in range(N)]
    res = {}
    for sit_out in (False, True):
        g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                      la.make_config(n_streams=S, max_points=H * W, max_width=W))
        res[sit_out] = batch_logs.run(g, logs, H, W, sit_out=sit_out)
        subset = int(g.modes()["subset_steps"])
        g.close()
        assert res[sit_out]["status_bits"] == 0 and res[sit_out]["scans"] == sum(lengths)
        assert (subset > 0) == sit_out
    a, b = res[False], res[True]
    assert a["steps"] == b["steps"] and a["slot_of_log"] == b["slot_of_log"]
    assert a["gpu_scans"] == a["steps"] * S and b["gpu_scans"] == sum(lengths) < a["gpu_scans"]
    for i in range(N):
        assert a["poses"][i].shape == (lengths[i], 7) and bits(a["poses"][i]) == bits(b["poses"][i]), ("log", i)
