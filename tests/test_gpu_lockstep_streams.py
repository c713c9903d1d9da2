"""The incremental cell hash of lock-step handles (n_streams >= 16: k_hash_build every kHbPeriod-th scan of a stream, k_hash_append
in between — kernels_rebuild.h) off the lock-step path and at the limits of its point array.

(1) Streams of one lock-step handle stepped one at a time (liodom_process_scan, liodom_odometry_step — INTEGRATION.md) and at
    different rates, mixed with lock-step liodom_process_resident steps: every stream must keep its own rebuild period.  Per step
    and stream: pose within 1e-4 m / 1e-4 rad of orc.Odometer fed the same scans, map size, LM iteration counts and terminations
    equal to the oracle's, both passes' correspondences exactly equal to the oracle's loop (laser_odometry.cc:320-361) on the
    GPU's own queries and local map — an evicted frame's point left live in the table shows up there —, and the whole schedule
    bit-identical to a rebuild every scan (LIODOM_HASH_INCR=0).
(2) The room k_hash_build grants every cell (LIODOM_HB_SLACK) must stay in front of the spill list at the end of the point array.

Two shapes with P = 5 > kHbPeriod: A's table has exactly kLdsSlots = 8192 slots (the LDS table's mask and the global table's
agree), B's has 16384.  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

import liodom_amd as la

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-4   # metres
POSE_TOL_R = 1e-4   # radians
S = 16              # the smallest lock-step handle
SHAPES = {
    # name: H, W, R, epr, P, table slots
    "A": (16, 900, 4, 10, 5, "8192"),
    "B": (16, 900, 6, 10, 5, "16384"),
}
KNOBS = ("LIODOM_KNN8", "LIODOM_KNN_EXACT_ONLY", "LIODOM_KNN_SAVE", "LIODOM_HASH_INCR", "LIODOM_HB_SLACK", "LIODOM_HB_NEW_ROOM")


def rot_angle(qa, qb):
    d = abs(float(np.dot(qa, qb)) / (np.linalg.norm(qa) * np.linalg.norm(qb)))
    return 2.0 * np.arccos(min(1.0, d))


def mk(orc, H, W, R, epr, P, S=1, debug=0, **cfgkw):
    po = orc.make_params(lidar_type=0, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1)
    pg = la.make_params(lidar_type=0, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P)
    cg = la.make_config(n_streams=S, max_points=H * W, max_width=W, debug_buffers=debug, **cfgkw)
    return po, la.Liodom(pg, cg)


def set_env(monkeypatch, env):
    for name in set(KNOBS) | {n for n in os.environ if n.startswith("LIODOM_")}:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


def open_handle(orc, shape, env, monkeypatch):
    H, W, R, epr, P, slots = SHAPES[shape]
    set_env(monkeypatch, env)
    po, g = mk(orc, H, W, R, epr, P, S=S, debug=1)
    modes = g.modes()
    assert modes["knn8"] == "1" and modes["hash_build"] == "lds" and modes["table_size"] == slots, modes
    assert modes["hash_incr"] == ("0" if env.get("LIODOM_HASH_INCR") == "0" else "1"), modes
    return po, g, modes


def check_step(orc, po, g, s, info, pose, od, local_map, x, H, W, what):
    """One step of stream s against the oracle: od is fed the same scan; local_map is what the step searched."""
    o = orc.extract(po, x, H, W)
    first = od.window_frames() == 0
    pose_o, info_o = od.step(o["edges"])
    assert info.n_edges == info_o.n_edges, what
    dt = np.linalg.norm(pose[4:] - pose_o[4:])
    dr = rot_angle(pose[:4], pose_o[:4])
    assert dt <= POSE_TOL_T and dr <= POSE_TOL_R, (what, dt, dr)
    if first:
        return
    assert info.map_points == info_o.map_points, what
    for it in (0, 1):
        vg, ag, bg = g.correspondences(it, stream=s)
        vk, ak, bk = orc.match_edges(po, local_map, g.knn_queries(it, stream=s))
        assert np.array_equal(vk, vg) and np.array_equal(ak, ag) and np.array_equal(bk, bg), \
            "%s pass %d: kNN / line gate differ from the oracle on identical inputs at edges %s" % (
                what, it, np.nonzero((vk != vg) | (ak != ag) | (bk != bg))[0][:10])
        assert info.matches[it] == int(vk.sum()), (what, it)
        assert info.lm[it].iterations == info_o.lm[it].iterations, (what, it)
        assert info.lm[it].termination == info_o.lm[it].termination, (what, it)


def replay_schedule(orc, synth, shape, schedule, env, monkeypatch, check_oracle):
    """Runs `schedule` on a 16-stream handle: ("lock",) steps every stream through process_resident, ("scan", s) steps stream s through
    process_scan, ("step", s) through odometry_step with the oracle's edges.  Stream s replays synthetic stream 50 + s in order, one
    scan per step of its own.  The streams named by single-stream steps (and stream 15, stepped in lock-step only) are recorded —
    pose bits, match counts, both passes' correspondences — and, with check_oracle, checked against the oracle.  Returns the
    records and the handle's modes after the run (stream 0's hash_* counters)."""
    H, W = SHAPES[shape][:2]
    po, g, _ = open_handle(orc, shape, env, monkeypatch)
    cfg = synth.make_cfg(H, W, 0)
    tracked = sorted({op[1] for op in schedule if op[0] != "lock"} | ({S - 1} if ("lock",) in schedule else set()))
    ods = {s: orc.Odometer(po) for s in tracked}
    n = [0] * S
    g.alloc_resident(1)
    records = []
    for j, op in enumerate(schedule):
        stepped = list(range(S)) if op[0] == "lock" else [op[1]]
        scans = {s: synth.scan(cfg, 50 + s, n[s])[0] for s in stepped}
        maps = {s: g.local_map(s)[0] for s in stepped if s in tracked} if check_oracle else {}
        if op[0] == "lock":
            for s in stepped:
                g.upload_scan(s, 0, scans[s])
            poses, infos = g.process_resident(0, H * W, H, W, readback=True)
            out = {s: (poses[s].copy(), infos[s]) for s in stepped}
        elif op[0] == "scan":
            out = {op[1]: g.process_scan(scans[op[1]], H, W, stream=op[1])}
        else:
            out = {op[1]: g.odometry_step(orc.extract(po, scans[op[1]], H, W)["edges"], stream=op[1])}
        for s in stepped:
            pose, info = out[s]
            what = "%s step %d (%s) stream %d, its scan %d" % (shape, j, op[0], s, n[s])
            assert info.status == 0, (what, info.status)
            if s in tracked:
                if check_oracle:
                    check_step(orc, po, g, s, info, pose, ods[s], maps[s], scans[s], H, W, what)
                corr = [tuple(a.copy() for a in g.correspondences(it, stream=s)) for it in (0, 1)]
                records.append((what, pose.view(np.uint64).copy(), tuple(info.matches), corr))
            n[s] += 1
    g.sync()
    modes = g.modes()
    g.close()
    assert n[0] >= SHAPES[shape][4] + 8, n      # the most irregular stream (0) evicts frames for several periods
    return records, modes


def assert_records_equal(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x[0] == y[0], what
        assert np.array_equal(x[1], y[1]), (what, x[0], "pose")
        assert x[2] == y[2], (what, x[0], "matches")
        for it in (0, 1):
            assert all(np.array_equal(p, q) for p, q in zip(x[3][it], y[3][it])), (what, x[0], "correspondences", it)


def _alternating():
    # (a) one lock-step step, then streams 0 and 1 alternately through process_scan
    return [("lock",)] + [("scan", i % 2) for i in range(26)]


def _rates_1_2_3():
    # (b) streams 0, 1, 2 at rates 1 : 2 : 3 — stream 0 comes every 6th call, which a handle-wide period of 4 never rebuilds
    return [("scan", s) for _ in range(13) for s in (2, 1, 2, 0, 2, 1)]


def _late_start():
    # (c) stream 0's first step after 11 steps of the others (its first step fell on an append of a handle-wide period)
    return [("scan", 1 + i % 2) for i in range(11)] + [("scan", s) for _ in range(7) for s in (0, 1, 0, 2)]


def _mixed():
    # (d) lock-step steps between single-stream process_scan and odometry_step calls
    return [op for _ in range(5) for op in (("lock",), ("scan", 0), ("step", 1), ("step", 0), ("scan", 2))]


SCHEDULES = {"alternating": _alternating, "rates_1_2_3": _rates_1_2_3, "late_start": _late_start, "mixed": _mixed}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("shape", ["A", "B"])
def test_streams_stepped_one_at_a_time(orc, synth, monkeypatch, shape, schedule):
    """Finding: the rebuild-or-append choice was made for the whole handle while the table state is per stream — a stream stepped
    alone could go without a rebuild for good (evicted frames' points stayed live in k_knn8, the spill list overflowed silently) or
    start with an append into the freshly initialised table (shape A)."""
    sched = SCHEDULES[schedule]()
    assert len(sched) >= 24
    incr, modes = replay_schedule(orc, synth, shape, sched, {}, monkeypatch, check_oracle=True)
    assert int(modes["hash_appends"]) > 0 and int(modes["hash_rebuilds"]) > 1, modes      # (stream 0's counters)
    full, _ = replay_schedule(orc, synth, shape, sched, {"LIODOM_HASH_INCR": "0"}, monkeypatch, check_oracle=False)
    assert_records_equal(incr, full, (shape, schedule, "LIODOM_HASH_INCR=0"))


def lockstep_run(orc, synth, scans, env, monkeypatch):
    """Shape B in lock-step (stream s replays scans[s % D]): per step the poses, match counts and both passes' correspondences of
    streams 0 .. D-1, checked against the oracle's loop on the GPU's own queries and local map; the window of stream 0 after the
    first step (what the first k_hash_build binned); the modes after the run."""
    H, W = SHAPES["B"][:2]
    D, K = len(scans), len(scans[0])
    po, g, _ = open_handle(orc, "B", env, monkeypatch)
    g.alloc_resident(K)
    for s in range(S):
        for k in range(K):
            g.upload_scan(s, k, scans[s % D][k])
    out, win0 = [], None
    for k in range(K):
        maps = [g.local_map(d)[0] for d in range(D)]
        poses, infos = g.process_resident(k, H * W, H, W, readback=True)
        assert all(i.status == 0 for i in infos), (env, k, [i.status for i in infos])
        corr = [[tuple(a.copy() for a in g.correspondences(it, stream=d)) for it in (0, 1)] for d in range(D)]
        if k == 0:
            win0 = g.window(0)[0]
        else:
            for d in range(D):
                for it in (0, 1):
                    vk, ak, bk = orc.match_edges(po, maps[d], g.knn_queries(it, stream=d))
                    vg, ag, bg = corr[d][it]
                    assert np.array_equal(vk, vg) and np.array_equal(ak, ag) and np.array_equal(bk, bg), \
                        (env, k, d, it, np.nonzero((vk != vg) | (ak != ag) | (bk != bg))[0][:10])
        out.append(("step %d" % k, poses[:D].view(np.uint64).copy(), [tuple(i.matches) for i in infos[:D]], corr))
    g.sync()
    modes = g.modes()
    g.close()
    return out, win0, modes


def _assert_lockstep_runs_equal(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x[1], y[1]), (what, x[0], "poses")
        assert x[2] == y[2], (what, x[0], "matches")
        for cx, cy in zip(x[3], y[3]):
            for it in (0, 1):
                assert all(np.array_equal(p, q) for p, q in zip(cx[it], cy[it])), (what, x[0], "correspondences", it)


def test_rebuild_slack_stays_clear_of_the_spill_list(orc, synth, monkeypatch):
    """Finding: k_hash_build granted every cell room beyond its population (hash_cell_slack) when 2M + slack * cells fitted the whole
    point array, spill list included — its cells could then reach into the places k_hash_append's spill writes go.  The window of
    the first rebuild (one frame: few points over many cells) decides the slack that reaches that far; the replay under that
    LIODOM_HB_SLACK and under the largest slack that stays clear must equal a rebuild every scan."""
    H, W = SHAPES["B"][:2]
    K, D = 12, 2
    cfg = synth.make_cfg(H, W, 0)
    scans = [[synth.scan(cfg, 60 + d, k)[0] for k in range(K)] for d in range(D)]
    _, g, modes = open_handle(orc, "B", {}, monkeypatch)      # (the point array's layout of an incremental handle)
    g.close()
    sorted_cap, spill_base = int(modes["sorted_cap"]), int(modes["hb_spill_base"])
    assert 0 < spill_base < sorted_cap
    # the window does not depend on the hash mode: a rebuild every scan is the dry run and the reference at once
    ref, win0, _ = lockstep_run(orc, synth, scans, {"LIODOM_HASH_INCR": "0"}, monkeypatch)
    M = len(win0)
    keys = np.floor(win0[:, :3]).astype(np.int64)           # (1 m cells: pack_cell of floor(x * kCellInv), kCellInv = 1)
    _, cnt = np.unique(keys, axis=0, return_counts=True)
    U = len(cnt)

    def alloc(slack):       # places k_hash_build allocates with this slack: every cell max(population, slack)
        return M + int(np.maximum(cnt, slack).sum())

    s_over = (sorted_cap - 2 * M) // U                       # the largest slack the bound against the whole array grants
    s_clear = (spill_base - 2 * M) // U                      # the largest slack the bound against the spill list grants
    assert s_over > s_clear >= 1, (M, U, s_over, s_clear)
    assert alloc(s_over) > spill_base, (M, U, s_over, alloc(s_over), spill_base)       # the cells reach into the spill list
    assert alloc(s_clear) <= spill_base, (M, U, s_clear, alloc(s_clear), spill_base)
    for slack in (s_over, s_clear):
        out, _, m = lockstep_run(orc, synth, scans, {"LIODOM_HB_SLACK": str(slack)}, monkeypatch)
        _assert_lockstep_runs_equal(ref, out, ("LIODOM_HB_SLACK", slack))
        assert int(m["hash_appends"]) > 0 and int(m["hash_rebuilds"]) > 1, (slack, m)
        if slack == s_over:
            assert int(m["hash_points_spilled"]) > 0, m        # spill writes did happen
