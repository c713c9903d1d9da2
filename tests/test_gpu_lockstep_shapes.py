"""Lock-step batches (n_streams >= 16) at the VLP-16 and Ouster-128 shapes of bench.py's WORKLOADS, checked against the CPU oracle
directly, and the cell hash tables of the incremental hash (k_hash_build every kHbPeriod-th scan, k_hash_append in between —
kernels_rebuild.h) switching between LDS and global per stream inside one lock-step launch.

These shapes reach code that the 16 x 900 and 64 x 1800 batches never run:
  * VLP-16: k_ring_split_lb at 16 x 1800 (ring pitch 2032), 168 pick slots per ring, the incremental hash with P = 10 on a
    65 536-slot table.  The handle has 32 streams: launch_extract takes the look-back split only for launches of more workgroups
    than the all-resident k_ring_split may hold (ring_split_max_wgs, at most 256), and 16 streams of 15 tiles are 240 — the
    32-stream launch's 480 take k_ring_split_lb, as bench.py's 256-stream batched leg does;
  * Ouster-128: organised clouds split row by row by k_row_compact across 16 streams (lidar_type 1: neither ring split runs), the
    one-workgroup solve at an edge capacity of 11 264, and a ragged stream whose window occupies more than kLdsCellsMax = 6144
    one-metre cells — it falls back to the global table (hash_build_global) while the regular streams of the same launch stay on
    their LDS tables;
  * scans of more than edge_cap / 2 edges: k_knn8's workgroups walk their second query block (the grid is half the blocks).
Every test proves from the handle's modes, the GPU's own local maps, edge counts and counters that its path ran.  Run with -m gpu
on an MI355X."""
import collections
import hashlib
import os

import numpy as np
import pytest

import liodom_amd as la
from test_gpu_parity import _assert_batch_runs_equal, assert_edges_equal, rot_angle

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-4     # metres
POSE_TOL_R = 1e-4     # radians
HB_PERIOD = 4         # kHbPeriod: a lock-step launch rebuilds every stream on steps 0, 4, 8, ... and appends in between
LDS_CELLS_MAX = 6144  # kLdsCellsMax: a rebuild whose window occupies more cells builds the global table
TILE_PTS = 2048       # kTilePts: points per workgroup of the ring splits
SHAPES = {
    # name: H, W, lidar_type, R, epr, P (bench.py WORKLOADS)
    "vlp16": (16, 1800, 0, 8, 20, 10),
    "ouster128": (128, 2048, 1, 8, 10, 30),
}
STREAMS = {"vlp16": 32, "ouster128": 16}        # lock-step handles (>= 16 streams); see the module docstring for 32
SPLIT = {"vlp16": "k_ring_split_lb", "ouster128": "k_row_compact"}


def split_kernel(modes, H, W, lidar_type, n_streams):
    """The ring split launch_extract runs for a launch of all n_streams streams of this handle (max_points = H * W)."""
    if lidar_type == 1:
        return "k_row_compact"                  # organised cloud: ring = row
    fits = -(-H * W // TILE_PTS) * n_streams <= int(modes["ring_split_max_wgs"]) and modes["ring_split"] == "1"
    if modes["ring_split_lb"] == "1" and not fits:
        return "k_ring_split_lb"
    return "k_ring_split" if fits else "k_classify + k_ring_scatter"


def device_edge_cap(H, R, epr):
    # liodom_create: one slot per pick of every region of every ring, rounded up to 64
    return -(-H * R * (epr + 1) // 64) * 64


def device_table_size(H, R, epr, P):
    # liodom_create's doubling rule: the smallest power of two from 1024 up that holds twice the window's capacity
    ts = 1024
    while ts < 2 * device_edge_cap(H, R, epr) * P:
        ts <<= 1
    return ts


def cell_count(win):
    """Occupied 1 m cells of a window as k_hash_build counts them: floor of the float32 coordinates (kCellInv = 1) of the points
    that pass point_ok (|x|, |y|, |z| < 1e9)."""
    p = win[:, :3]
    c = np.floor(p[np.all(np.abs(p) < 1e9, axis=1)]).astype(np.int64) + (1 << 20)
    return len(np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]))


def predicted_hash_counters(cells, cells_max, incr=True):
    """(hash_rebuilds, hash_appends) of a stream whose window after step k occupies cells[k] cells.  Both count LDS work only
    (kernels_rebuild.h: k_hash_build's LDS path, k_hash_append's append path).  A rebuild bins the window after its step and is
    an LDS rebuild iff that window occupies at most cells_max cells; the appends up to the next rebuild follow its table kind
    (a global table has no room: k_hash_append rebuilds it globally).  incr=False: a rebuild on every step."""
    rebuilds = appends = 0
    lds = False
    for k, n in enumerate(cells):
        if not incr or k % HB_PERIOD == 0:
            lds = n <= cells_max
            rebuilds += int(lds)
        else:
            appends += int(lds)
    return rebuilds, appends


def scans_of(synth, shape, stream, K, noise_sigma=0.01, ragged=lambda k: False):
    H, W, lt = SHAPES[shape][:3]
    cfg = synth.make_cfg(H, W, lt, noise_sigma=noise_sigma)
    out = []
    for k in range(K):
        x = synth.scan(cfg, stream, k)[0]
        out.append(synth.ragged(x, H, W, lt, seed=100 + k) if ragged(k) else x)
    return out


def set_env(monkeypatch, env):
    for name in [n for n in os.environ if n.startswith("LIODOM_")]:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


Record = collections.namedtuple("Record", "pose n_edges map_points matches lm edges corr")
Replay = collections.namedtuple("Replay", "out cells n_edges modes worst records")


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def assert_records_equal(a, b, what):
    """Two per-stream step records (Record) bit-identical field by field."""
    for field in Record._fields:
        assert getattr(a, field) == getattr(b, field), (what, field)


def lockstep_replay(orc, dims, data, env, want_modes, want_split, monkeypatch, oracle=(), track=(), next_slot=False):
    """Replays data[s] (scan k of handle stream s: data[s][k]) on a handle of len(data) streams of shape dims = (H, W, lidar_type,
    R, epr, P) under `env`, every step one process_resident launch over all streams; with next_slot that launch also issues the
    next step's extraction, as bench.py's batched leg does.  The handle's modes must hold want_modes and its ring split must be
    want_split (split_kernel on the handle's modes).
    Per step and stream: status 0, and a Record — pose bits, n_edges, map_points, match counts, LM iterations and terminations of
    both passes, digests of get_edges and of both passes' correspondences; streams that replay the same sequence object have
    equal records.  After the run every stream's pose log equals its steps' readbacks, scan_index k on step k.
    Streams in `oracle` against the oracle: edges bit-equal to orc.extract, n_edges and map_points equal, both passes' valid flags
    and line-point indices exactly equal to the oracle's loop (laser_odometry.cc:320-361) on the GPU's own queries and the local
    map the step searched, match counts, LM iterations and terminations equal to orc.Odometer's, pose within 1e-4 m / 1e-4 rad.
    Returns a Replay: out (per step: poses, match counts of every stream, both passes' correspondences of the streams in
    `track` — _assert_batch_runs_equal's layout), cells[k, j] (cells of the window of stream track[j] after step k: what a
    rebuild on step k bins), n_edges[k, j], the modes after the run (stream 0's hash_* counters), the worst pose errors against
    the oracle and records[k][s]."""
    H, W, lt, R, epr, P = dims
    N, S, K = H * W, len(data), len(data[0])
    track, oracle = list(track), list(oracle)
    seen = sorted(set(track) | set(oracle))
    set_env(monkeypatch, env)
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1)
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(n_streams=S, max_points=N, max_width=W, debug_buffers=1, pose_log_capacity=K + 8))
    modes = g.modes()
    for key, val in want_modes.items():
        assert modes[key] == val, (dims, S, env, key, modes)
    assert split_kernel(modes, H, W, lt, S) == want_split, (dims, S, env, modes)
    g.alloc_resident(K)
    for s in range(S):
        for k in range(K):
            g.upload_scan(s, k, data[s][k])
    first = {}                                          # streams replaying one sequence object: their first stream
    for s in range(S):
        first.setdefault(id(data[s]), s)
    ods = {s: orc.Odometer(po) for s in oracle}
    out, records, readback = [], [], []
    cells = np.zeros((K, len(track)), np.int64)
    n_edges = np.zeros((K, len(track)), np.int64)
    worst_t = worst_r = 0.0
    maps = {s: g.local_map(s)[0] for s in seen}         # what the next step's kNN passes search, per checked stream
    for k in range(K):
        poses, infos = g.process_resident(k, N, H, W, readback=True, next_slot=(k + 1 if next_slot and k + 1 < K else -1))
        readback.append((poses.copy(), [bytes(i) for i in infos]))
        recs, corr, edges = [], {}, {}
        for s in range(S):
            what = (dims, S, env, "step", k, "stream", s)
            ig = infos[s]
            assert ig.status == 0, (what, ig.status)
            c = [tuple(a.copy() for a in g.correspondences(it, stream=s)) for it in (0, 1)]
            e = g.get_edges(s)
            recs.append(Record(poses[s].view(np.uint64).tobytes(), ig.n_edges, ig.map_points, tuple(ig.matches),
                               tuple((t.iterations, t.termination) for t in ig.lm),
                               digest(e["edges"].view(np.uint32), e["ring"], e["idx_in_ring"], e["src"]),
                               tuple(digest(*ci) for ci in c)))
            assert_records_equal(recs[s], recs[first[id(data[s])]], what)      # equal data, equal bits
            if s in seen:
                corr[s], edges[s] = c, e
        for s in oracle:
            what = (dims, S, env, "step", k, "stream", s)
            ig = infos[s]
            o = orc.extract(po, data[s][k], H, W)
            assert_edges_equal(edges[s], o)
            pose_o, info_o = ods[s].step(o["edges"])
            assert ig.n_edges == info_o.n_edges, what
            dt = np.linalg.norm(poses[s][4:] - pose_o[4:])
            dr = rot_angle(poses[s][:4], pose_o[:4])
            worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
            assert dt <= POSE_TOL_T and dr <= POSE_TOL_R, (what, dt, dr)
            if k == 0:
                continue
            assert ig.map_points == info_o.map_points, what
            for it in (0, 1):
                vg, ag, bg = corr[s][it]
                vk, ak, bk = orc.match_edges(po, maps[s], g.knn_queries(it, stream=s))
                assert np.array_equal(vk, vg) and np.array_equal(ak, ag) and np.array_equal(bk, bg), \
                    "%s pass %d: kNN / line gate differ from the oracle on identical inputs at edges %s" % (
                        what, it, np.nonzero((vk != vg) | (ak != ag) | (bk != bg))[0][:10])
                assert ig.matches[it] == int(vk.sum()), (what, it)
                assert ig.lm[it].iterations == info_o.lm[it].iterations, (what, it)
                assert ig.lm[it].termination == info_o.lm[it].termination, (what, it)
        maps = {s: g.local_map(s)[0] for s in seen}
        for j, s in enumerate(track):
            cells[k, j] = cell_count(maps[s])
            n_edges[k, j] = infos[s].n_edges
        out.append((poses.copy(), [tuple(i.matches) for i in infos], [corr[s] for s in track]))
        records.append(recs)
    g.sync()
    for s in range(S):
        lp, li = g.pose_log(s, 0, K)
        for k in range(K):
            assert np.array_equal(lp[k].view(np.uint64), readback[k][0][s].view(np.uint64)), (dims, S, env, "pose log", k, s)
            assert bytes(li[k]) == readback[k][1][s] and li[k].scan_index == k, (dims, S, env, "info log", k, s, li[k].scan_index)
    modes = g.modes()
    g.close()
    return Replay(out, cells, n_edges, modes, (worst_t, worst_r), records)


def replay_shape(orc, shape, data, env, want_modes, monkeypatch, check_oracle):
    """lockstep_replay of `data` (per data stream d: data[d][k]) at SHAPES[shape] on STREAMS[shape] streams, handle stream s
    replaying data stream s % D; streams 0 .. D-1 tracked and, with check_oracle, checked against the oracle."""
    S, D = STREAMS[shape], len(data)
    return lockstep_replay(orc, SHAPES[shape], [data[s % D] for s in range(S)], env, want_modes, SPLIT[shape], monkeypatch,
                           oracle=range(D) if check_oracle else (), track=range(D))


def report(name, cells, n_edges, cap):
    print("%s: cells at the rebuilds %s; most edges %s of %d" % (
        name, [list(map(int, r)) for r in cells[::HB_PERIOD].T], list(map(int, n_edges.max(axis=0))), cap))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_lockstep_batch_against_the_oracle(orc, synth, monkeypatch, shape):
    """The batched kernels of bench.py's vlp16 / ouster128 workloads — k_knn8 + k_line_gate, the incremental cell hash, the
    one-workgroup k_lm_solve, the lock-step extraction (k_ring_split_lb at VLP-16 on 32 streams, k_row_compact at Ouster-128
    on 16) — against the oracle (lockstep_replay), per stream and step, for P + 3
    rebuild periods + 2 scans: the window fills, evicts, and is rebuilt at least three more times.  Data streams: ragged stream
    1003 (on handle stream 0, whose counters modes() reports), synthetic streams 1000 and 1001, and 1002 — with 3 cm range noise
    at VLP-16.  At VLP-16 the ragged and the noisy stream exceed edge_cap / 2 = 1344 edges, and every window stays far below
    kLdsCellsMax; at Ouster-128 the ragged stream exceeds 5632 edges and, from the rebuild of step 12 on, kLdsCellsMax cells,
    while the regular streams of the same launch stay below it at every rebuild (stream 1000 peaks at ~6180 cells on step 29,
    between two rebuilds)."""
    H, W, lt, R, epr, P = SHAPES[shape]
    K = P + 3 * HB_PERIOD + 2
    cap = device_edge_cap(H, R, epr)
    data = [scans_of(synth, shape, 1003, K, ragged=lambda k: True),
            scans_of(synth, shape, 1000, K),
            scans_of(synth, shape, 1001, K),
            scans_of(synth, shape, 1002, K, noise_sigma=0.03 if shape == "vlp16" else 0.01)]
    want = {"knn8": "1", "hash_incr": "1", "hash_build": "lds", "line_gate_kernel": "1", "lm_groups": "1",
            "ring_split_lb": "1" if lt == 0 else "0", "table_size": str(device_table_size(H, R, epr, P))}
    _, cells, n_edges, modes, (wt, wr), _ = replay_shape(orc, shape, data, {}, want, monkeypatch, check_oracle=True)
    report(shape, cells, n_edges, cap)
    assert wt < 1e-6 and wr < 1e-6, (wt, wr)
    # the paths ran: k_knn8's second query block; stream 0's table kinds as its counters tell; at Ouster one launch on both tables
    assert n_edges.max() > cap // 2, (n_edges.max(axis=0), cap)
    assert (int(modes["hash_rebuilds"]), int(modes["hash_appends"])) == predicted_hash_counters(cells[:, 0], LDS_CELLS_MAX), \
        (modes, cells[::HB_PERIOD, 0])
    lds = cells[::HB_PERIOD] <= LDS_CELLS_MAX
    if shape == "ouster128":
        assert (lds.any(axis=1) & ~lds.all(axis=1)).any(), cells[::HB_PERIOD]
    else:
        assert lds.all(), cells[::HB_PERIOD]


def test_lockstep_cell_hash_table_kind_transitions(orc, synth, monkeypatch):
    """LDS -> global -> LDS table switches of single streams in a lock-step batch with the incremental hash on: VLP-16 with the LDS
    table's limit lowered to 2140 cells (LIODOM_LDS_CELLS_MAX).  Handle stream 0 replays stream 1001 ragged while its first window
    fills and regular after (its window rises above the limit and falls below it once the ragged frames are evicted), 1: regular
    stream 1000 (stays below), 2: stream 1002 ragged throughout (above once the window is full), 3: stream 1003 with 3 cm range
    noise (rises across the limit).  The GPU's own windows must show exactly that at the rebuilds, 30 cells clear of the limit, so
    that the test cannot pass without the switches.  The same replay with a rebuild every scan (LIODOM_HASH_INCR=0) and with the
    three-kernel global build (LIODOM_HASH_BUILD=global: no LDS table, no incremental hash) must give bit-identical poses, match
    counts and correspondences of both passes; the default run meets test_lockstep_batch_against_the_oracle's bar."""
    shape = "vlp16"
    H, W, lt, R, epr, P = SHAPES[shape]
    K = P + 3 * HB_PERIOD + 2
    cap = device_edge_cap(H, R, epr)
    limit, margin = 2140, 30      # (at 2000, stream 1001's window at the rebuild of step 4 holds 1992 cells: inside the margin)
    data = [scans_of(synth, shape, 1001, K, ragged=lambda k: k < P),
            scans_of(synth, shape, 1000, K),
            scans_of(synth, shape, 1002, K, ragged=lambda k: True),
            scans_of(synth, shape, 1003, K, noise_sigma=0.03)]
    env = {"LIODOM_LDS_CELLS_MAX": str(limit)}
    want = {"knn8": "1", "hash_incr": "1", "hash_build": "lds", "table_size": str(device_table_size(H, R, epr, P))}
    base, cells, n_edges, modes, (wt, wr), _ = replay_shape(orc, shape, data, env, want, monkeypatch, check_oracle=True)
    report("vlp16, limit %d" % limit, cells, n_edges, cap)
    assert wt < 1e-6 and wr < 1e-6, (wt, wr)
    assert n_edges.max() > cap // 2, (n_edges.max(axis=0), cap)
    reb = np.arange(0, K, HB_PERIOD)
    rc = cells[reb]
    # every rebuild of every checked stream at least `margin` cells from the limit: the table kinds below do not hang on a few cells
    assert (np.abs(rc - limit) >= margin).all(), rc.T
    high = rc > limit                                   # global table for the period this rebuild starts
    # stream 0: LDS, then global, then LDS again — one run of global periods with LDS periods before and after it
    g0 = np.flatnonzero(high[:, 0])
    assert len(g0) and g0[0] > 0 and g0[-1] < len(reb) - 1 and (np.diff(g0) == 1).all(), rc[:, 0]
    assert not high[:, 1].any(), rc[:, 1]
    assert not high[0, 2] and high[reb >= P - 1, 2].all(), rc[:, 2]
    assert not high[0, 3] and high[-1, 3], rc[:, 3]
    rebuilds, appends = predicted_hash_counters(cells[:, 0], limit)
    assert 0 < rebuilds < len(reb) and appends > 0
    assert (int(modes["hash_rebuilds"]), int(modes["hash_appends"])) == (rebuilds, appends), (modes, rc[:, 0])
    for extra, want2 in (({"LIODOM_HASH_INCR": "0"}, {"knn8": "1", "hash_incr": "0", "hash_build": "lds"}),
                         ({"LIODOM_HASH_BUILD": "global"}, {"knn8": "1", "hash_incr": "0", "hash_build": "global"})):
        env2 = dict(env, **extra)
        other, cells2, _, modes2, _, _ = replay_shape(orc, shape, data, env2, want2, monkeypatch, check_oracle=False)
        _assert_batch_runs_equal(base, other, env2)
        assert np.array_equal(cells, cells2), env2
        # (a rebuild on every step: one LDS rebuild per step whose window fits the limit; the global build counts nothing)
        want_counters = predicted_hash_counters(cells[:, 0], limit, incr=False) if want2["hash_build"] == "lds" else (0, 0)
        assert (int(modes2["hash_rebuilds"]), int(modes2["hash_appends"])) == want_counters, (env2, modes2)
