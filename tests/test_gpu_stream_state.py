"""Streams with a life of their own: liodom_reset_stream, liodom_export_stream_state, liodom_import_stream_state
(include/liodom_hip.h, csrc/kernels_state.h, layout in csrc/stream_state_format.h) on one-stream, few-stream (streamed rebuild) and lock-step (LDS-built table, k_knn8,
incremental cell hash) handles.

  1. one stream of a handle is reset while the others go on: the others are bit-identical to the run without the reset, the reset
     stream to the same stream of a fresh handle;
  2. export after n scans, a NEW handle, import, go on: bit-identical to the uninterrupted run (poses, step infos, scan_index,
     windows; with filter_local_map, mapping, pose_covariance; one-stream handles in chain mode through liodom_replay_resident);
     and import into a slot of the same RUNNING handle that has a log of its own behind it: bit-identical to the exporting stream;
  3. a stream moves between handle shapes (3 <-> 1 streams: bit-identical; 16 <-> 1: 1e-9, the bound
     test_sixteen_lockstep_streams_match_single_stream uses for that pair, whose solves sum in a different order);
  4. a lock-step run with an export / import and a reset in the middle, against the CPU oracle directly;
  5. continuous batching (tools/batch_logs.py): 24 logs of unequal length through 16 slots, every log bit-identical to its replay
     from scan 0 on a fresh handle;
  6. refusals leave the handle untouched.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
from test_gpu_lockstep_streams import check_step

pytestmark = pytest.mark.gpu

HB = 4                                  # kHbPeriod
DIMS = (16, 900, 0, 6, 10, 5)           # H, W, lidar_type, R, epr, P: the shape of test_sixteen_lockstep_streams_match_single_stream
VLP16 = (16, 1800, 0, 8, 20, 10)        # a chain-mode shape (test_chain_mode_replay_against_the_oracle)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clean_env(monkeypatch):
    for name in [n for n in os.environ if n.startswith("LIODOM_")]:
        monkeypatch.delenv(name, raising=False)


def open_handle(orc, dims, S=1, debug=0, params=None, **cfgkw):
    H, W, lt, R, epr, P = dims
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1, **(params or {}))
    pg = la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, **(params or {}))
    cg = la.make_config(n_streams=S, max_points=H * W, max_width=W, debug_buffers=debug, **cfgkw)
    return po, la.Liodom(pg, cg)


def info_key(i):
    """Everything of a step info, costs as bits."""
    return (i.n_edges, i.map_points, tuple(i.matches), i.status, i.scan_index,
            tuple((l.iterations, l.accepted, l.termination, np.float64(l.initial_cost).view(np.uint64).item(),
                   np.float64(l.final_cost).view(np.uint64).item()) for l in i.lm))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def load(g, data, K):
    """data[s][k] -> resident slot k of stream s."""
    g.alloc_resident(K)
    for s, log in enumerate(data):
        for k in range(K):
            g.upload_scan(s, k, log[k])


def lock_steps(g, dims, first, last, K, ahead=True, before=None):
    """Lock-step steps first .. last - 1 from the resident slots of the same number (the next step's extraction issued ahead);
    before(k) runs in front of step k.  Returns per step (poses bits per stream, info keys per stream)."""
    H, W = dims[:2]
    out = []
    for k in range(first, last):
        if before:
            before(k)
        poses, infos = g.process_resident(k, H * W, H, W, readback=True, next_slot=(k + 1 if ahead and k + 1 < K else -1))
        out.append(([bits(p) for p in poses], [info_key(i) for i in infos]))
    return out


def windows(g, S):
    return [(bits(w), nf) for w, nf in (g.window(s) for s in range(S))]


def logs_of(synth, dims, streams, K):
    cfg = synth.make_cfg(dims[0], dims[1], dims[2])
    return [[synth.scan(cfg, d, k)[0] for k in range(K)] for d in streams]


# ---- 1. reset of one stream -----------------------------------------------------------------------------------------------------
def _reset_run(orc, dims, data, K, j=None, k0=None, want=None):
    S = len(data)
    _, g = open_handle(orc, dims, S=S)
    if want:
        m = g.modes()
        assert all(m[k] == v for k, v in want.items()), m
    load(g, data, K)
    win_j = []

    def before(k):
        if k > 0 and j is not None:
            win_j.append(windows(g, S)[j])         # stream j's window after step k - 1
        if k == k0:
            g.reset_stream(j)

    steps = lock_steps(g, dims, 0, K, K, before=before)
    wins = windows(g, S)
    win_j.append(wins[j] if j is not None else None)
    g.sync()
    modes = g.modes()
    g.close()
    return steps, wins, win_j, modes


@pytest.mark.parametrize("S", [3, 16])
def test_reset_of_one_stream(orc, synth, monkeypatch, S):
    clean_env(monkeypatch)
    P = DIMS[5]
    K = P + 3 * HB + 2
    j = 1 if S == 3 else 5
    want = {"knn8": "1", "hash_incr": "1", "hash_build": "lds"} if S == 16 else {"early_rebuild": "1"}
    base = logs_of(synth, DIMS, range(S), K)                     # distinct data per stream
    new = logs_of(synth, DIMS, [40], K)[0]
    plain, plain_wins, _, _ = _reset_run(orc, DIMS, base, K, want=want)
    fresh, _, fresh_win_j, _ = _reset_run(orc, DIMS, [new if s == j else base[s] for s in range(S)], K, j=j, want=want)
    for k0 in (2, P, P + HB + 1):
        data = [(base[s][:k0] + new[:K - k0]) if s == j else base[s] for s in range(S)]
        steps, wins, win_j, modes = _reset_run(orc, DIMS, data, K, j=j, k0=k0, want=want)
        for k in range(K):
            for s in range(S):
                if s != j or k < k0:
                    assert steps[k][0][s] == plain[k][0][s] and steps[k][1][s] == plain[k][1][s], (S, k0, k, s)
                else:
                    assert steps[k][0][s] == fresh[k - k0][0][s], (S, k0, k, "pose of the reset stream")
                    assert steps[k][1][s] == fresh[k - k0][1][s], (S, k0, k, "step info of the reset stream")
                    assert steps[k][1][s][4] == k - k0 and steps[k][1][s][3] == 0        # scan_index restarts, status 0
                    assert win_j[k] == fresh_win_j[k - k0], (S, k0, k, "window of the reset stream")
        assert all(wins[s] == plain_wins[s] for s in range(S) if s != j), (S, k0)
        if S == 16:
            assert int(modes["hash_appends"]) > 0, modes


# ---- 2. round trip, same shape --------------------------------------------------------------------------------------------------
def _continue_on_new_handle(orc, dims, S, data, K, n, params=None, before=None, cov=False, **cfgkw):
    """n lock-step steps, export every stream, close; a new handle, import, steps n .. K - 1."""
    _, g = open_handle(orc, dims, S=S, params=params, **cfgkw)
    load(g, data, K)
    head = lock_steps(g, dims, 0, n, K, before=before)
    blobs = [g.export_stream_state(s) for s in range(S)]
    g.import_stream_state(0, blobs[0])
    assert g.export_stream_state(0) == blobs[0], "export -> import into the same stream -> export is not byte-equal"
    g.close()
    for b in blobs:
        st = api.parse_stream_state(b)
        assert st["scan_counter"] == n and st["frame_count"] == n and st["n_frames"] == min(n, dims[5])
    _, g = open_handle(orc, dims, S=S, params=params, **cfgkw)
    load(g, data, K)
    for s in range(S):
        g.import_stream_state(s, blobs[s])
    tail = lock_steps(g, dims, n, K, K, before=before)
    wins = windows(g, S)
    covs = [g.pose_covariance_log(s, n, K - n) for s in range(S)] if cov else None
    g.close()
    return head + tail, wins, covs, blobs


def _cov_bits(recs):
    return [(r["scan_index"], r["flags"], r["n_residuals"], r["termination"], bits(np.array([r["final_cost"], r["sigma2"]])),
             bits(r["information"]), bits(r["covariance"]), bits(r["eigenvalues"]), bits(r["eigenvectors"])) for r in recs]


@pytest.mark.parametrize("S", [3, 16])
def test_round_trip_lockstep(orc, synth, monkeypatch, S):
    clean_env(monkeypatch)
    P = DIMS[5]
    K = P + 3 * HB + 4
    data = logs_of(synth, DIMS, [10 + s for s in range(S)], K)
    _, g = open_handle(orc, DIMS, S=S)
    load(g, data, K)
    ref = lock_steps(g, DIMS, 0, K, K)
    ref_wins = windows(g, S)
    g.close()
    for n in (0, 1, P - 1, P, P + 3 * HB + 1):
        steps, wins, _, _ = _continue_on_new_handle(orc, DIMS, S, data, K, n)
        for k in range(K):
            assert steps[k] == ref[k], (S, n, k, [s for s in range(S) if steps[k][0][s] != ref[k][0][s] or steps[k][1][s] != ref[k][1][s]])
        assert wins == ref_wins, (S, n)


def test_round_trip_one_stream_chain_mode(orc, synth, monkeypatch):
    """One-stream handle, liodom_replay_resident(depth = 1): chain mode, speculative hand-overs."""
    clean_env(monkeypatch)
    H, W, lt, R, epr, P = VLP16
    K = P + 3 * HB + 4
    scans = logs_of(synth, VLP16, [7], K)[0]

    def run(first_count, blob=None):
        _, g = open_handle(orc, VLP16, pose_log_capacity=K + 8)
        load(g, [scans], K)
        if blob is not None:
            g.import_stream_state(0, blob)
        first, count = first_count
        poses, infos = g.replay_resident(first, count, H * W, H, W, depth=1)
        m = g.modes()
        assert m["chain"] == "1" and m["safe_mode"] == "0", m
        # chain_done starts with the first-pass workgroups launched in chain mode since the handle was created or the import (which
        # starts the count over): the scans behind the two warm-up scans of this call did run in chain mode
        launched = int(m["chain_done"].split("/")[0])
        assert (launched > 0) == (count > 2), (first_count, m["chain_done"])
        out = [(bits(poses[i][0]), info_key(infos[i])) for i in range(count)]
        return g, out

    g, ref = run((0, K))
    ref_win = windows(g, 1)
    g.close()
    for n in (0, 1, P - 1, P, P + 3 * HB + 1):      # (K - n >= 3: at least one scan after every import runs in chain mode)
        g, head = run((0, n))
        blob = g.export_stream_state(0)
        g.close()
        g, tail = run((n, K - n), blob)
        assert head + tail == ref, (n, [k for k in range(K) if (head + tail)[k] != ref[k]])
        assert windows(g, 1) == ref_win, n
        log, infos = g.pose_log(0, n, K - n)
        assert [i.scan_index for i in infos] == list(range(n, K)) and [bits(p) for p in log] == [t[0] for t in tail], n
        g.close()


@pytest.mark.parametrize("variant", ["filter_local_map", "pose_covariance"])
def test_round_trip_filtered_map_and_covariance(orc, synth, monkeypatch, variant):
    clean_env(monkeypatch)
    P, S = DIMS[5], 3
    K = P + 6
    data = logs_of(synth, DIMS, [20 + s for s in range(S)], K)
    params = {"filter_local_map": 1} if variant == "filter_local_map" else None
    cfgkw = {"pose_covariance": 1, "pose_log_capacity": 64} if variant == "pose_covariance" else {}
    _, g = open_handle(orc, DIMS, S=S, params=params, **cfgkw)
    load(g, data, K)
    ref = lock_steps(g, DIMS, 0, K, K)
    ref_wins = windows(g, S)
    ref_cov = [_cov_bits(g.pose_covariance_log(s, 0, K)) for s in range(S)] if variant == "pose_covariance" else None
    if variant == "filter_local_map":
        assert g.local_map(0)[1], "the filtered local map never became active"
    g.close()
    for n in (1, P, P + 2):            # P, P + 2: the window is full, the search structure is the VoxelGrid cloud
        steps, wins, covs, _ = _continue_on_new_handle(orc, DIMS, S, data, K, n, params=params, cov=variant == "pose_covariance", **cfgkw)
        assert steps == ref and wins == ref_wins, (variant, n)
        if covs is not None:
            for s in range(S):
                assert _cov_bits(covs[s]) == ref_cov[s][n:], (n, s)


def test_round_trip_mapping(orc, synth, monkeypatch):
    """mapping = 1: the received ~map cloud travels in the blob.  The map is delivered on even scans only, as
    test_external_map_feeds_the_knn_cloud builds it, so that the scans right after an import search the imported one."""
    clean_env(monkeypatch)
    H, W, lt, R, epr, P = 16, 900, 0, 6, 10, 4
    dims = (H, W, lt, R, epr, P)
    K = 14
    scans = logs_of(synth, dims, [0], K)[0]
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1, mapping=1)
    od, mo, hist, loc = orc.Odometer(po), orc.Map(), [], {}
    for k in range(K):
        e = orc.extract(po, scans[k], H, W)["edges"]
        if k > P:
            e_old, T_old = hist[k - P - 1]
            mo.update(e_old, T_old)
            if k % 2 == 0:
                loc[k] = mo.local(hist[-1][1], 2, 1)
                od.set_received_map(loc[k])
        pose_o, _ = od.step(e)
        T = np.eye(4)[:3].copy()
        q = pose_o[:4]
        x, y, z, w = q / np.linalg.norm(q)
        T[:, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        T[:, 3] = pose_o[4:]
        hist.append((e, T))
    assert len(loc) >= 3 and all(len(v) > 0 for v in loc.values())

    def run(g, first, last):
        out = []
        for k in range(first, last):
            if k in loc:
                g.set_received_map(loc[k])
            pose, info = g.process_scan(scans[k], H, W)
            out.append((bits(pose), info_key(info)))
        return out

    _, g = open_handle(orc, dims, params={"mapping": 1}, recv_capacity=65536)
    ref = run(g, 0, K)
    ref_lm = bits(g.local_map()[0])
    g.close()
    for n in (P + 3, P + 5):           # odd scans: no delivery in front of scan n
        assert n not in loc and (n - 1) in loc
        _, g = open_handle(orc, dims, params={"mapping": 1}, recv_capacity=65536)
        head = run(g, 0, n)
        blob = g.export_stream_state(0)
        st = api.parse_stream_state(blob)
        assert st["mapping"] == 1 and len(st["received_map"]) == len(loc[n - 1])
        g.close()
        _, g = open_handle(orc, dims, params={"mapping": 1}, recv_capacity=65536)
        g.import_stream_state(0, blob)
        assert bits(g.received_map()) == bits(st["received_map"])
        tail = run(g, n, K)
        assert head + tail == ref, n
        assert bits(g.local_map()[0]) == ref_lm
        g.close()
    # a map larger than the importing handle's recv_capacity is refused
    _, g = open_handle(orc, dims, params={"mapping": 1}, recv_capacity=8)
    rc = g.L.liodom_import_stream_state(g.h, 0, blob, len(blob))
    assert rc == api.ERR_CAPACITY
    g.close()


@pytest.mark.parametrize("S,variant", [(3, "plain"), (3, "filter_local_map"), (16, "plain")])
def test_import_takes_over_a_running_slot(orc, synth, monkeypatch, S, variant):
    """Stream a's state goes into stream b of the SAME running handle at step n, b having run another log until then (its tables
    — both of a streamed-rebuild handle, the LDS-built one, the voxel table of a filtered map — are occupied): from there b fed a's
    scans is bit-identical to a, step by step, and so is its window."""
    clean_env(monkeypatch)
    P = DIMS[5]
    K, a, b = P + 3 * HB + 2, 0, S - 1
    params = {"filter_local_map": 1} if variant == "filter_local_map" else None
    base = logs_of(synth, DIMS, [60 + s for s in range(S)], K)
    for n in (2, P - 1, P + HB + 1):
        data = [(base[b][:n] + base[a][n:]) if s == b else base[s] for s in range(S)]
        _, g = open_handle(orc, DIMS, S=S, params=params)
        load(g, data, K)
        head = lock_steps(g, DIMS, 0, n, K)
        assert all(step[0][b] != step[0][a] for step in head[1:]), "stream b did not run a log of its own"
        if variant == "filter_local_map" and n > P:
            assert g.local_map(b)[1], "stream b's filtered local map was not active"
        blob = g.export_stream_state(a)
        g.import_stream_state(b, blob)
        assert g.export_stream_state(b) == blob
        tail = lock_steps(g, DIMS, n, K, K)
        for k, step in enumerate(tail):
            assert step[0][b] == step[0][a] and step[1][b] == step[1][a], (S, variant, n, n + k)
        wins = windows(g, S)
        assert wins[b] == wins[a], (S, variant, n)
        g.close()


# ---- 3. migration between shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [3, 16])
def test_migration_between_shapes(orc, synth, monkeypatch, S):
    """Stream j of an S-stream handle moves to a one-stream handle (liodom_process_scan) and back."""
    clean_env(monkeypatch)
    H, W = DIMS[:2]
    P = DIMS[5]
    K, n1, n2, j = P + 3 * HB + 2, P - 1, P + HB + 2, 1
    data = logs_of(synth, DIMS, [30 + s for s in range(S)], K)
    _, g = open_handle(orc, DIMS, S=S)
    load(g, data, K)
    ref = lock_steps(g, DIMS, 0, K, K)
    g.close()
    _, g = open_handle(orc, DIMS, S=S)
    load(g, data, K)
    got = [(s[0][j], s[1][j]) for s in lock_steps(g, DIMS, 0, n1, K)]
    blob = g.export_stream_state(j)
    g.close()
    _, g1 = open_handle(orc, DIMS)
    g1.import_stream_state(0, blob)
    for k in range(n1, n2):
        pose, info = g1.process_scan(data[j][k], H, W)
        got.append((bits(pose), info_key(info)))
    blob = g1.export_stream_state(0)
    g1.close()
    _, g = open_handle(orc, DIMS, S=S)
    load(g, data, K)
    for s in range(S):                 # the other streams come along from scratch: replay them up to n2 on their own is not needed —
        if s != j:                     # they only have to be fed; stream j is what is compared
            g.reset_stream(s)
    g.import_stream_state(j, blob)
    got += [(s[0][j], s[1][j]) for s in lock_steps(g, DIMS, n2, K, K)]
    g.close()
    for k in range(K):
        want_pose, want_info = ref[k][0][j], ref[k][1][j]
        if S == 3:
            assert got[k] == (want_pose, want_info), (k, "3 <-> 1 streams: bit-identical")
        else:
            a, b = np.frombuffer(got[k][0], np.float64), np.frombuffer(want_pose, np.float64)
            assert np.max(np.abs(a - b)) < 1e-9, (k, np.max(np.abs(a - b)))
            assert got[k][1][2] == want_info[2] and got[k][1][4] == want_info[4] == k, (k, "matches / scan_index")


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------
def test_lockstep_run_with_import_and_reset_against_the_oracle(orc, synth, monkeypatch):
    clean_env(monkeypatch)
    H, W = DIMS[:2]
    P, S = DIMS[5], 16
    K, n_imp, k_reset, j = P + 3 * HB + 2, P + 2, P + HB + 3, 5
    tracked = [0, 2, j]
    base = logs_of(synth, DIMS, [50 + s for s in range(S)], K)
    new = logs_of(synth, DIMS, [90], K)[0]
    data = [(base[s][:k_reset] + new[:K - k_reset]) if s == j else base[s] for s in range(S)]
    po, g = open_handle(orc, DIMS, S=S, debug=1)
    m = g.modes()
    assert m["knn8"] == "1" and m["hash_incr"] == "1" and m["hash_build"] == "lds", m
    load(g, data, K)
    ods = {s: orc.Odometer(po) for s in tracked}
    for k in range(K):
        if k == n_imp:
            blobs = [g.export_stream_state(s) for s in range(S)]
            g.close()
            po, g = open_handle(orc, DIMS, S=S, debug=1)
            load(g, data, K)
            for s in range(S):
                g.import_stream_state(s, blobs[s])
        if k == k_reset:
            g.reset_stream(j)
            ods[j] = orc.Odometer(po)
        maps = {s: g.local_map(s)[0] for s in tracked}
        poses, infos = g.process_resident(k, H * W, H, W, readback=True, next_slot=(k + 1 if k + 1 < K else -1))
        assert all(i.status == 0 for i in infos), (k, [i.status for i in infos])
        for s in tracked:
            check_step(orc, po, g, s, infos[s], poses[s], ods[s], maps[s], data[s][k], H, W, "step %d stream %d" % (k, s))
    g.sync()
    assert int(g.modes()["hash_appends"]) > 0
    g.close()


# ---- 5. continuous batching -----------------------------------------------------------------------------------------------------
def test_continuous_batching(orc, synth, monkeypatch):
    clean_env(monkeypatch)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import batch_logs
    finally:
        sys.path.pop(0)
    H, W = DIMS[:2]
    P, S, N = DIMS[5], 16, 24
    lo, hi = 6, P + 3 * HB + 2
    lengths = [lo + (i * (hi - lo)) // (N - 1) for i in range(N)]
    lengths = [lengths[(7 * i) % N] for i in range(N)]           # (not sorted: slots free up in an irregular order)
    assert min(lengths) == lo and max(lengths) == hi
    cfg = synth.make_cfg(H, W, 0)
    logs = [[synth.scan(cfg, 100 + i, k)[0] for k in range(lengths[i])] for i in range(N)]
    _, g = open_handle(orc, DIMS, S=S)
    res = batch_logs.run(g, logs, H, W)
    g.close()
    assert sorted(res["slot_of_log"]) == list(range(N)) and res["status_bits"] == 0, res["status_bits"]
    assert len(set(res["slot_of_log"].values())) > 1 and res["steps"] < sum(lengths)
    # every log alone from scan 0 on a fresh 16-stream handle (16 logs per handle, one per stream; shorter ones repeat their last scan)
    for first in range(0, N, S):
        group = list(range(first, min(first + S, N)))
        Kg = max(lengths[i] for i in group)
        data = [[logs[i][min(k, lengths[i] - 1)] for k in range(Kg)] for i in group]
        data += [data[0]] * (S - len(group))
        _, g = open_handle(orc, DIMS, S=S)
        load(g, data, Kg)
        steps = lock_steps(g, DIMS, 0, Kg, Kg)
        g.close()
        for slot, i in enumerate(group):
            assert len(res["poses"][i]) == lengths[i]
            for k in range(lengths[i]):
                assert bits(res["poses"][i][k]) == steps[k][0][slot], ("log", i, "scan", k)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_untouched(orc, synth, monkeypatch):
    clean_env(monkeypatch)
    H, W = DIMS[:2]
    scans = logs_of(synth, DIMS, [3], 8)[0]
    _, g = open_handle(orc, DIMS)
    ref = [bits(g.process_scan(x, H, W)[0]) for x in scans]
    g.close()
    _, other = open_handle(orc, (16, 900, 0, 6, 10, 7))          # another local_map_size
    other.process_scan(scans[0], H, W)
    foreign = other.export_stream_state(0)
    other.close()
    _, g = open_handle(orc, DIMS)
    L = g.L
    for k in range(4):
        assert bits(g.process_scan(scans[k], H, W)[0]) == ref[k]
    blob = g.export_stream_state(0)
    n = C.c_int64()
    buf = (C.c_ubyte * len(blob))()
    assert L.liodom_export_stream_state(g.h, 0, buf, len(blob) - 16, C.byref(n)) == api.ERR_CAPACITY and n.value == len(blob)
    assert L.liodom_export_stream_state(g.h, 0, buf, len(blob), C.byref(n)) == 0 and bytes(buf) == blob
    assert g.stream_state_size() >= len(blob)
    flipped = bytes([blob[0] ^ 1]) + blob[1:]
    for bad in (flipped, blob[:-16], blob[:100], foreign):
        assert L.liodom_import_stream_state(g.h, 0, bad, len(bad)) == api.ERR_INVALID_ARG, len(bad)
    for fn in (L.liodom_reset_stream,):
        assert fn(g.h, 1) == api.ERR_INVALID_ARG and fn(g.h, -1) == api.ERR_INVALID_ARG
    assert L.liodom_export_stream_state(g.h, 1, buf, len(blob), C.byref(n)) == api.ERR_INVALID_ARG
    assert L.liodom_import_stream_state(g.h, 2, blob, len(blob)) == api.ERR_INVALID_ARG
    assert g.export_stream_state(0) == blob                       # nothing of it reached the stream
    # an outstanding edge ticket
    t = g.extract_edges_device(scans[4], H, W)
    assert t is not None
    assert L.liodom_reset_stream(g.h, 0) == api.ERR_BUSY
    assert L.liodom_export_stream_state(g.h, 0, buf, len(blob), C.byref(n)) == api.ERR_BUSY
    assert L.liodom_import_stream_state(g.h, 0, blob, len(blob)) == api.ERR_BUSY
    pose, _ = g.odometry_step_device(t)
    assert bits(pose) == ref[4], "the stream's next pose changed by the refused calls"
    for k in range(5, 8):
        assert bits(g.process_scan(scans[k], H, W)[0]) == ref[k]
    g.close()


def test_reset_stream_on_a_one_stream_handle_equals_reset(orc, synth, monkeypatch):
    clean_env(monkeypatch)
    H, W, lt, R, epr, P = VLP16
    K = P + 6
    a, b = logs_of(synth, VLP16, [11, 12], K)
    _, g = open_handle(orc, VLP16, pose_log_capacity=K + 8)
    load(g, [b], K)
    poses, infos = g.replay_resident(0, K, H * W, H, W, depth=1)
    ref = [(bits(poses[k][0]), info_key(infos[k])) for k in range(K)]
    g.close()
    _, g = open_handle(orc, VLP16, pose_log_capacity=K + 8)
    load(g, [a], K)
    g.replay_resident(0, K - 3, H * W, H, W, depth=1)            # warm: chain mode, speculative hand-overs
    g.reset_stream(0)
    load(g, [b], K)
    poses, infos = g.replay_resident(0, K, H * W, H, W, depth=1)
    assert [(bits(poses[k][0]), info_key(infos[k])) for k in range(K)] == ref
    assert g.modes()["chain"] == "1"
    g.close()


# ---- replay harness -------------------------------------------------------------------------------------------------------------
def test_replay_harness_resumes_from_a_saved_state(synth, tmp_path):
    """liodom_replay over K scans, and again as save_state after scan K / 2 followed by load_state: the result files of the two
    parts, one behind the other, are byte-equal to the uninterrupted run's (odom.txt carries 17 digits and the twist, i.e. the
    host side's previous pose and stamp as well)."""
    import subprocess
    exe = os.path.join(ROOT, "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (__graft_entry__.build())"
    H, W, K = 16, 900, 14
    m = K // 2
    cfg = synth.make_cfg(H, W, 0)
    scan_dir = tmp_path / "scans"
    scan_dir.mkdir()
    for k in range(K):
        synth.scan(cfg, 0, k)[0].astype(np.float32).tofile(str(scan_dir / ("%06d.bin" % k)))
    common = ["scan_lines=16", "scan_regions=6", "edges_per_region=10", "prev_frames=5"]
    state = str(tmp_path / "state.bin")
    runs = {"whole": [], "head": ["save_state=" + state, "save_at=%d" % m, "last=%d" % m], "tail": ["load_state=" + state, "first=%d" % (m + 1)]}
    for name, extra in runs.items():
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([exe, str(scan_dir), str(out) + "/"] + common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-1500:])
    # option combinations that would do something else than asked are refused before anything runs
    for bad in (["save_state=" + state], ["save_at=3"], ["first=3"], ["load_state=" + state], ["save_state=" + state, "save_at=99"],
                ["save_state=" + state, "save_at=3", "threads=true"], ["load_state=" + state, "first=3", "threads=true"],
                ["save_state=" + state, "save_at=9", "last=5"]):
        r = subprocess.run([exe, str(scan_dir), str(tmp_path / "whole") + "/x_"] + common + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "liodom_replay:" in r.stderr, (bad, r.returncode, r.stderr[-300:])
    st = api.parse_stream_state(open(state, "rb").read()[:-128])      # (the host's trailer: LaserOdometer::saveState)
    assert st["scan_counter"] == m + 1 and st["n_frames"] == 5
    for f in ("poses.txt", "odom.txt"):
        whole = (tmp_path / "whole" / f).read_bytes()
        parts = (tmp_path / "head" / f).read_bytes() + (tmp_path / "tail" / f).read_bytes()
        assert len(whole.splitlines()) == K and parts == whole, f
