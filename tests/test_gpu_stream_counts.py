"""Lock-step batches at bench.py's batched size (256 streams) and handles at every stream count where liodom_create switches
code paths, every stream on data of its own.

Batch tests that replay a few data streams round-robin cannot see a kernel that reads or writes another stream's buffers when that
stream holds equal data.  Here every stream sees a different scan at every step, so a per-stream offset or indexing mistake — in
the 57 x 256 tiles of k_ring_split_lb and their shared ticket counter, k_ring_split_fix's per-stream flags, the per-stream tables
and logs — changes that stream's result:
  A. bench.py's batched leg (hdl64: 64 x 1800, P = 20, 256 streams, next step's extraction overlapped) against the oracle on six
     streams, against sixteen 16-stream handles that replay the same 256 sequences in other positions (bit-identical per
     stream), and with a ring pitch every regular ring outgrows (k_ring_split_fix redoes those streams);
  B. at 16 x 900, S = 4 (streamed rebuild, four-workgroup solve), 5 and 15 (three-kernel global rebuild, k_knn<256>), 16
     (lock-step: k_knn8 + k_line_gate, LDS cell hash, incremental hash), and on both sides of the largest launch that
     k_ring_split may hold resident (ring_split_max_wgs): every stream against the oracle.
Run with -m gpu on an MI355X."""
import functools

import numpy as np
import pytest

import liodom_amd as la
from test_gpu_lockstep_shapes import (HB_PERIOD, LDS_CELLS_MAX, TILE_PTS, assert_records_equal, lockstep_replay,
                                      predicted_hash_counters)

pytestmark = pytest.mark.gpu

HDL64 = (64, 1800, 0, 8, 10, 20)      # bench.py WORKLOADS["hdl64"]: H, W, lidar_type, R, epr, P
SMALL = (16, 900, 0, 6, 10, 5)        # the cheap oracle shape of test_sixteen_lockstep_streams_match_single_stream


def bench_batch_data(synth, S, K, bases=8):
    """Handle stream s replays base sequence s % bases from its scan s // bases on: no two streams see the same scan at one step.
    The last base is ragged (synth.ragged: NaN no-returns, rings of unequal length, dead rings)."""
    H, W, lt = HDL64[:3]
    cfg = synth.make_cfg(H, W, lt)
    n = K + (S - 1) // bases
    base = [[synth.scan(cfg, 1000 + b, k)[0] for k in range(n)] for b in range(bases)]
    base[-1] = [synth.ragged(x, H, W, lt, seed=100 + k) for k, x in enumerate(base[-1])]
    return base, [base[s % bases][s // bases:s // bases + K] for s in range(S)]


def test_bench_batched_leg_256_streams(orc, synth, monkeypatch):
    """bench.py's batched leg (256 lock-step streams at the headline shape, process_resident with the next step's extraction
    overlapped) for K = 32 steps: the window fills on step 19, the rebuilds of steps 20, 24 and 28 follow evictions.  Every
    stream and step: status 0, pose log equal to the readback.  Streams 0, 15, 16, 128, 200, 255 (15 and 255 ragged) against
    the oracle.  Then the same 256 sequences on sixteen 16-stream handles, handle j position i replaying stream
    16 j + (i + j + 1) % 16: every stream's record (pose bits, n_edges, map_points, match counts, LM iterations and
    terminations, digests of edges and correspondences) bit-identical — a stream's result must not depend on which streams
    share its launch.  Then six steps with a ring pitch of 1500 (LIODOM_RING_PITCH): k_ring_split_fix redoes every stream
    whose ring outgrew it, bit-identical to the default run."""
    H, W, lt, R, epr, P = HDL64
    S, K = 256, 32
    checked = [0, 15, 16, 128, 200, 255]
    base, data = bench_batch_data(synth, S, K)
    want = {"n_streams": str(S), "knn8": "1", "hash_incr": "1", "hash_build": "lds", "lm_groups": "1", "line_gate_kernel": "1"}
    big = lockstep_replay(orc, HDL64, data, {}, want, "k_ring_split_lb", monkeypatch, oracle=checked, track=[0], next_slot=True)
    print("256-stream handle modes:", " ".join("%s=%s" % kv for kv in big.modes.items()))
    assert big.worst[0] < 1e-6 and big.worst[1] < 1e-6, big.worst
    assert K > P + 2 * HB_PERIOD and big.n_edges.min() > 0
    assert (int(big.modes["hash_rebuilds"]), int(big.modes["hash_appends"])) == \
        predicted_hash_counters(big.cells[:, 0], LDS_CELLS_MAX), (big.modes, big.cells[::HB_PERIOD, 0])

    # stream independence: the same sequences in other launches and positions
    want16 = dict(want, n_streams="16")
    for j in range(S // 16):
        src = [16 * j + (i + j + 1) % 16 for i in range(16)]
        small = lockstep_replay(orc, HDL64, [data[s] for s in src], {}, want16, "k_ring_split_lb", monkeypatch, next_slot=True)
        for k in range(K):
            for i, s in enumerate(src):
                assert_records_equal(small.records[k][i], big.records[k][s],
                                     ("16-stream handle", j, "position", i, "256-stream handle stream", s, "step", k))

    # k_ring_split_fix at 256 streams: with a pitch of 1500 every ring of 1500+ points is cut and its stream redone
    K6, pitch = 6, 1500
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P)

    @functools.lru_cache(maxsize=None)
    def outgrows(b, k):
        offs, _ = orc.split(po, base[b][k], H, W)
        return int(np.diff(offs).max()) > pitch

    over = [any(outgrows(s % 8, s // 8 + k) for k in range(K6)) for s in range(S)]
    assert sum(over) > S // 2, sum(over)
    fix = lockstep_replay(orc, HDL64, [d[:K6] for d in data], {"LIODOM_RING_PITCH": str(pitch)}, want, "k_ring_split_lb",
                          monkeypatch, next_slot=True)
    for k in range(K6):
        for s in range(S):
            assert_records_equal(fix.records[k][s], big.records[k][s], ("LIODOM_RING_PITCH", pitch, "step", k, "stream", s))


@functools.lru_cache(maxsize=None)
def ring_split_max_wgs():
    """The launch size (workgroups) up to which k_ring_split runs: a property of the device and of H, not of the stream count."""
    H, W, lt, R, epr, P = SMALL
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(n_streams=1, max_points=H * W, max_width=W))
    m = g.modes()
    g.close()
    assert m["ring_split"] == "1", m
    return int(m["ring_split_max_wgs"])


def stream_count(label):
    fit = ring_split_max_wgs() // -(-SMALL[0] * SMALL[1] // TILE_PTS)      # streams of 8 tiles the all-resident split holds
    return {"fit": fit, "fit+1": fit + 1}.get(label) or int(label)


@pytest.mark.parametrize("label", ["4", "5", "15", "16", "fit", "fit+1"])
def test_stream_count_switches_against_the_oracle(orc, synth, monkeypatch, label):
    """The paths liodom_create picks by stream count, at 16 x 900 (R = 6, epr = 10, P = 5, K = 12, next step's extraction
    overlapped), every stream on its own synthetic stream 100 + s (ragged where s % 4 == 3) and every stream against the oracle:
      S <= 4: streamed rebuild, solves of four workgroups (lm_groups from the edge capacity, 1056 here);
      S 5-15: three-kernel global rebuild, one-workgroup solves, k_knn<256>;
      S >= 16: lock-step — k_knn8 + k_line_gate, the LDS cell hash, rebuilt every kHbPeriod-th step and appended in between;
      fit = ring_split_max_wgs // 8 (a scan is 8 tiles): the largest launch of the all-resident k_ring_split; fit + 1 takes
      k_ring_split_lb (lock-step handles) or k_classify + k_ring_scatter."""
    H, W, lt, R, epr, P = SMALL
    K = 12
    S = stream_count(label)
    fit = stream_count("fit")
    print("ring_split_max_wgs %d: S_fit = %d" % (ring_split_max_wgs(), fit))
    cfg = synth.make_cfg(H, W, lt)
    data = [[synth.scan(cfg, 100 + s, k)[0] for k in range(K)] for s in range(S)]
    for s in range(3, S, 4):
        data[s] = [synth.ragged(x, H, W, lt, seed=100 * s + k) for k, x in enumerate(data[s])]
    lockstep = S >= 16
    want = {"n_streams": str(S),
            "early_rebuild": "1" if S <= 4 else "0",
            "hash_build": "streamed" if S <= 4 else ("lds" if lockstep else "global"),
            "lm_groups": "4" if S <= 4 else "1",
            "knn_instance": "128" if lockstep else "256",
            "knn8": "1" if lockstep else "0",
            "line_gate_kernel": "1" if lockstep else "0",
            "hash_incr": "1" if lockstep else "0"}
    split = "k_ring_split" if S <= fit else ("k_ring_split_lb" if lockstep else "k_classify + k_ring_scatter")
    r = lockstep_replay(orc, SMALL, data, {}, want, split, monkeypatch, oracle=range(S), track=[0], next_slot=True)
    assert r.worst[0] < 1e-6 and r.worst[1] < 1e-6, r.worst
    if lockstep:
        assert (int(r.modes["hash_rebuilds"]), int(r.modes["hash_appends"])) == \
            predicted_hash_counters(r.cells[:, 0], LDS_CELLS_MAX), (r.modes, r.cells[::HB_PERIOD, 0])
