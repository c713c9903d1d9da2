"""The ring split of unorganised clouds (lidar_type 0) on the designed clouds of tests/designed_splits.py: classify_point — the
float fast path next to every bin edge and range limit, the FP64 path on them, non-finite, overflowing, underflowing and
origin points — and the four partitions (k_ring_split; k_classify + k_ring_scatter; k_ring_split_lb with k_ring_split_fix)
on skewed tiles, at the batch tails of their histogram and look-back loops and at the pitch edge.

Bar (the project's): ring offsets, FP64 smoothness bits (ring-major, so every position counts) and the edges of every stream
EXACTLY equal to the oracle's, through check() of tests/test_gpu_designed_extract.py.  The oracle is the single reference; the
GPU legs are not compared with each other.  That every world reaches what it was built for, that the oracle equals a float64
restatement on it and that the observable notices a swapped pair is asserted in tests/test_designed_splits.py.  Which kernel
a handle runs is asserted from liodom_get_modes.  scan_regions 4, edges_per_region 0: min_points_per_scan is 10, so a ring of
its ten guard points is already extracted.

What this observable cannot see: whether k_ring_split_fix ran.  It redoes a stream's split into the compact layout and the
answer is the oracle's either way, so an overflow flag raised for a ring of exactly `pitch` points, or one left standing for
the next launch, costs time and changes no result.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import liodom_amd as la
import designed_splits as ds
from test_gpu_designed_extract import _Env, check, want

pytestmark = pytest.mark.gpu

HS = [16, 32, 64]
R, EPR, MAX_WIDTH = ds.R_SPLIT, ds.EPR_SPLIT, 980
P_TEST = 264
ONE_STREAM = {"1": "k_ring_split", "0": "k_classify + k_ring_scatter"}


def open_handle(orc, H, lo, hi, max_points, S=1, env=None):
    kw = dict(lidar_type=0, scan_lines=H, scan_regions=R, edges_per_region=EPR, min_range=float(lo), max_range=float(hi))
    with _Env(env or {}):
        g = la.Liodom(la.make_params(**kw), la.make_config(n_streams=S, max_points=max(int(max_points), 16), max_width=MAX_WIDTH, debug_buffers=1))
    return g, orc.make_params(**kw)


def padded(x, n):
    """The cloud with NaN points behind it, n points in all (the streams of one launch share the point count)."""
    out = np.full((n, 4), np.nan, np.float32)
    out[:len(x)] = x
    out[len(x):, 3] = 0
    return out


def answer(orc, po, name, x, H):
    return want(orc, po, ("split", name, po.min_range, po.max_range, len(x)), x, H, 0)


def assert_one_stream_path(g, split, n):
    m = g.modes()
    assert m["ring_split"] == split and m["n_streams"] == "1", m
    if split == "1":
        assert int(m["ring_split_max_wgs"]) >= -(-n // ds.TILE), m        # (the scan's tiles fit k_ring_split's launch)


def by_limits(worlds):
    groups = {}
    for w in worlds:
        groups.setdefault((w.min_range, w.max_range), []).append(w)
    return groups


# ---------------------------------------------------------------------------------------------
# one stream
# ---------------------------------------------------------------------------------------------
def world_group(H, group):
    """designed_splits.worlds is the six clouds of decisions (bin edges, three pairs of range limits, odd values with min_range 0
    and 3), then the skewed ones."""
    ws = ds.worlds(H)
    assert [w.name.split("_")[0] for w in ws[:7]] == ["bin", "range", "range", "range", "odd", "odd", "skew"]
    return {"decisions": ws[:6], "skew": ws[6:], "tiles": ds.batch_tails(H)}[group]


@pytest.mark.parametrize("group", ["decisions", "skew", "tiles"])
@pytest.mark.parametrize("size", ["exact", "larger"])
@pytest.mark.parametrize("split", list(ONE_STREAM))
@pytest.mark.parametrize("H", HS)
def test_one_stream_worlds(orc, H, split, size, group):
    """Every world of designed_splits.worlds (`decisions`: bin edges, range limits at three limit pairs, odd values with min_range 0
    and 3, the origin point among them; `skew`: every pattern and cloud length) and the batch tails of 8 | 9 | 17 and 64 | 65 tiles
    (`tiles`), on handles whose max_points is the cloud's n (one per pair of range limits and n) and on one that is larger (one per
    pair of range limits, serving all its clouds)."""
    env = {"LIODOM_RING_SPLIT": split}
    for (lo, hi), ws in by_limits(world_group(H, group)).items():
        larger = max(len(w.x) for w in ws) + 1000
        g, cap = None, None
        for w in sorted(ws, key=lambda w: len(w.x)):
            want_cap = len(w.x) if size == "exact" else larger
            if cap != want_cap:
                if g is not None:
                    g.close()
                g, po = open_handle(orc, H, lo, hi, want_cap, env=env)
                cap = want_cap
                assert_one_stream_path(g, split, cap)
            check(g, answer(orc, po, w.name, w.x, H), g.extract_edges(w.x, H, 0), H, (w.name, H, split, size))
        g.close()


@pytest.mark.parametrize("split", list(ONE_STREAM))
def test_a_short_scan_between_two_long_ones(orc, split):
    """One handle, three extractions: 66 tiles, one tile, 66 tiles again — nothing of the longer scan (id bytes, histogram rows,
    arrival counters) may survive into the shorter one, nor the other way round."""
    H = 64
    long_, short = ds.tiles(H, ds.lookback_tiles(H)), ds.skew(H, "round_robin", 2047)
    g, po = open_handle(orc, H, 3.0, 75.0, len(long_.x), env={"LIODOM_RING_SPLIT": split})
    assert_one_stream_path(g, split, len(long_.x))
    for k, w in enumerate((long_, short, long_)):
        check(g, answer(orc, po, w.name, w.x, H), g.extract_edges(w.x, H, 0), H, (w.name, split, k))
    g.close()


# ---------------------------------------------------------------------------------------------
# several streams in one launch
# ---------------------------------------------------------------------------------------------
def run_launches(orc, g, po, H, n, deals, clouds, what):
    """Uploads deals[k][s] (indices into clouds = [(name, padded cloud)]) into slot k, runs the launches in order and checks every
    stream of each against the oracle."""
    S = len(deals[0])
    g.alloc_resident(len(deals))
    for k, deal in enumerate(deals):
        for s in range(S):
            g.upload_scan(s, k, clouds[deal[s]][1])
    for k, deal in enumerate(deals):
        g.process_resident(k, n, H, 0, readback=True)
        for s in range(S):
            name, x = clouds[deal[s]]
            check(g, answer(orc, po, name, x, H), g.get_edges(s), H, what + (k, s, name), stream=s)


@pytest.mark.parametrize("lo", [3.0, 0.0])
@pytest.mark.parametrize("H", HS)
def test_three_streams_two_kernels(orc, H, lo):
    """liodom_process_resident on three streams with LIODOM_RING_SPLIT=0: the multi-row grid of k_classify / k_ring_scatter.  The
    streams carry bin_edges, skew(one_ring_tile) and odd_values (min_range 3, and 0 with the origin points) in one launch; the
    second launch deals them differently."""
    ws = [ds.bin_edges(H), ds.skew(H, "one_ring_tile"), ds.odd_values(H, lo)]
    n = max(len(w.x) for w in ws)
    clouds = [(w.name, padded(w.x, n)) for w in ws]
    g, po = open_handle(orc, H, lo, 75.0, n, S=3, env={"LIODOM_RING_SPLIT": "0"})
    m = g.modes()
    assert m["ring_split"] == "0" and m["ring_split_lb"] == "0" and m["n_streams"] == "3", m
    run_launches(orc, g, po, H, n, [[0, 1, 2], [2, 0, 1]], clouds, (H, lo, "three"))
    g.close()


def open_lockstep(orc, H, lo, n, env=None):
    """Sixteen lock-step streams on k_ring_split_lb + k_ring_split_fix (LIODOM_RING_SPLIT=0: small launches would otherwise fit
    k_ring_split).  (k_hash_build publishes 8192 slots per stream whatever the window: the table must hold them.)"""
    g, po = open_handle(orc, H, lo, 75.0, n, S=16, env=dict({"LIODOM_RING_SPLIT": "0"}, **(env or {})))
    m = g.modes()
    assert m["ring_split_lb"] == "1" and m["ring_split"] == "0" and m["n_streams"] == "16" and int(m["table_size"]) >= 8192, m
    return g, po


@pytest.mark.parametrize("lo", [3.0, 0.0])
@pytest.mark.parametrize("H", HS)
def test_lockstep_worlds(orc, H, lo):
    """Worlds 1 - 4 dealt over sixteen lock-step streams, two launches with different deals: bin edges, range limits and odd values
    (the handle's min_range: 3, and 0 with the origin points) through classify_point as k_ring_split_lb compiles it; the skew
    patterns through its ranks and look-back — skew(one_ring_tile) outgrows 9/8 of the nominal ring length by itself and reaches
    k_ring_split_fix at the default pitch.  Then one stream alone through the same handle."""
    ws = [ds.bin_edges(H), ds.range_limits(H, 3.0, 75.0), ds.odd_values(H, lo)] + [ds.skew(H, p) for p in ds.PATTERNS]
    ws += [ds.skew(H, "blocks", 2049), ds.skew(H, "round_robin", 513), ds.skew(H, "empty_rings", 2048), ds.skew(H, "round_robin", 1),
           ds.tiles(H, 9), ds.skew(H, "round_robin", 2047), ds.skew(H, "empty_rings", 513), ds.skew(H, "blocks", 511)]
    n = max(len(w.x) for w in ws)
    clouds = [(w.name, padded(w.x, n)) for w in ws]
    assert len(clouds) == 17
    g, po = open_lockstep(orc, H, lo, n)
    nominal_pitch = -(-n * 9 // (H * 8))
    assert np.diff(answer(orc, po, clouds[3][0], clouds[3][1], H)["offs"]).max() > nominal_pitch + 8        # one_ring_tile: k_ring_split_fix
    deals = [[(s + 7 * k) % 17 for s in range(16)] for k in range(2)]
    run_launches(orc, g, po, H, n, deals, clouds, (H, lo, "lockstep"))
    name, x = clouds[0]
    check(g, answer(orc, po, name, x, H), g.extract_edges(x, H, 0, stream=15), H, (H, lo, "alone"), stream=15)
    g.close()


@pytest.mark.parametrize("lo", [3.0, 0.0])
@pytest.mark.parametrize("H", HS)
def test_subset_step(orc, H, lo):
    """liodom_process_resident_subset over streams 1, 2, 7, 15 of sixteen: the kList instances of k_ring_split_lb and
    k_ring_split_fix, into which classify_point is compiled on its own.  A full launch first gives every stream a plain skewed
    cloud, so that nothing but the subset step classifies a designed decision: its four streams then carry the odd values (the
    origin points with min_range 0), the bin edges, skew(one_ring_tile) — k_ring_split_fix<true> — and the range limits.  The
    streams that sit out keep the first launch's answer."""
    plain_ws = [ds.skew(H, "round_robin"), ds.skew(H, "blocks"), ds.skew(H, "late_ring"), ds.skew(H, "dead_tile")]
    ws = [ds.odd_values(H, lo), ds.bin_edges(H), ds.skew(H, "one_ring_tile"), ds.range_limits(H, 3.0, 75.0)]
    n = max(len(w.x) for w in ws + plain_ws)
    first = [(w.name, padded(w.x, n)) for w in plain_ws]
    g, po = open_lockstep(orc, H, lo, n)
    deal = [s % 4 for s in range(16)]
    run_launches(orc, g, po, H, n, [deal], first, (H, lo, "first"))
    subset = [1, 2, 7, 15]
    for s, w in zip(subset, ws):
        g.upload_scan(s, 0, padded(w.x, n))
    g.process_resident_subset(0, subset, n, H, 0, readback=True)
    for s, w in zip(subset, ws):
        check(g, answer(orc, po, w.name, padded(w.x, n), H), g.get_edges(s), H, (H, lo, "subset", s, w.name), stream=s)
    for s in (0, 3, 8, 14):
        name, x = first[deal[s]]
        check(g, answer(orc, po, name, x, H), g.get_edges(s), H, (H, lo, "sat out", s, name), stream=s)
    g.close()


@pytest.mark.parametrize("H", HS)
def test_lockstep_pitch_edge(orc, H):
    """LIODOM_RING_PITCH=P.  Launch 0: streams 3 and 12 carry a ring of P + 1 points (k_ring_split_fix redoes them), stream 5 one
    of exactly P points (it fits: pre + mine == pitch), the others rings of at most P - 1.  Launch 1 on the same handle: no
    stream over, streams 3 and 12 now at exactly P — the overflow flag and the launch tag of launch 0 are gone.  Launch 2: the
    overflow moves to streams 0 and 15.  Every stream of every launch equals the oracle."""
    P = P_TEST
    kinds = {0: {3: "over", 12: "over", 5: "full"}, 1: {3: "full", 12: "full", 5: "over"}, 2: {0: "over", 15: "over", 3: "under"}}
    del kinds[1][5]                                           # (launch 1: nothing over)
    ws, deals = [], []
    for k in range(3):
        deal = []
        for s in range(16):
            ws.append(ds.pitch(H, P, kinds[k].get(s, "under"), seed=s + 16 * k))
            deal.append(len(ws) - 1)
        deals.append(deal)
    n = max(len(w.x) for w in ws)
    assert H * P >= n
    clouds = [("%s_k%d" % (w.name, i // 16), padded(w.x, n)) for i, w in enumerate(ws)]
    g, po = open_lockstep(orc, H, 3.0, n, env={"LIODOM_RING_PITCH": str(P)})
    for k in range(3):
        top = [np.diff(answer(orc, po, clouds[i][0], clouds[i][1], H)["offs"]).max() for i in deals[k]]
        assert [s for s in range(16) if top[s] > P] == sorted(s for s, v in kinds[k].items() if v == "over")
        assert [s for s in range(16) if top[s] == P] == sorted(s for s, v in kinds[k].items() if v == "full")
    run_launches(orc, g, po, H, n, deals, clouds, (H, "pitch"))
    g.close()


def test_lockstep_second_look_back_batch(orc):
    """66 tiles at H = 64 on all sixteen streams: thread (w, r) of k_ring_split_lb sums eight predecessors per batch, 8 * (512 / 64)
    tiles in all, so tiles 65 and 66 run a second batch.  One cloud and one oracle answer for all streams."""
    H = 64
    w = ds.tiles(H, ds.lookback_tiles(H))
    n = len(w.x)
    assert -(-n // ds.TILE) == 8 * (512 // H) + 2
    g, po = open_lockstep(orc, H, 3.0, n)
    o = answer(orc, po, w.name, w.x, H)
    g.alloc_resident(1)
    for s in range(16):
        g.upload_scan(s, 0, w.x)
    g.process_resident(0, n, H, 0, readback=True)
    for s in range(16):
        check(g, o, g.get_edges(s), H, (w.name, s), stream=s)
    g.close()
