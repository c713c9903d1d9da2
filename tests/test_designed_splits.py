"""The designed clouds of tests/designed_splits.py on the CPU: the float64 restatement of the ring split equals the oracle on
every world (offsets, the source indices implied by the order, and the smoothness bits), every world reaches what it was
built for (asserted on the restatement, not assumed), and the observable of tests/test_gpu_designed_split.py — ring offsets
and ring-major smoothness — is sensitive: swapping two adjacent points of a ring changes the smoothness bits at both places,
and so does moving a point next to a bin edge into the neighbouring ring."""
import numpy as np
import pytest

import designed_splits as ds

HS = [16, 32, 64]
P_TEST = 264


def all_worlds(H):
    ws = ds.worlds(H) + ds.batch_tails(H) + [ds.pitch(H, P_TEST, kind, seed) for kind in ("over", "full", "under") for seed in (0, 1)]
    if H == 64:
        ws.append(ds.tiles(H, ds.lookback_tiles(H)))
    return ws


def params(orc, w):
    return orc.make_params(min_range=w.min_range, max_range=w.max_range, lidar_type=0, scan_lines=w.H,
                           scan_regions=ds.R_SPLIT, edges_per_region=ds.EPR_SPLIT)


def bits(c):
    return np.where(np.isnan(c), np.uint64(0xFFFFFFFFFFFFFFFF), np.ascontiguousarray(c).view(np.uint64))


@pytest.mark.parametrize("H", HS)
def test_restatement_equals_the_oracle(orc, H):
    names = set()
    for w in all_worlds(H):
        po = params(orc, w)
        assert po.min_points_per_scan == 10
        offs, order = orc.split(po, w.x, H, 0)
        r_offs, r_order = ds.split_ref(w.x, H, w.min_range, w.max_range)
        assert np.array_equal(offs, r_offs), w.name
        assert np.array_equal(order, r_order), w.name
        c = ds.smoothness_ref(w.x, r_offs, r_order)
        assert np.array_equal(bits(orc.extract(po, w.x, H, 0, want_curv=True)["curv"][:len(c)]), bits(c)), w.name
        names.add((w.name, w.min_range, w.max_range))
    assert len(names) == len(all_worlds(H))


# ---------------------------------------------------------------------------------------------
# every world reaches what it was built for
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
def test_bin_edges_straddle_every_decision(H):
    lo, hi, vlo, vhi = ds.edges_of(H)
    assert len(lo) == H + 1 and (vlo != vhi).all() and (np.nextafter(lo, np.inf) == hi).all()
    assert vlo[0] == -1 or vhi[0] == -1                      # the edges into and out of "dropped" count
    assert vlo[-1] == -1 or vhi[-1] == -1
    if H == 64:
        assert hi[0] == -24.33 and vlo[0] == -1 and vhi[0] == 63 and lo[-1] == 2.0 and vlo[-1] == 0 and vhi[-1] == -1
    assert sorted(set(vlo) | set(vhi)) == list(range(-1, H))
    w = ds.bin_edges(H)
    assert w.designed.sum() == 285 * (H + 1) and len(w.x) == 285 * (H + 1) + 10 * H
    ring, a, d = ds.classify(w.x, H, w.min_range, w.max_range)
    ring, a, d = ring[w.designed], a[w.designed], d[w.designed]
    e = w.info["edge_of"]
    off = np.abs(a - hi[e])
    assert (d > 3.3).all() and (d < 72).all()                # the range decides nothing here
    for k in range(H + 1):
        near = (e == k) & (off < 1e-5)
        assert set(ring[near]) == {vlo[k], vhi[k]}, (H, k)   # both verdicts next to every edge
        m = e == k                                           # and either side of the 2e-4 degree margin of the fast path
        assert ((off[m] > 1.5e-4 - 1e-5) & (off[m] < 2e-4)).any() and ((off[m] > 2e-4) & (off[m] < 3e-4 + 1e-5)).any()
    assert (off < 1e-6).sum() >= 400, (H, (off < 1e-6).sum())


@pytest.mark.parametrize("pair", ds.LIMIT_PAIRS)
@pytest.mark.parametrize("H", HS)
def test_range_limits_straddle_both_limits(H, pair):
    w = ds.range_limits(H, *pair)
    ring, a, d = ds.classify(w.x, H, *pair)
    assert (ring[~w.designed] >= 0).all()
    ring, d = ring[w.designed], d[w.designed]
    for which, L in enumerate(pair):
        m = w.info["limit"] == which
        two = m & (np.abs(d - L) <= 2 * float(np.spacing(np.float32(L))))
        assert (ring[two] >= 0).any() and (ring[two] < 0).any(), (H, L)          # both verdicts within 2 ulps of the limit
        exact = m & (d == L)
        if float(np.float32(L)) == L:
            assert exact.sum() >= 4 and (ring[exact] >= 0).all(), (H, L)         # the limits are inclusive
        else:
            assert not exact.any()
        rel = np.abs(d[m & (w.info["steps"] == 99)] / L - 1.0)
        assert ((rel > 0.4e-4) & (rel < 1e-4)).sum() >= 4 and ((rel > 1e-4) & (rel < 2.1e-4)).sum() >= 4
    # without its range margin the float fast path would decide some of them wrongly: per limit, a point whose float range
    # (float products, sum and square root, as classify_point forms it) lies on the other side of the float limit than the double one
    x = w.x[w.designed]
    df = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    assert df.dtype == np.float32
    below = (df < np.float32(pair[0])) != (d < pair[0])
    above = (df > np.float32(pair[1])) != (d > pair[1])
    assert below[w.info["limit"] == 0].sum() >= 2 and above[w.info["limit"] == 1].sum() >= 2, (H, pair, below.sum(), above.sum())
    # a dropped point's verdict is the range's alone: every designed point sits mid-bin
    assert np.array_equal(ring >= 0, (d >= pair[0]) & (d <= pair[1]))


@pytest.mark.parametrize("H", HS)
def test_odd_values_and_the_origin(orc, H):
    odd = ds.odd_points()
    for lo in (0.0, 3.0):
        w = ds.odd_values(H, lo)
        ring = ds.classify(w.x, H, lo, 75.0)[0]
        assert (ring[~w.designed] >= 0).all()
        ring, x = ring[w.designed], w.x[w.designed]
        which = w.info["odd"]
        assert len(which) == len(ring) == 3 * len(odd)
        with np.errstate(invalid="ignore"):
            bad = ~np.isfinite(x[:, :3]).all(axis=1)
        assert bad.sum() == 27 and (ring[bad] == -1).all()
        w_only = ~np.isfinite(x[:, 3]) & ~bad
        assert w_only.sum() == 9 and (ring[w_only] >= 0).all()          # a non-finite intensity is no reason to drop
        origin = (x[:, 0] == 0) & (x[:, 1] == 0)
        assert origin.sum() >= 3 * 18 and (ring[origin] == -1).all()    # z = 0: a NaN angle; z != 0: +-90 degrees
        tiny = (np.abs(x[:, 0]) < 1e-20) & (x[:, 0] != 0) & (x[:, 1] == 0) & (x[:, 2] == 0)
        assert tiny.sum() >= 9 and ((ring[tiny] >= 0) == (lo == 0.0)).all()
        huge = np.abs(x[:, :2]).max(axis=1) >= 1e19
        assert huge.sum() >= 3 * 15 and (ring[huge] == -1).all()
    # the origin cloud of the issue: only (1e-30, 0, 0) and (5, 0, 0) stay
    x = np.zeros((6, 4), np.float32)
    x[:, :3] = [(0, 0, 0), (0, 0, 1), (-0.0, 0, -0.0), (1e-30, 0, 0), (5, 0, 0), (0, 0, -1)]
    po = orc.make_params(min_range=0.0, lidar_type=0, scan_lines=H, scan_regions=ds.R_SPLIT, edges_per_region=ds.EPR_SPLIT)
    offs, order = orc.split(po, x, H, 0)
    assert sorted(order) == [3, 4] and np.array_equal(ds.split_ref(x, H, 0.0, 75.0)[1], order)
    assert ds.ring_from_angle(np.nan, H) == -1


@pytest.mark.parametrize("H", HS)
def test_skewed_clouds_are_what_they_say(H):
    T = ds.TILE
    got = {}
    for p in ds.PATTERNS:
        w = ds.skew(H, p)
        ring = ds.classify(w.x, H, 3.0, 75.0)[0]
        assert np.array_equal(ring, w.info["ring"]), p       # mid-bin points take the ring they were made for
        got[p] = ring
    assert (got["one_ring_tile"][T:2 * T] == H // 2).all() and len(set(got["one_ring_tile"][:T])) == H
    assert (got["dead_tile"][T:2 * T] == -1).all() and (got["dead_tile"][:T] >= 0).all() and (got["dead_tile"][2 * T:] >= 0).all()
    late = np.nonzero(got["late_ring"] == H - 2)[0]
    assert len(late) >= 30 and late.min() >= 2 * T and len(set(got["late_ring"][:2 * T])) == H - 1
    e = got["empty_rings"]
    assert set(e[:len(e) // 2]) == {0, H - 1} and set(e[len(e) // 2:]) == {H // 2}
    rr = got["round_robin"]
    d = ds.skew(H, "round_robin").designed
    assert (rr[1:] != rr[:-1])[d[1:] & d[:-1]].all() and np.array_equal(rr[d], np.nonzero(d)[0] % H)
    b = got["blocks"][ds.skew(H, "blocks").designed]
    runs = np.diff(np.nonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))[0])
    assert {64, 65, 512} <= set(runs[1:-1])
    for n in ds.LENGTHS:
        for p in ("round_robin", "blocks", "empty_rings"):
            w = ds.skew(H, p, n)
            assert len(w.x) == n and np.array_equal(ds.classify(w.x, H, 3.0, 75.0)[0], w.info["ring"])
            assert w.designed.all() == (n < 20 * H or p == "empty_rings")


@pytest.mark.parametrize("H", HS)
def test_tiles_and_pitch(H):
    Ts = [8, 9, 17, 64, 65] + ([ds.lookback_tiles(H)] if H == 64 else [])
    assert ds.lookback_tiles(64) == 66
    for T in Ts:
        w = ds.tiles(H, T)
        assert -(-len(w.x) // ds.TILE) == T and len(w.x) % ds.TILE != 0
        ring = ds.classify(w.x, H, 3.0, 75.0)[0]
        assert np.array_equal(ring, w.info["ring"]) and 0.03 < (ring < 0).mean() < 0.07
        if T <= 17:
            for t in range(T):
                assert len(set(ring[t * ds.TILE:(t + 1) * ds.TILE])) == H + 1      # every ring, and dropped points, in every tile
    for kind, top in (("over", P_TEST + 1), ("full", P_TEST), ("under", P_TEST - 1)):
        w = ds.pitch(H, P_TEST, kind)
        cnt = np.diff(ds.split_ref(w.x, H, 3.0, 75.0)[0])
        assert np.array_equal(cnt, w.info["counts"]) and cnt.max() == cnt[H // 2] == top and np.sort(cnt)[-2] < P_TEST
        assert not np.array_equal(w.x, ds.pitch(H, P_TEST, kind, 1).x)


# ---------------------------------------------------------------------------------------------
# the observable is sensitive
# ---------------------------------------------------------------------------------------------
def ring_smoothness(x, members):
    out = np.full(len(members), np.nan)
    if len(members) >= 11:
        out[5:len(members) - 5] = ds.stencil(x[members, :3], ds.taps(len(members)))
    return out


@pytest.mark.parametrize("H", HS)
def test_a_swapped_pair_changes_the_smoothness(H):
    """Every adjacent pair of a ring with a designed point in it and both stencils defined: with the two swapped, the smoothness
    bits change at both positions."""
    for w in ds.worlds(H) + [ds.tiles(H, 9), ds.pitch(H, P_TEST, "over")]:
        offs, order = ds.split_ref(w.x, H, w.min_range, w.max_range)
        pairs = 0
        with np.errstate(over="ignore", invalid="ignore"):
            for r in range(H):
                mem = order[offs[r]:offs[r + 1]]
                n = len(mem)
                if n < 12:
                    continue
                P = w.x[mem, :3]
                t = ds.taps(n)                               # rows: items 5 .. n - 6
                c = ds.stencil(P, t)
                first, second = t[:-1].copy(), t[1:].copy()  # the pair (j, j + 1): item j with taps 5, 6 swapped, j + 1 with 4, 5
                first[:, [5, 6]] = first[:, [6, 5]]
                second[:, [4, 5]] = second[:, [5, 4]]
                des = w.designed[mem][5:n - 6] | w.designed[mem][6:n - 5]
                assert (bits(ds.stencil(P, first)) != bits(c[:-1]))[des].all(), (w.name, r)
                assert (bits(ds.stencil(P, second)) != bits(c[1:]))[des].all(), (w.name, r)
                pairs += int(des.sum())
        if len(w.x) >= 20 * H:
            assert pairs > 0, w.name


@pytest.mark.parametrize("H", HS)
def test_a_point_moved_over_an_edge_changes_the_smoothness(H):
    """Per edge, the designed point nearest to it: given the verdict of the other side it changes the smoothness of the ring it
    leaves and of the ring it joins."""
    w = ds.bin_edges(H)
    lo, hi, vlo, vhi = ds.edges_of(H)
    ring, a, _ = ds.classify(w.x, H, w.min_range, w.max_range)
    di = np.nonzero(w.designed)[0]
    e = w.info["edge_of"]
    for k in range(H + 1):
        cand = di[e == k]
        i = cand[np.argmin(np.abs(a[cand] - hi[k]))]
        assert abs(a[i] - hi[k]) < 1e-5
        other = vhi[k] if ring[i] == vlo[k] else vlo[k]
        moved = ring.copy()
        moved[i] = other
        for r in (ring[i], other):
            if r >= 0:
                assert not np.array_equal(bits(ring_smoothness(w.x, np.nonzero(ring == r)[0])),
                                          bits(ring_smoothness(w.x, np.nonzero(moved == r)[0]))), (H, k, r)
        assert not np.array_equal(ds.partition(ring, H)[0], ds.partition(moved, H)[0])
