"""Designed clouds for the ring split of unorganised scans (lidar_type 0: classify_point and the four partitions k_classify +
k_ring_scatter, k_ring_split, k_ring_split_lb, k_ring_split_fix), and a float64 restatement of the split.  NumPy only,
deterministic, no file I/O.

The restatement (classify, split_ref, smoothness_ref) is written from the statement of the split in liodom_math.h and the
reference lines quoted there (feature_extractor.cc:84-102 isValidPoint, :127-151 the three binning formulas, :115-175 the
append in input order, :195-229 the smoothness), not from the kernels: validity in double, atan(z / dist) * 180 / pi with
libm's atan (element by element: a SIMD arctan need not round like libm), truncation toward zero, the branch of the 64-line
formula at -8.83 with its drop tests at 2 and -24.33, a NaN angle dropped (x = y = 0 with z = 0 and min_range 0: the
reference converts NaN to int, which C++ leaves undefined), and a stable partition by ring.
tests/test_designed_splits.py holds it equal to the oracle on every world.

What the device shows of a split is the ring offsets, the per-ring FP64 smoothness (ring-major: it depends on which point
sits at which position) and the edges with their source indices.  So that this sees everything:
  * every designed point differs from its ring neighbours by metres in x or y (its own range and azimuth, or ordinary points
    between the designed ones of a ring), so a swapped pair changes the smoothness at the swapped positions;
  * the smoothness is undefined for the first and last five points of a ring: with guard=True a world puts, per ring, five
    plain points (mid-bin elevation, mid range, distinct) in front of the cloud and five behind it;
  * the worlds are meant for scan_regions 4, edges_per_region 0 (min_points_per_scan 10: a ring of its guards alone is
    already extracted).

Worlds (World(name, H, min_range, max_range, x, designed, info); `designed` marks the points that are not guards or filler):
  bin_edges(H)       every decision of the binning formula (17 | 33 | 65 edges for H = 16 | 32 | 64, found by bisection on the
                     restatement, the edges into and out of "dropped" included).  Per edge three walks at XY ranges near
                     min_range, mid and near max_range; every point of a walk has its own range and azimuth; z is the float
                     next to range * tan(edge), stepped through -40 .. +40 ulps, plus points at edge +- {3e-6, 3e-5, 1.5e-4,
                     1.9e-4, 2.1e-4, 3e-4, 1e-3} degrees (either side of the 2e-4 degree margin of the float fast path).
  range_limits(H, lo, hi)   the XY range exactly at each limit where floats can say it, x stepped through -40 .. +40 ulps
                     around the limit on the axes and at oblique azimuths, and ranges at +- {0.5, 0.9, 1.1, 2} * 1e-4 relative
                     (either side of the kernel's range margin).  The designed points take rings in turn and every block of H
                     of them is followed by H ordinary ones, so the ring neighbours of a designed point are ordinary.
  odd_values(H)      NaN / inf in one coordinate or in the intensity, magnitudes whose float square overflows or underflows,
                     subnormals, x = y = 0 with z = 0, -0, +-1, a subnormal, huge |z| over a valid XY; rings in turn, every
                     odd point followed by two ordinary ones (its ring's and the ring of 0 degrees).  Run with min_range 0 and with min_range 3.
  skew(H, pattern, n)   the partition, elevations mid-bin: one_ring_tile, dead_tile, late_ring, empty_rings, round_robin,
                     blocks (see skew).  Indices are those of the finished cloud: the guards REPLACE its first and last 5 H
                     points.  A cloud shorter than 20 H points takes no guards; what is then unobserved is said in skew.
  tiles(H, T)        an ordinary mixed cloud of T tiles of 2048 points (the last one 37 short), 5 % invalid.
  pitch(H, P, kind)  for lock-step batches with LIODOM_RING_PITCH=P: ring H // 2 holds P + 1 (`over`), exactly P (`full`) or
                     P - 1 (`under`) points, every other ring fewer.
"""
import functools
import math
from collections import namedtuple

import numpy as np

World = namedtuple("World", "name H min_range max_range x designed info")

TILE = 2048
R_SPLIT, EPR_SPLIT = 4, 0          # scan_regions, edges_per_region the worlds are meant for: min_points_per_scan == 10
GOLD, PLASTIC = 0.6180339887498949, 0.7548776662466927
DELTAS = (3e-6, 3e-5, 1.5e-4, 1.9e-4, 2.1e-4, 3e-4, 1e-3)       # degrees either side of an edge
WALK = np.arange(-40, 41)                                         # float ulps
OBLIQUE_WALKS = 8
REL = (0.5e-4, 0.9e-4, 1.1e-4, 2e-4)                              # relative distance from a range limit
LIMIT_PAIRS = ((3.0, 75.0), (0.5, 120.0), (0.1, 100.3))           # the last pair is not representable in float
LENGTHS = (1, 511, 512, 513, 2047, 2048, 2049, 4097)
PATTERNS = ("one_ring_tile", "dead_tile", "late_ring", "empty_rings", "round_robin", "blocks")


# ---------------------------------------------------------------------------------------------
# the split, restated in float64
# ---------------------------------------------------------------------------------------------
def ring_from_angle(angle, H):
    """Velodyne elevation binning (:127-151); -1: dropped.  int(): truncation toward zero.  A NaN angle is dropped."""
    a = np.asarray(angle, np.float64)
    with np.errstate(invalid="ignore"):
        if H == 64:
            sid = np.where(a >= -8.83, np.trunc((2 - a) * 3.0 + 0.5), H // 2 + np.trunc((-8.83 - a) * 2.0 + 0.5))
            drop = (a > 2) | (a < -24.33) | (sid > 63) | (sid < 0)
        elif H == 32:
            sid = np.trunc((a + 92.0 / 3.0) * 3.0 / 4.0)
            drop = (sid > H - 1) | (sid < 0)
        elif H == 16:
            sid = np.trunc((a + 15) / 2 + 0.5)
            drop = (sid > H - 1) | (sid < 0)
        else:
            raise ValueError(H)
    drop = drop | np.isnan(a)
    return np.where(drop, -1.0, sid).astype(np.int64)


def angle_deg(z, dist):
    """atan(z / distance) * 180 / M_PI (:128) with libm's atan."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.asarray(z, np.float64) / np.asarray(dist, np.float64)
    return np.array([math.atan(v) for v in t.tolist()], np.float64) * 180 / math.pi


def dist64(x, y):
    x, y = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(x * x + y * y)


def classify(xyzi, H, min_range, max_range):
    """(ring id or -1, elevation in degrees, XY range) of every point: isValidPoint (:84-102), then the binning."""
    p = np.asarray(xyzi, np.float32).reshape(-1, 4)
    d = dist64(p[:, 0], p[:, 1])
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(p[:, :3]).all(axis=1) & ~(d > max_range) & ~(d < min_range)
    a = angle_deg(p[:, 2], d)
    return np.where(valid, ring_from_angle(a, H), -1), a, d


def partition(ring, H):
    """(ring offsets [H + 1], source indices ring-major, in input order inside a ring) of ring ids (-1: dropped)."""
    ring = np.asarray(ring)
    keep = np.nonzero(ring >= 0)[0]
    order = keep[np.argsort(ring[keep], kind="stable")]
    offs = np.concatenate([[0], np.cumsum(np.bincount(ring[keep], minlength=H))])
    return offs.astype(np.int32), order.astype(np.int32)


def split_ref(xyzi, H, min_range, max_range):
    """The split: every point's verdict, then the stable partition."""
    return partition(classify(xyzi, H, min_range, max_range)[0], H)


def stencil(P, idx):
    """The smoothness (:195-229) of the items whose eleven taps are the rows of idx (in the order of the sum, the centre in column
    5): float sums from left to right, `10 * x` a float product, the three results widened and squared in double."""
    P = np.asarray(P, np.float32)
    s = P[idx[:, 0]].copy()
    for c in range(1, 5):
        s = s + P[idx[:, c]]
    s = s - np.float32(10) * P[idx[:, 5]]
    for c in range(6, 11):
        s = s + P[idx[:, c]]
    d = s.astype(np.float64)
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def taps(n):
    """Tap indices of the items 5 .. n - 6 of a ring of n points."""
    return np.arange(5, max(5, n - 5))[:, None] + np.arange(-5, 6)[None, :]


def smoothness_ref(xyzi, offs, order, min_points=R_SPLIT * EPR_SPLIT + 10):
    """Ring-major smoothness of a partition, NaN where undefined (the ends of a ring; rings under min_points_per_scan)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(xyzi, np.float32).reshape(-1, 4)
        out = np.full(len(order), np.nan)
        for r in range(len(offs) - 1):
            a, b = int(offs[r]), int(offs[r + 1])
            if b - a >= max(min_points, 11):
                out[a + 5:b - 5] = stencil(x[order[a:b], :3], taps(b - a))
    return out


# ---------------------------------------------------------------------------------------------
# the decisions of the binning formula
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges_of(H):
    """(lo, hi, ring_lo, ring_hi), ascending: adjacent doubles lo < hi at which the verdict changes, by bisection."""
    g = np.linspace(-60.0, 60.0, 120001)
    v = ring_from_angle(g, H)
    k = np.nonzero(v[1:] != v[:-1])[0]
    lo, hi, vlo = g[k].copy(), g[k + 1].copy(), v[k]
    while True:
        mid = lo + (hi - lo) / 2
        live = (mid > lo) & (mid < hi)
        if not live.any():
            break
        same = ring_from_angle(mid, H) == vlo
        lo, hi = np.where(live & same, mid, lo), np.where(live & ~same, mid, hi)
    for a in (lo, hi):
        a.setflags(write=False)
    return lo, hi, vlo, ring_from_angle(hi, H)


@functools.lru_cache(maxsize=None)
def ring_centres(H):
    """Mid-bin elevation of every ring, in degrees."""
    lo, hi, _, vhi = edges_of(H)
    c = np.full(H, np.nan)
    for i in range(len(lo) - 1):
        if vhi[i] >= 0:
            c[vhi[i]] = (hi[i] + lo[i + 1]) / 2
    assert not np.isnan(c).any()
    c.setflags(write=False)
    return c


# ---------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------
def ulp_step(f, k):
    """The float k ulps above f (below for k < 0), through zero and the subnormals."""
    i = np.asarray(f, np.float32).view(np.int32).astype(np.int64)
    key = np.where(i >= 0, i, -(i & 0x7FFFFFFF)) + np.asarray(k, np.int64)
    return np.where(key >= 0, key, (-key) | 0x80000000).astype(np.uint32).view(np.float32)


def polar(d, az):
    return (np.asarray(d) * np.cos(az)).astype(np.float32), (np.asarray(d) * np.sin(az)).astype(np.float32)


def z_at(x, y, angle):
    """The float z next to (XY range of the float x, y) * tan(angle)."""
    return (dist64(x, y) * np.tan(np.radians(angle))).astype(np.float32)


def rows(x, y, z, w=None):
    out = np.zeros((len(x), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = x, y, z
    out[:, 3] = np.arange(len(x)) % 251 if w is None else w
    return out


def plain(rings, H, start=0):
    """One ordinary point per entry of `rings`: mid-bin elevation, a range of 8 .. 58 m and an azimuth of its own (low-discrepancy
    sequences over start + position: neighbours lie metres apart).  An entry of -1 gives an invalid point, of four kinds in
    turn: NaN x, too near (1 m), too far (90 m), 45 degrees up (outside every field of view)."""
    rings = np.asarray(rings, np.int64)
    i = np.arange(start, start + len(rings), dtype=np.float64)
    d = 8.0 + 50.0 * ((i * GOLD) % 1.0)
    dead = rings < 0
    kind = np.arange(len(rings)) % 4
    d = np.where(dead & (kind == 1), 1.0, np.where(dead & (kind == 2), 90.0, d))
    x, y = polar(d, 2 * np.pi * ((i * PLASTIC) % 1.0))
    ang = np.where(dead & (kind == 3), 45.0, ring_centres(H)[np.maximum(rings, 0)])
    out = rows(x, y, z_at(x, y, ang))
    out[dead & (kind == 0), 0] = np.nan
    return out


def guards(H, which):
    return plain(np.tile(np.arange(H), 5), H, start=(1 + which) * 10_000_019)


def finish(name, H, lo, hi, body, guard, info=None):
    """The world of a body, with the guards in front of it and behind it."""
    designed = np.ones(len(body), bool)
    if guard:
        body = np.concatenate([guards(H, 0), body, guards(H, 1)])
        designed = np.concatenate([np.zeros(5 * H, bool), designed, np.zeros(5 * H, bool)])
    body = np.ascontiguousarray(body, np.float32)
    body.setflags(write=False)
    designed.setflags(write=False)
    return World(name, H, float(lo), float(hi), body, designed, info or {})


def from_rings(name, H, r, guard, start, info=None, absent=None):
    """A world of plain points from ring ids.  The guards REPLACE the first and last 5 H ids (a cloud under 20 H points stays as
    it is); `absent`: a ring that gets no guards in front (its place goes to the ring above it)."""
    r = np.array(r, np.int64)
    n = len(r)
    designed = np.ones(n, bool)
    if guard and n >= 20 * H:
        g = np.tile(np.arange(H), 5)
        r[:5 * H], r[n - 5 * H:] = np.where(g == absent, g + 1, g) if absent is not None else g, g
        designed[:5 * H] = designed[n - 5 * H:] = False
    x = plain(r, H, start=start)
    for a in (x, designed, r):
        a.setflags(write=False)
    return World(name, H, 3.0, 75.0, x, designed, dict(info or {}, ring=r))


def in_turn(x, y, H, z=None, w=None, start=0):
    """Designed points (x, y) on rings 0, 1, .. H - 1, 0, .. (z: mid-bin of that ring unless given), every block of H of them
    followed by H ordinary points, one per ring.  Returns (cloud, mask of the designed points)."""
    m = len(x)
    ring = np.arange(m) % H
    zz = z_at(x, y, ring_centres(H)[ring]) if z is None else z
    pts = rows(x, y, zz, w)
    out, mask = [], []
    for b in range(0, m, H):
        out += [pts[b:b + H], plain(np.arange(H), H, start=start + b)]
        mask += [np.ones(len(pts[b:b + H]), bool), np.zeros(H, bool)]
    return np.concatenate(out), np.concatenate(mask)


# ---------------------------------------------------------------------------------------------
# worlds
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bin_edges(H, guard=True):
    lo, hi, _, _ = edges_of(H)
    rng = np.random.default_rng(1000 + H)
    per = len(WALK) + 2 * len(DELTAS)
    dl = np.array([s * d for d in DELTAS for s in (-1.0, 1.0)])
    out, edge_of = [], []
    for e in range(len(lo)):
        for base in (3.5, 30.0, 70.0):
            x, y = polar(base + 0.013 * rng.permutation(per), rng.uniform(0.0, 2 * np.pi, per))
            z = z_at(x, y, np.concatenate([np.full(len(WALK), hi[e]), hi[e] + dl]))
            z[:len(WALK)] = ulp_step(z[:len(WALK)], WALK)
            out.append(rows(x, y, z))
            edge_of.append(np.full(per, e))
    w = finish("bin_edges", H, 3.0, 75.0, np.concatenate(out), guard)
    return w._replace(info=dict(edge_of=np.concatenate(edge_of), n_edges=len(lo)))


@functools.lru_cache(maxsize=None)
def range_limits(H, lo=3.0, hi=75.0, guard=True):
    """info: `limit` (0 / 1: which limit a designed point belongs to, in the order of the designed points) and `steps` (ulps in x
    from the float at which the range crosses the limit; 99 for the points placed by relative distance)."""
    rng = np.random.default_rng(2000 + H)
    xs, ys, lim, steps = [], [], [], []

    def add(x, y, which, k):
        xs.append(np.asarray(x, np.float32).reshape(-1)); ys.append(np.asarray(y, np.float32).reshape(-1))
        lim.append(np.full(len(xs[-1]), which)); steps.append(np.broadcast_to(np.asarray(k), xs[-1].shape))

    for which, L in enumerate((lo, hi)):
        f = np.float32(L)
        # on the axes: the limit itself where a float holds it, and the walk; the axis changes from point to point
        ax = ulp_step(np.full(len(WALK) + 4, f), np.concatenate([[0, 0, 0, 0], WALK]))
        turn = np.arange(len(ax)) % 4
        sgn = np.where(turn < 2, 1.0, -1.0).astype(np.float32)
        add(np.where(turn % 2 == 0, sgn * ax, 0), np.where(turn % 2 == 1, sgn * ax, 0), which, np.concatenate([[0, 0, 0, 0], WALK]))
        if float(np.float32(0.6 * L)) == 0.6 * L and float(np.float32(0.8 * L)) == 0.8 * L:       # a 3-4-5 triangle in floats
            add([0.6 * L, -0.8 * L], [0.8 * L, 0.6 * L], which, 0)
        # oblique: y fixed by the azimuth (within 60 degrees of the x axis, so a step of x moves the range), x walks
        # (several walks: among the points within an ulp of the limit, a few have a float range on the other side of it than the
        #  double one; tests/test_designed_splits.py asserts that every limit of every world has such a point)
        for _ in range(OBLIQUE_WALKS):
            az = rng.uniform(-np.pi / 3, np.pi / 3, len(WALK))
            y = (L * np.sin(az)).astype(np.float32)
            x0 = np.sqrt(L * L - y.astype(np.float64) ** 2).astype(np.float32)
            add(ulp_step(x0, WALK) * rng.choice(np.array([-1.0, 1.0], np.float32), len(WALK)), y, which, WALK)
        # either side of the margin of the float fast path
        rel = np.array([s * r for r in REL for s in (-1.0, 1.0)] * 2)
        x, y = polar(L * (1.0 + rel), rng.uniform(0.0, 2 * np.pi, len(rel)))
        add(x, y, which, 99)
    body, mask = in_turn(np.concatenate(xs), np.concatenate(ys), H, start=3000)
    w = finish("range_limits_%g_%g" % (lo, hi), H, lo, hi, body, guard)
    designed = w.designed.copy()
    designed[w.designed] = mask
    designed.setflags(write=False)
    return w._replace(designed=designed, info=dict(limit=np.concatenate(lim), steps=np.concatenate(steps)))


def odd_points():
    """[(x, y, z, w)]: None = the ordinary value of the ring whose turn it is."""
    nan, inf = float("nan"), float("inf")
    o = []
    for c in range(3):                                   # non-finite in one coordinate alone
        for v in (nan, inf, -inf):
            o.append(tuple(v if k == c else None for k in range(3)) + (None,))
    o += [(None, None, None, v) for v in (nan, inf, -inf)]            # the intensity is no reason to drop
    for m in (1e19, 2e19, 1e30):                         # the float square overflows (2e19, 1e30), the double does not
        o += [(m, None, None, None), (None, m, None, None), (m, m, 0.0, None), (-m, None, None, None), (m, -m, m, None)]
    for m in (1e19, 1e30, 3e38):                         # |z| huge over a valid XY
        o += [(None, None, m, None), (None, None, -m, None)]
    for t in (1e-30, 1e-40, 1.4e-45):                    # the float square underflows to 0; subnormals
        o += [(t, 0.0, 0.0, None), (0.0, t, 0.0, None), (t, t, 0.0, None), (-t, 0.0, -0.0, None), (t, 0.0, t, None),
              (t, 0.0, -t, None), (t, None, None, None)]
    o += [(1e-30, 0.0, 1e-40, None), (1e-30, 0.0, -1e-40, None), (1e-20, 1e-20, 1e-22, None)]
    for z in (0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40):      # x = y = 0
        o += [(0.0, 0.0, z, None), (-0.0, 0.0, z, None), (0.0, -0.0, z, None)]
    o += [(0.0, 0.0, 0.0, None), (0.0, 0.0, 1.0, None), (-0.0, 0.0, -0.0, None), (1e-30, 0.0, 0.0, None), (5.0, 0.0, 0.0, None), (0.0, 0.0, -1.0, None)]
    return o


@functools.lru_cache(maxsize=None)
def odd_values(H, min_range=3.0, guard=True):
    """Every odd point three times (so that it meets three rings); `info["odd"]`: its index into odd_points(), in the order of
    the designed points."""
    odd = odd_points()
    which = np.tile(np.arange(len(odd)), 3)
    m = len(which)
    base = plain(np.arange(m) % H, H, start=5000)          # (ring i mod H: the ring in_turn gives the point)
    pts = base.copy()
    with np.errstate(over="ignore"):
        for i, k in enumerate(which):
            for c, v in enumerate(odd[k]):
                if v is not None:
                    pts[i, c] = v
    # every odd point is followed by an ordinary one of the ring whose turn it is and by one of the ring of 0 degrees, where the
    # tiny points land with min_range 0: no two odd points are neighbours in a ring
    zero = int(ring_from_angle(0.0, H))
    body = np.empty((3 * m, 4), np.float32)
    body[0::3], body[1::3], body[2::3] = pts, plain(np.arange(m) % H, H, start=6000), plain(np.full(m, zero), H, start=6500)
    mask = np.arange(3 * m) % 3 == 0
    wd = finish("odd_values_%g" % min_range, H, min_range, 75.0, body, guard)
    designed = wd.designed.copy()
    designed[wd.designed] = mask
    designed.setflags(write=False)
    return wd._replace(designed=designed, info=dict(odd=which))


def _mixed(n, H, seed, dead=0.0):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, H, n)
    if dead:
        r[rng.random(n) < dead] = -1
    return r


@functools.lru_cache(maxsize=None)
def skew(H, pattern, n=None, guard=True):
    """Ring ids by pattern (indices of the finished cloud; the guards replace its first and last 5 H points):
      one_ring_tile  3 tiles + 17: tile 1 — points 2048 .. 4095 — all in ring H // 2, the rest mixed;
      dead_tile      the same with tile 1 all invalid (the four kinds of plain());
      late_ring      2 tiles + 300 + 5 H: ring H - 2 receives points only from the last tile (every third point from 4100 on);
      empty_rings    n points (default 4097): the first half in rings 0 and H - 1 alternately, the second half in ring H // 2;
      round_robin    n points (default 4097): point i in ring i mod H;
      blocks         n points (default 4097): runs of 64, 65 and 512 points per ring in turn, so the runs start aligned and
                     misaligned to the wave and to the 512-thread sweep.
    A cloud under 20 H points takes no guards (n = 1, 511, 512, 513 at H = 32 and 64, n = 1 at H = 16): there the rings' first
    and last five points — for rings under 11 points all of them — are seen through the ring offsets alone, which still count
    every verdict but cannot tell a swapped pair."""
    mid = H // 2
    if pattern in ("one_ring_tile", "dead_tile"):
        n = 3 * TILE + 17 if n is None else n
        r = _mixed(n, H, 41)
        r[TILE:2 * TILE] = mid if pattern == "one_ring_tile" else -1
    elif pattern == "late_ring":
        n = 2 * TILE + 300 + 5 * H if n is None else n
        r = _mixed(n, H - 1, 42)
        r[r == H - 2] = H - 1
        r[2 * TILE + 4::3] = H - 2
    else:
        n = 4097 if n is None else n
        i = np.arange(n)
        if pattern == "empty_rings":
            r = np.where(i < n // 2, np.where(i % 2 == 0, 0, H - 1), mid)
        elif pattern == "round_robin":
            r = i % H
        elif pattern == "blocks":
            runs = np.tile([64, 65, 512], 1 + n // 641 + 1)
            r = np.repeat(np.arange(len(runs)) % H, runs)[:n]
        else:
            raise ValueError(pattern)
    assert len(r) == n
    return from_rings("skew_%s_%d" % (pattern, n), H, r, guard and pattern != "empty_rings", 7000,
                      absent=H - 2 if pattern == "late_ring" else None)


@functools.lru_cache(maxsize=None)
def tiles(H, T, guard=True):
    n = T * TILE - 37
    r = _mixed(n, H, 50 + T, dead=0.05)
    return from_rings("tiles_%d" % T, H, r, guard, 8000, info=dict(tiles=T))


@functools.lru_cache(maxsize=None)
def pitch(H, P, kind, seed=0):
    """Ring H // 2 holds P + 1 (`over`), P (`full`) or P - 1 (`under`) points, the guards counted; ring r otherwise
    P // 2 + r.  The body is shuffled (seeded)."""
    cnt = P // 2 + np.arange(H)
    assert cnt.max() < P - 1 and cnt.min() > 10
    cnt[H // 2] = P + {"over": 1, "full": 0, "under": -1}[kind]
    r = np.repeat(np.arange(H), cnt - 10)
    r = r[np.random.default_rng(60 + seed).permutation(len(r))]
    w = finish("pitch_%s_%d" % (kind, seed), H, 3.0, 75.0, plain(r, H, start=9000 + 100000 * seed), True)
    return w._replace(info=dict(counts=cnt))


# ---------------------------------------------------------------------------------------------
# what the tests run
# ---------------------------------------------------------------------------------------------
def worlds(H):
    """Worlds 1 - 4 as every path runs them: the decisions, the odd values with both min_range, every skew pattern at its own
    length and the length-independent ones at every cloud length."""
    ws = [bin_edges(H)] + [range_limits(H, lo, hi) for lo, hi in LIMIT_PAIRS] + [odd_values(H, 0.0), odd_values(H, 3.0)]
    ws += [skew(H, p) for p in PATTERNS]
    ws += [skew(H, p, n) for n in LENGTHS[:-1] for p in ("round_robin", "blocks", "empty_rings")]
    return ws


def batch_tails(H):
    """World 5 for one stream: 8 | 9 | 17 tiles (k_ring_scatter sums 8 tiles per batch), 64 | 65 (k_ring_split reads 64)."""
    return [tiles(H, T) for T in (8, 9, 17, 64, 65)]


def lookback_tiles(H):
    """The tile count at which k_ring_split_lb's look-back runs a second batch: 8 * (512 / H) + 2 (66 tiles at H = 64)."""
    return 8 * (512 // H) + 2
