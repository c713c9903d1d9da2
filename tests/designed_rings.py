"""Designed rings for the edge extraction (k_ring_extract, k_compact_edges; the splits k_row_compact, k_ring_split, k_classify +
k_ring_scatter and k_ring_split_lb feed them): inputs that reach, on purpose, the decisions that scenes and jagged rings reach
by accident or never.  NumPy only, deterministic, no file I/O.

Base ring: x = 16, y = k / 64, z = 0, intensity = k.  Everything is dyadic, so every 11-tap float sum is exact and the smoothness
is exactly 0 away from a bump.  A bump d in x at one point gives that item (10 d - neighbouring bumps)^2 and the ten items around
it d^2.  Consecutive points are 1/64 m apart (squared gap <= 0.05: continuous); a discontinuity is a step of 0.25 m in y.  A ring
longer than 4001 points folds back and forth in y (legs of 4000 steps, a parabolic turn over 8 steps whose smoothness stays
below 0.1), so that every point stays inside max_range.  z = 0 is ring 8 of the 16-line formula (bumps in z are positive, so
they stay there); the same ring is a row of a lidar_type 1 cloud (pack: shorter rows padded with NaN points).

A family is a Case(name, R, epr, rows, info): the rings, the (scan_regions, edges_per_region) they are designed for and one
dict per ring that says what the ring must show.  The conditions are asserted in tests/test_designed_rings.py on the oracle's
output (smoothness and picks), never taken for granted:

  ties(R)        sector 240.  c_lo = 1.5625 (bump 0.125 in x) at the lower index and c_hi = 1.5625 + 100 * 2^-32 (the same bump
                 plus 2^-16 in z) at the higher one: float32(c_hi) == float32(c_lo), c_hi > c_lo.  Region 0: both items of one
                 lane (offsets 50, 57: one block of 16 and of 24 items); region 1: neighbouring lanes of one quad (100, 120),
                 behind a stronger first pick, so the tie is among the second and third picks; region 2: lanes of different
                 quads (60, 200) and a third item with the same image (130, c_lo again); region 3: two identical bumps (70,
                 150), an exact tie of doubles that the lower index wins.  Condition: the images are equal, the doubles ordered
                 as said, and every tied item is picked, in the order largest double first, lowest index among equal doubles.
  cutoff(R)      sector 40, two rings, one bumped item each (in z, fine-tuned in y, at a point with y = 0): `below` has
                 c < 0.1 with float32(c) == float32(0.1) and yields no edge; `at_least` has the smallest c >= 0.1 the same
                 search reaches (its image is float32(0.1) too) and yields one.  No other item reaches 0.1.
  gaps(R)        sector 80, epr >= 5.  One strong pick j (bump 0.1875) in region 1, weak candidates at j -+ 5 (0.09375) and
                 j -+ 6 (0.0625).  Rows `gap`: for (j - 4) mod 32 in 22..31 and 0 (the 10-bit window of the continuity bits
                 ends in, or crosses into, the next word) x the ten positions k = j-4 .. j+5 of the only discontinuity; rows
                 `threshold`: a step between j+2 and j+3 of f (f^2 <= 0.05: continuous) and of nextafter(f) (f'^2 > 0.05);
                 rows `lane`: no discontinuity, j at region offset 15, 16, 23, 24 (the suppression crosses into the next lane of
                 the 16- and the 24-item instance); row `ends`: picks at j = 5 and j = nr - 6.  Condition: j is picked, nothing
                 else in [j - nb, j + nf], and the first candidate beyond each extent (j + nf + 1, j - nb - 1) is picked.
  cascade(R, variant)   epr 1.  `base`: sector 8, a weak candidate C at offset 6 of every region (0.0625) and a strong one A at
                 offset 1 of every region but the first (0.125): in order every region picks C, whose spill masks the next A;
                 speculatively every region >= 1 picks A, and each carry round repairs one region: jacobi_rounds == R - 1.
                 `twice`: C and a twin at offset 7 (0.078125 each) and E at offset 4 (0.0625): the spill-free run of a region
                 >= 1 picks A and the twin, whose spill (31) hits the next A; the re-run's pick spills 7, then 1: regions >= 2
                 are re-run with one non-zero mask after another, and their picks change with it.  `sector5`: sector 5, a
                 pick on the last item of a region masks the whole next region.
  boundaries()   one ring per case, candidates at seeded places with continuous gaps (suppression is active on the generic
                 path too): the longest region at 256 | 257 and 384 | 385 items, sector 5 | 4, R 64 | 65, nr 16384 | 16385, R
                 no multiple of 4, nr = R * epr + 10 and one below, a last region longer than the others by R - 1.
  counts(H, pattern, epr)   whole lidar_type 1 clouds of H rows of 150 points with a prescribed number of edges per ring (one
                 bump of 0.25 per wanted pick: discontinuous to its neighbours, 11 items apart): `full` (every ring R * (epr + 1)),
                 `ends_empty`, `middle_run`, `last_only`.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name R epr rows info")

LEG = 4000                      # steps of 1/64 m per leg of a folded ring
GAP_STEP = 0.25                 # a discontinuity: 0.0625 > 0.05
STRONG, A_DX, MID, C_DX = 0.1875, 0.125, 0.09375, 0.0625
F32_TENTH = np.float32(0.1)


# ---------------------------------------------------------------------------------------------
# rings
# ---------------------------------------------------------------------------------------------
def _exact32(a):
    b = np.asarray(a, np.float64).astype(np.float32)
    assert np.array_equal(b.astype(np.float64), np.asarray(a, np.float64)), "a designed coordinate is not a float"
    return b


def base_y(n, k0=0):
    """y of the base ring in float64: (k + k0) / 64 up to LEG steps, then folded (slopes in units of 1/512 m)."""
    if n <= LEG + 1:
        return (np.arange(n) + k0) / 64.0
    up, down = [7, 5, 3, 1, -1, -3, -5, -7], [-7, -5, -3, -1, 1, 3, 5, 7]
    cycle = [8] * LEG + up + [-8] * LEG + down
    s = np.array((cycle * ((n - 1) // len(cycle) + 1))[:n - 1], np.float64)
    return (np.concatenate([[0.0], np.cumsum(s)]) + 8 * k0) / 512.0


def base_ring(n, k0=0):
    r = np.zeros((n, 4), np.float64)
    r[:, 0] = 16.0
    r[:, 1] = base_y(n, k0)
    r[:, 3] = np.arange(n)
    return r


def smoothness(ring):
    """The reference's smoothness of every ring point (float 11-tap sums left to right, squares and their sum in double,
    feature_extractor.cc:196-229); NaN for the first and last five."""
    P = np.ascontiguousarray(ring[:, :3], np.float32)
    n = len(P)
    c = np.full(n, np.nan)
    if n < 11:
        return c
    m = n - 10
    s = P[0:m].copy()
    for o in (1, 2, 3, 4):
        s = s + P[o:o + m]
    s = s - np.float32(10) * P[5:5 + m]
    for o in (6, 7, 8, 9, 10):
        s = s + P[o:o + m]
    assert s.dtype == np.float32
    d = s.astype(np.float64)
    c[5:n - 5] = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return c


def continuity(ring):
    """ok[k]: the squared gap between points k - 1 and k is not above 0.05 (float differences, squares in double, :281-307)."""
    P = np.ascontiguousarray(ring[:, :3], np.float32)
    d = (P[1:] - P[:-1]).astype(np.float64)
    g = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return np.concatenate([[False], ~(g > 0.05)])


def extents(ring, j):
    """(nf, nb) of a pick at j: how far the +-5 suppression reaches before a discontinuity (:280-310)."""
    ok = continuity(ring)
    nf = nb = 5
    for l in range(1, 6):
        if not ok[j + l]:
            nf = l - 1
            break
    for l in range(1, 6):
        if not ok[j - l + 1]:
            nb = l - 1
            break
    return nf, nb


def regions_of(n, R):
    """[(first, end)] of the R regions in ring indices (:238-252)."""
    total = n - 10
    sector = total // R
    return [(5 + sector * g, 5 + (total if g == R - 1 else sector * (g + 1))) for g in range(R)]


def pack(rows, H=None, W=None):
    """The rows as one lidar_type 1 cloud: (cloud [H * W, 4], H, W).  None = an empty row; short rows end in NaN points."""
    H = len(rows) if H is None else H
    W = max([len(r) for r in rows if r is not None] + [1]) if W is None else W
    x = np.full((H, W, 4), np.nan, np.float32)
    for i, r in enumerate(rows):
        if r is not None:
            x[i, :len(r)] = r
    return x.reshape(-1, 4), H, W


# ---------------------------------------------------------------------------------------------
# plain selection: the reference's loop per region, and the carry as a fixed-point iteration
# ---------------------------------------------------------------------------------------------
def _key_reference(c):
    return c


def _key_image(c):
    return float(np.float32(c))


def select_region(c, ok, first, end, epr, marked, key=_key_reference, below=lambda c: c < 0.1):
    """The reference's walk over one region (sort by smoothness, ties by index; stop at the first unmarked item below the
    cut-off or after epr + 1 picks; mark +-5 up to a discontinuity, feature_extractor.cc:254-312).  `marked` is updated.
    Returns [(j, nf)]."""
    items = sorted(range(first, end), key=lambda j: (-key(c[j]), j))
    picks = []
    for j in items:
        if marked[j]:
            continue
        if below(c[j]) or len(picks) > epr:
            break
        marked[j] = True
        nf = 0
        for l in range(1, 6):
            if not ok[j + l]:
                break
            marked[j + l] = True
            nf = l
        for l in range(1, 6):
            if not ok[j - l + 1]:
                break
            marked[j - l] = True
        picks.append((j, nf))
    return picks


def select_ring(ring, R, epr, rule="reference"):
    """Picks of one ring, regions in order.  rule: `reference`; `image_lowest_index`: the lowest index among equal FLOAT IMAGES
    wins, the doubles are never compared; `cutoff_on_image`: the 0.1 cut-off is taken on the float image.  The two wrong rules
    are what a kernel that decided on its 32-bit keys alone would do."""
    if len(ring) < R * epr + 10:                                   # below min_points_per_scan (params.cc:63, feature_extractor.cc:188)
        return []
    c, ok = smoothness(ring), continuity(ring)
    key = _key_image if rule == "image_lowest_index" else _key_reference
    below = (lambda v: np.float32(v) < F32_TENTH) if rule == "cutoff_on_image" else (lambda v: v < 0.1)
    marked = [False] * len(ring)
    out = []
    for first, end in regions_of(len(ring), R):
        out += [j for j, _ in select_region(c, ok, first, end, epr, marked, key, below)]
    return out


def jacobi(ring, R, epr):
    """The in-order walk as the fixed point of `region g = select(region g | forward spill of region g - 1)`, iterated for all
    regions at once from the spill-free selection.  Returns (rounds in which some region's picks changed, final picks per region,
    [incoming masks per region] per round: bit o = item o of the region is marked by its predecessor, and the re-marks
    [(region, old mask, new mask)]: a region whose picks already come from a run with a non-zero mask — one that hit a pick of
    the spill-free run — gets another mask)."""
    c, ok = smoothness(ring), continuity(ring)
    regs = regions_of(len(ring), R)

    def run(g, mask):
        first, end = regs[g]
        marked = [False] * len(ring)
        for o in range(5):
            if (mask >> o) & 1:
                marked[first + o] = True
        return select_region(c, ok, first, end, epr, marked)

    def spill(g, picks):
        m = 0
        for j, nf in picks:
            for l in range(1, nf + 1):
                if j + l >= regs[g][1]:
                    m |= 1 << (j + l - regs[g][1])
        return m

    picks = [run(g, 0) for g in range(R)]
    rounds, history, used, remarks = 0, [], [0] * R, []
    while True:
        masks = [0] + [spill(g, picks[g]) for g in range(R - 1)]
        history.append(masks)
        for g in range(R):
            if masks[g] != used[g]:
                if used[g]:
                    remarks.append((g, used[g], masks[g]))
                    used[g] = masks[g]
                elif any(j - regs[g][0] < 5 and (masks[g] >> (j - regs[g][0])) & 1 for j, _ in picks[g]):
                    used[g] = masks[g]
        new = [run(g, masks[g]) for g in range(R)]
        if new == picks:
            return rounds, [[j for j, _ in p] for p in picks], history, remarks
        picks = new
        rounds += 1
        assert rounds <= R, "no fixed point"


def jacobi_rounds(ring, R, epr):
    return jacobi(ring, R, epr)[0]


# ---------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------
def _bump(r, j, dx=0.0, dy=0.0, dz=0.0):
    r[j, 0] += dx
    r[j, 1] += dy
    r[j, 2] += dz


TIE_DZ = 2.0 ** -16


def ties(R=4):
    assert R >= 4
    sector = 240
    n = 10 + R * sector
    r = base_ring(n)
    b = [5 + sector * g for g in range(R)]
    lo = lambda j: _bump(r, j, dx=A_DX)
    hi = lambda j: _bump(r, j, dx=A_DX, dz=TIE_DZ)
    lo(b[0] + 50); hi(b[0] + 57)
    _bump(r, b[1] + 20, dx=STRONG); lo(b[1] + 100); hi(b[1] + 120)
    lo(b[2] + 60); lo(b[2] + 130); hi(b[2] + 200)
    lo(b[3] + 70); lo(b[3] + 150)
    info = dict(
        # (lower index with c_lo, higher index with c_hi > c_lo of the same image, placement)
        pairs=[(b[0] + 50, b[0] + 57, "lane"), (b[1] + 100, b[1] + 120, "quad"), (b[2] + 60, b[2] + 200, "quads")],
        equal=[(b[2] + 60, b[2] + 130), (b[3] + 70, b[3] + 150)],
        order={0: [b[0] + 57, b[0] + 50], 1: [b[1] + 20, b[1] + 120, b[1] + 100],
               2: [b[2] + 200, b[2] + 60, b[2] + 130], 3: [b[3] + 70, b[3] + 150]},
        sector=sector)
    return Case("ties", R, 3, [_exact32(r)], [info])


def _cutoff_search():
    """Deterministic: the z bump is fixed, the y perturbation walks 8193 consecutive floats; the item has y = 0, its neighbours
    (i - 5) / 64.  Returns (dz, dy just below, c below, dy at least, c at least)."""
    dz = np.float32(0.03160499408841133)
    u = np.float32(0.0010603659320622683).view(np.uint32) + np.arange(-4096, 4097)
    dy = u.astype(np.uint32).view(np.float32)
    w = np.zeros((len(dy), 11, 3), np.float32)
    w[:, :, 0] = 16.0
    w[:, :, 1] = ((np.arange(11) - 5) / 64.0).astype(np.float32)
    w[:, 5, 1] = dy
    w[:, 5, 2] = dz
    s = w[:, 0].copy()
    for o in (1, 2, 3, 4):
        s = s + w[:, o]
    s = s - np.float32(10) * w[:, 5]
    for o in (6, 7, 8, 9, 10):
        s = s + w[:, o]
    d = s.astype(np.float64)
    c = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    below = np.nonzero((c < 0.1) & (c.astype(np.float32) == F32_TENTH))[0]
    above = np.nonzero(c >= 0.1)[0]
    assert len(below) and len(above)
    ib, ia = below[np.argmax(c[below])], above[np.argmin(c[above])]
    return dz, dy[ib], float(c[ib]), dy[ia], float(c[ia])


def cutoff(R=4):
    sector = 40
    n = 10 + R * sector
    j = 5 + sector + 20
    dz, dy_b, c_b, dy_a, c_a = _cutoff_search()
    rows, info = [], []
    for kind, dy, c in (("below", dy_b, c_b), ("at_least", dy_a, c_a)):
        r = base_ring(n, k0=-j).astype(np.float32)
        r[j, 1] = dy
        r[j, 2] = dz
        rows.append(r)
        info.append(dict(kind=kind, j=j, c=c, edges=[] if kind == "below" else [j]))
    return Case("cutoff", R, 1, rows, info)


GAP_SHIFTS = list(range(22, 32)) + [0]
GAP_POSITIONS = list(range(-4, 6))


def _gap_row(n, j, k0=0):
    r = base_ring(n, k0)
    _bump(r, j, dx=STRONG)
    for o, d in ((5, MID), (6, C_DX)):
        if j - o >= 5:
            _bump(r, j - o, dx=d)
        if j + o <= n - 6:
            _bump(r, j + o, dx=d)
    return r


def threshold_step():
    """The largest float f with f * f <= 0.05 in double."""
    f = np.float32(np.sqrt(0.05))
    while float(f) * float(f) > 0.05:
        f = np.nextafter(f, np.float32(0))
    while float(np.nextafter(f, np.float32(1))) ** 2 <= 0.05:
        f = np.nextafter(f, np.float32(1))
    return f


def gaps(R=2):
    assert R >= 2
    sector = 80
    n = 10 + R * sector
    first = 5 + sector                                    # region 1
    rows, info = [], []
    for sh in GAP_SHIFTS:
        j = 100 + sh if sh else 132                       # (j - 4) mod 32 == sh; region offsets 37 .. 47: all of it inside region 1
        for p in GAP_POSITIONS:
            r = _gap_row(n, j)
            r[j + p:, 1] += GAP_STEP
            rows.append(_exact32(r))
            info.append(dict(kind="gap", j=j, shift=sh, pos=p, nf=p - 1 if p >= 1 else 5, nb=-p if p <= 0 else 5))
    f = threshold_step()
    for step, nf in ((f, 5), (np.nextafter(f, np.float32(1)), 2)):
        j = first + 40
        r = _exact32(_gap_row(n, j, k0=-(j + 2)))         # y = 0 at j + 2, so that the float difference across the step is `step`
        r[j + 3:, 1] = np.float32(step) + (np.arange(n - j - 3) / 64.0).astype(np.float32)
        assert r.dtype == np.float32 and r[j + 2, 1] == 0 and r[j + 3, 1] - r[j + 2, 1] == step
        rows.append(r)
        info.append(dict(kind="threshold", j=j, step=float(step), nf=nf, nb=5))
    for off in (15, 16, 23, 24):
        rows.append(_exact32(_gap_row(n, first + off)))
        info.append(dict(kind="lane", j=first + off, nf=5, nb=5))
    r = base_ring(n)
    for j, o in ((5, 1), (n - 6, -1)):
        _bump(r, j, dx=STRONG)
        _bump(r, j + 5 * o, dx=MID)
        _bump(r, j + 6 * o, dx=C_DX)
    rows.append(_exact32(r))
    info.append(dict(kind="ends", j=5, j2=n - 6, nf=5, nb=5))
    return Case("gaps", R, 5, rows, info)


def cascade(R, variant="base"):
    sector = 5 if variant == "sector5" else 8
    n = 10 + R * sector
    r = base_ring(n)
    b = [5 + sector * g for g in range(R)]
    info = dict(variant=variant, sector=sector)
    if variant == "base":
        for g in range(R):
            _bump(r, b[g] + 6, dx=C_DX)
            if g:
                _bump(r, b[g] + 1, dx=A_DX)
        info["C"] = [b[g] + 6 for g in range(R)]
    elif variant == "twice":
        for g in range(R):
            _bump(r, b[g] + 6, dx=0.078125)
            _bump(r, b[g] + 7, dx=0.078125)
            if g:
                _bump(r, b[g] + 1, dx=A_DX)
                _bump(r, b[g] + 4, dx=C_DX)
    else:
        # a weak candidate on the last item of every region, a strong one on the first item of every region but the first
        for g in range(R):
            _bump(r, b[g] + 4, dx=C_DX)
            if g:
                _bump(r, b[g], dx=-A_DX)
    return Case("cascade_%s_%d" % (variant, R), R, 1, [_exact32(r)], [info])


def _candidates(n, seed):
    """A ring with bumps at seeded places, 2 to 9 items apart (2 to 4 on a ring of fewer than 100 points), every gap continuous."""
    rng = np.random.default_rng(seed)
    r = base_ring(n)
    j = 5 + int(rng.integers(0, 4))
    sizes = np.array([C_DX, MID, A_DX, STRONG, -C_DX, -MID, -A_DX, -STRONG])
    while j < n - 5:
        _bump(r, j, dx=float(sizes[rng.integers(0, len(sizes))]))
        j += int(rng.integers(2, 10 if n >= 100 else 5))      # (a short ring: closer together, so that picks mark candidates)
    r = _exact32(r)
    assert continuity(r)[1:].all()
    return r


# (name, R, epr, ring length, instance: items per lane that the handle's max_width selects)
BOUNDARY_SHAPES = [
    ("len256", 4, 2, 10 + 4 * 256, 16), ("len257", 4, 2, 10 + 4 * 256 + 1, 16),
    ("len384", 4, 2, 10 + 4 * 384, 24), ("len385", 4, 2, 10 + 4 * 384 + 1, 24),
    ("sector5", 8, 1, 10 + 8 * 5, 16), ("sector4", 8, 1, 10 + 8 * 5 - 1, 16),
    ("r64", 64, 1, 10 + 64 * 8, 16), ("r65", 65, 1, 10 + 65 * 8, 16),
    ("nr16384", 64, 1, 16384, 24), ("nr16385", 64, 1, 16385, 24),
    ("r6_min", 6, 5, 6 * 5 + 10, 16), ("r6_below_min", 6, 5, 6 * 5 + 9, 16),
    ("r6_long_last", 6, 2, 10 + 6 * 20 + 5, 16), ("r7", 7, 2, 10 + 7 * 30 + 3, 16),
]


def register_path(n, R, ipl):
    """Whether a ring of n points stays on the register path of the instance with `ipl` items per lane: the shape test of
    k_ring_extract (regions of 5 .. 16 * ipl items, at most 64 regions, at most 16384 points)."""
    total = n - 10
    sector = total // R
    longest = max(sector, total - sector * (R - 1))
    return longest <= 16 * ipl and sector >= 5 and R <= 64 and n <= 16384


def width_for(R, ipl):
    """A max_width that makes liodom_create choose the instance with `ipl` items per lane for R regions."""
    return 10 + R * (200 if ipl == 16 else 300)


def boundaries():
    return [Case(name, R, epr, [_candidates(n, seed=100 + i)], [dict(n=n, ipl=ipl, fast=register_path(n, R, ipl))])
            for i, (name, R, epr, n, ipl) in enumerate(BOUNDARY_SHAPES)]


COUNT_W = 150
COUNT_R = 4
COUNT_PATTERNS = ("full", "ends_empty", "middle_run", "last_only")


def wanted_counts(H, pattern, epr, R=COUNT_R):
    full = R * (epr + 1)
    if pattern == "full":
        return np.full(H, full, np.int64)
    if pattern == "last_only":
        c = np.zeros(H, np.int64)
        c[H - 1] = full
        return c
    c = (np.arange(H) * 7 + 3) % (full + 1)
    c[c == 0] = full
    if pattern == "ends_empty":
        c[0] = c[H - 1] = 0
    else:
        c[H // 2 - H // 8:H // 2 + H // 8 + 1] = 0         # (H = 129, 254: the run crosses ring 64 / 128, a wave of the count scan)
    return c


def counts(H, pattern, epr):
    """Rows with wanted_counts(...) edges each: region g of a row gets up to epr + 1 bumps, 11 items apart.  A row that wants
    none is all NaN (an empty ring) when its number is even and a smooth ring when it is odd."""
    R, n = COUNT_R, COUNT_W
    want = wanted_counts(H, pattern, epr)
    sector = (n - 10) // R
    assert 6 + 11 * epr < sector
    rows = []
    for i in range(H):
        if want[i] == 0 and i % 2 == 0:
            rows.append(None)
            continue
        r = base_ring(n)
        left = int(want[i])
        for g in range(R):
            for k in range(min(epr + 1, left)):
                _bump(r, 5 + sector * g + 6 + 11 * k, dx=0.25)
            left -= min(epr + 1, left)
        rows.append(_exact32(r))
    return Case("counts_%d_%s_%d" % (H, pattern, epr), R, epr, rows, [dict(want=want)])


def instance_for(max_width, R):
    """Items per lane of the k_ring_extract instance a handle created with this max_width launches: by the longest region of a
    ring of max_width points (the last one takes the remainder of the split)."""
    total = max(0, max_width - 10)
    return 24 if total - (total // max(1, R)) * (R - 1) > 256 else 16


# ---------------------------------------------------------------------------------------------
# several streams in one launch: one family per stream, one parameter set for all of them
# ---------------------------------------------------------------------------------------------
STREAM_R, STREAM_EPR, STREAM_H, STREAM_W = 4, 5, 128, 980


def stream_families():
    """[(name, rows)]: what the streams of one launch carry, all for R = 4, epr = 5 (every family keeps its picks with more
    picks allowed: only its designed candidates reach 0.1).  Rows of up to 970 points, at most 128 per family."""
    R = STREAM_R
    cas = [cascade(R, v).rows[0] for v in ("base", "twice", "sector5")]
    cand = [_candidates(n, seed=200 + n) for n in (970, 523, 300, 131, 64, 40, 30, 29)]
    cnt = counts(16, "middle_run", 2).rows
    fams = [("ties", ties(R).rows), ("cutoff", cutoff(R).rows), ("gaps", gaps(R).rows), ("cascade", cas),
            ("candidates", cand), ("counts", cnt)]
    fams.append(("mixed", [rows[len(rows) // 2] for _, rows in fams] + [None] + [rows[0] for _, rows in fams]))
    assert all(len(rows) <= STREAM_H and max(len(r) for r in rows if r is not None) <= STREAM_W for _, rows in fams)
    return fams


def stream_rings():
    """[(name, ring)]: single rings (ring 8 of a 16-line cloud) for the streams of one launch, R = 4, epr = 5."""
    out = []
    for name, rows in stream_families()[:5]:
        pick = range(len(rows)) if len(rows) <= 8 else (0, 5, 38, 73, 109, 110, 111, 112, 116)
        out += [("%s_%d" % (name, i), rows[i]) for i in pick if len(rows[i]) >= STREAM_R * STREAM_EPR + 10]
    return out
