"""Designed edge clouds for the correspondence search (k_knn<256>, k_knn<128>, k_knn8 + k_knn8_exact, k_line_gate) and the
local-map filter (kernels_filter.h): inputs whose stated property holds EXACTLY in float, which scene data only meets by chance.

NumPy only, seeded, no file I/O.  Every generator returns (map, queries): float32 (n, 4) clouds (x, y, z, intensity).
Coordinates are multiples of a lattice step q(origin) around an exactly representable origin: q = 1/64 m wherever a float
can hold it (|x| < 2^17 m), the float quantum itself beyond (1/16 m at 1e6 m, 1/8 m beyond 2^20 m); lattice worlds assert
float32(x) == x for every coordinate they emit, so that no world silently degenerates by rounding.
A "pole" is a vertical run of points: five neighbours on it pass the line gate (laser_odometry.cc:344).

  poles(origin)          ~60 poles, 0.125 m spacing in z, queries = map points + N(0, 5 cm)               baseline
  poles_snapped(origin)  the same, queries rounded to the lattice: exact multi-way ties of float distances, also 5th / 6th
  on_faces(origin)       poles at integer-metre xy (pairs 1 m apart), z multiples of 0.125 m, queries on the 1/32 m lattice,
                         a quarter of them exactly on a pole's axis (a cell edge), a quarter exactly midway between the two
                         poles of a pair (ties across two cells): points and queries on cell faces, edges, corners
  decoys(origin)         poles with ~0.2 m spacing plus, beside every other pole point, one point ~0.35 m off the axis; queries
                         N(0, 12 cm); map order shuffled: swapping one of NN2..NN4 for the 6th neighbour flips the line gate
  dense()                4 poles of 2000 points (2^-11 m spacing) inside 6 cells, one run of exactly 512 points inside one
                         0.4 m leaf: cell-major streaming, many rounds per cell, > 512 points per leaf
  sparse()               five-point clusters over +-200 m, queries N(0, 30 cm): neighbour-cell probing, gate near 1.0
  gate_edge()            five-point lines whose fifth point is at float sq_dist 1 - 2^-23 (two ulp below the gate), exactly 1.0,
                         and above 1.0 two cells away — with the fifth point in a face-, edge- and corner-adjacent cell, along
                         each axis, on both sides of 0
  few()                  maps of 0, 1, 4, 5 and 6 points

ORIGINS are the five of the list below; ALIAS_ORIGIN lies beyond 2^20 m, where pack_cell's 21 bits per axis wrap: the pole
worlds there get a second group of poles 2^21 m away, in the cells that alias with the first group's.

Measured with the oracle alone (tests/test_designed_clouds.py prints these rows with -s and asserts the conditions below on
them; on every row brute force = kd-tree on every query and float64 NumPy neighbours = float neighbours on every clearly
ordered query; 3000 queries per world; tied6 / tied01: exact tie of float distances among the six nearest / between NN0 and
NN1; left out: share of the queries that are not clearly ordered, which the float64 leg leaves to the oracle comparison):

  world          origin                   points  cells  valid  tied6  tied01  fifth-sensitive  left out
  poles          (0,0,0) .. (-61000,..)     2400    348  1.000  0.000-0.001  0.000-0.001        0.000-0.001
  poles          (1e6,-1e6,0)               2400    347  1.000  0.960  0.458                    0.960
  poles          alias                      4800    698  1.000  0.947  0.000                    0.947
  poles_snapped  (0,0,0) .. (-61000,..)     2400    354  1.000  0.240  0.119                    0.240
  poles_snapped  (1e6,-1e6,0)               2400    354  1.000  0.959  0.461                    0.959
  poles_snapped  alias                      4800    709  1.000  0.946  0.000                    0.946
  on_faces       (0,0,0) .. (-61000,..)     2480    310  1.000  0.618  0.424                    0.618
  on_faces       (1e6,-1e6,0)               2480    310  1.000  0.971  0.608                    0.971
  on_faces       alias                      4960    682  1.000  0.963  0.251                    0.963
  decoys         (0,0,0) .. (-61000,..)     2250  543-557  0.315-0.316  0.000-0.009  0.000-0.002  0.950-0.951  0.000-0.009
  decoys         (1e6,-1e6,0)               2250    536  0.413  0.565  0.035   0.865            0.565
  decoys         alias                      4500   1469  0.427  0.966  0.506   0.802            0.966
  dense          -                          8512      7  1.000  0.000  0.000                    0.003   (largest cell 2000 points)
  sparse         -                         15000   6608  0.771  0.000  0.000                    0.000   (4 of 3000 queries within 1e-3 of the gate)
  gate_edge      -                           270         18 of 54 queries valid: the 18 "below" cases
(poles are 1.25 m apart at the least, so a pole world's queries are always valid; at the two largest origins a float cannot tell
"snapped" from "not snapped" — the float grid snaps every query — and the 5 % cap on "left out" applies where the lattice is
1/64 m.  Twenty exact copies of a cloud give five identical neighbours and no valid query: duplicates stay with
test_knn_ties_are_ordered_by_window_index.)

Conditions (MIN_VALID, MIN_TIED, MIN_FIFTH_SENSITIVE, MAX_LEFT_OUT below): every test asserts them on the oracle's output
before it looks at the GPU's answer, so that no case passes by being empty.
"""
import numpy as np

ORIGINS = [
    (0.0, 0.0, 0.0),
    (-37.5, -12.25, -3.0),
    (4100.5, -3900.25, 130.0),
    (-61000.0, 58000.0, -400.0),
    (1e6, -1e6, 0.0),
]
# beyond +-2^20 m: pack_cell keeps 21 bits per axis, so cell 2^20 + k and cell -2^20 + k share a key
ALIAS_ORIGIN = (float(2 ** 20 + 3000), -float(2 ** 20 + 5000), 0.0)
ALIAS_SHIFT = (-float(2 ** 21), float(2 ** 21), 0.0)
ALL_ORIGINS = ORIGINS + [ALIAS_ORIGIN]


def origin_id(o):
    return "alias" if tuple(o) == ALIAS_ORIGIN else "o%g_%g_%g" % tuple(o)


def lattice_step(origin, reach=64.0):
    """The lattice step of a world around `origin`: 1/64 m, or the float quantum at its largest coordinate if that is coarser."""
    top = max(abs(c) for c in origin) + reach
    return max(1.0 / 64.0, float(np.spacing(np.float32(top))))


def _cloud(xyz, group=None):
    """float32 (n, 4) cloud; the intensity of a map point is the number of its group (pole, cluster, run): groups lie more than
    1 m apart wherever the world says so, which lets a test spread a map over several frames that cannot match each other."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3) + 0.0      # (no -0.0: the pose transform would return +0.0 for it)
    out = np.zeros((xyz.shape[0], 4), np.float32)
    out[:, :3] = xyz
    out[:, 3] = 0 if group is None else group
    return out


def _exact_cloud(xyz, group=None):
    """float32 cloud of coordinates that must already be floats: asserts float32(x) == x for every one."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz), "a lattice coordinate is not a float"
    return _cloud(xyz, group)


def groups_of(cloud):
    return cloud[:, 3].astype(np.int64)


def _snap(x, q):
    return np.round(np.asarray(x, dtype=np.float64) / q) * q


def _finish(origin, q, rel_map, rel_q, snap_queries, group):
    """Map (always on the lattice) and queries (on it if asked for, or if the float grid at this origin is the lattice anyway)."""
    o = np.asarray(origin, dtype=np.float64)
    m = _exact_cloud(o + _snap(rel_map, q), group)
    if snap_queries or q > 1.0 / 64.0:
        return m, _exact_cloud(o + _snap(rel_q, q if q > 1.0 / 64.0 else snap_queries))
    return m, _cloud(o + rel_q)


def _with_alias(origin, rel_map, rel_q, group):
    """At ALIAS_ORIGIN: a second copy of the world 2^21 m away along x and y — same low 21 bits of every cell index."""
    if tuple(origin) != ALIAS_ORIGIN:
        return rel_map, rel_q, group
    sh = np.asarray(ALIAS_SHIFT)
    # (the copy is shifted by one pole spacing in z so that it is not an exact duplicate modulo the shift)
    far_map = rel_map + sh + [0.0, 0.0, 0.125 * 3]
    far_q = rel_q[: len(rel_q) // 2] + sh + [0.0, 0.0, 0.125 * 3]
    return np.concatenate([rel_map, far_map]), np.concatenate([rel_q[len(rel_q) // 2:], far_q]), np.concatenate([group, group + group.max() + 1])


def _pole_axes(rng, n_poles, q, half=20.0, min_sep=0.0):
    """Distinct lattice positions in xy within +-half of the origin, at least min_sep apart."""
    out = []
    while len(out) < n_poles:
        c = _snap(rng.uniform(-half, half, 2), max(q, 1.0 / 64.0))
        if all(np.hypot(*(c - p)) >= max(min_sep, 1e-9) for p in out):
            out.append(c)
    return np.array(out)


POLE_SEP = 1.25          # metres between any two poles: points of different poles never pass the distance gate together


def _poles_rel(rng, n_poles, pts_per_pole, q, dz=0.125):
    axes = _pole_axes(rng, n_poles, q, min_sep=POLE_SEP)
    z0 = _snap(rng.uniform(-2.0, 0.0, n_poles), 0.125)
    pts = np.zeros((n_poles, pts_per_pole, 3))
    pts[:, :, 0] = axes[:, None, 0]
    pts[:, :, 1] = axes[:, None, 1]
    pts[:, :, 2] = z0[:, None] + dz * np.arange(pts_per_pole)[None, :]
    return pts.reshape(-1, 3)


def poles(origin=ORIGINS[0], n_queries=3000, seed=1, n_poles=60, pts_per_pole=40, snapped=False):
    rng = np.random.default_rng(seed)
    q = lattice_step(origin)
    rel_map = _poles_rel(rng, n_poles, pts_per_pole, q)
    rel_q = rel_map[rng.integers(0, len(rel_map), n_queries)] + rng.normal(0.0, 0.05, (n_queries, 3))
    rel_map, rel_q, group = _with_alias(origin, rel_map, rel_q, np.repeat(np.arange(n_poles), pts_per_pole))
    return _finish(origin, q, rel_map, rel_q, 1.0 / 64.0 if snapped else 0, group)


def poles_snapped(origin=ORIGINS[0], n_queries=3000, seed=2, **kw):
    return poles(origin, n_queries, seed, snapped=True, **kw)


def on_faces(origin=ORIGINS[0], n_queries=3000, seed=3, n_pairs=31, pts_per_pole=40):
    rng = np.random.default_rng(seed)
    q = lattice_step(origin)
    o_int = np.round(np.asarray(origin, dtype=np.float64))          # integer-metre origin: cell faces are at absolute integers
    left = set()
    while len(left) < n_pairs:
        c = tuple(int(v) for v in rng.integers(-12, 12, 2))
        if all(abs(c[0] - p[0]) > 2 or abs(c[1] - p[1]) > 1 for p in left):      # pairs do not touch: poles 1 m apart at the least
            left.add(c)
    left = np.array(sorted(left), dtype=np.float64)
    if tuple(origin) == ORIGINS[0]:
        assert (left < 0).any() and (left >= 0).any()               # both sides of 0
    axes = np.concatenate([left, left + [1.0, 0.0]])
    z0 = np.tile(rng.integers(-3, 0, n_pairs).astype(np.float64), 2)
    pts = np.zeros((len(axes), pts_per_pole, 3))
    pts[:, :, 0] = axes[:, None, 0]
    pts[:, :, 1] = axes[:, None, 1]
    pts[:, :, 2] = z0[:, None] + 0.125 * np.arange(pts_per_pole)[None, :]
    rel_map = pts.reshape(-1, 3)
    pick = rel_map[rng.integers(0, len(rel_map), n_queries)]
    rel_q = pick + rng.normal(0.0, 0.05, (n_queries, 3))
    kind = rng.integers(0, 4, n_queries)
    rel_q[kind == 0, :2] = pick[kind == 0, :2]                      # exactly on the pole's axis: a vertical cell edge
    mid = kind == 1                                                 # exactly midway between the poles of the pair
    pair_left = rel_map[rng.integers(0, len(left) * pts_per_pole, n_queries)]
    rel_q[mid, 0] = pair_left[mid, 0] + 0.5
    rel_q[mid, 1] = pair_left[mid, 1] + rng.normal(0.0, 0.05, int(mid.sum()))
    rel_q[mid, 2] = pair_left[mid, 2] + rng.normal(0.0, 0.05, int(mid.sum()))
    rel_map, rel_q, group = _with_alias(origin, rel_map, rel_q, np.repeat(np.arange(len(axes)), pts_per_pole))
    return _finish(o_int, q, rel_map, rel_q, 1.0 / 32.0, group)


def decoys(origin=ORIGINS[0], n_queries=3000, seed=4, n_poles=50, pts_per_pole=30):
    rng = np.random.default_rng(seed)
    q = lattice_step(origin)
    dz = max(round(0.2 / q), 1) * q
    off = max(round(0.35 / q), 1) * q if q < 0.125 else 0.5         # (0.25 m spacing on the 1/8 m grid: the decoy keeps its rank)
    axes = _pole_axes(rng, n_poles, q, min_sep=3.0)
    z0 = _snap(rng.uniform(-2.0, 0.0, n_poles), 0.125)
    pts = np.zeros((n_poles, pts_per_pole, 3))
    pts[:, :, 0] = axes[:, None, 0]
    pts[:, :, 1] = axes[:, None, 1]
    pts[:, :, 2] = z0[:, None] + dz * np.arange(pts_per_pole)[None, :]
    side = pts[:, ::2, :].copy()
    ang = rng.integers(0, 4, side.shape[:2])                        # the decoy sits off the axis along +-x or +-y
    side[:, :, 0] += off * np.array([1, -1, 0, 0])[ang]
    side[:, :, 1] += off * np.array([0, 0, 1, -1])[ang]
    on_axis = pts.reshape(-1, 3)
    # (N(0, 12 cm); on the coarse float grids wide enough that the queries do not all round onto the axis)
    rel_q = on_axis[rng.integers(0, len(on_axis), n_queries)] + rng.normal(0.0, max(0.12, 1.5 * q), (n_queries, 3))
    rel_map = np.concatenate([on_axis, side.reshape(-1, 3)])
    group = np.concatenate([np.repeat(np.arange(n_poles), pts_per_pole), np.repeat(np.arange(n_poles), side.shape[1])])
    perm = rng.permutation(len(rel_map))
    rel_map, rel_q, group = _with_alias(origin, rel_map[perm], rel_q, group[perm])
    return _finish(origin, q, rel_map, rel_q, 0, group)


DENSE_STEP = 2.0 ** -11


def dense(n_queries=3000, seed=5, pts_per_pole=2000):
    """Four poles of pts_per_pole points 2^-11 m apart (with 2000: one pole fills one 1 m cell, two straddle a cell face, one
    lies at negative indices: 6 cells, the largest 2000 points, 819 or 820 points per 0.4 m leaf) and a run of exactly 512
    points inside one leaf."""
    rng = np.random.default_rng(seed)
    starts = [(0.25, 0.25, 0.0), (2.5, 0.25, 0.5), (0.25, 2.5, -0.5), (-1.75, -1.75, -1.0)]
    runs = []
    for x, y, z in starts:
        p = np.zeros((pts_per_pole, 3))
        p[:, 0], p[:, 1] = x, y
        p[:, 2] = z + DENSE_STEP * np.arange(pts_per_pole)
        runs.append(p)
    p = np.zeros((512, 3))                                           # leaf [4.4, 4.8) x [0.4, 0.8) x [0.4, 0.8)
    p[:, 0], p[:, 1] = 4.5, 0.5
    p[:, 2] = 0.4375 + DENSE_STEP * np.arange(512)
    runs.append(p)
    rel_map = np.concatenate(runs)
    rel_q = rel_map[rng.integers(0, len(rel_map), n_queries)] + rng.normal(0.0, 0.005, (n_queries, 3))
    group = np.concatenate([np.full(len(r), i) for i, r in enumerate(runs)])
    return _exact_cloud(rel_map, group), _cloud(rel_q)


def sparse(n_queries=3000, seed=6, n_clusters=3000, half=200.0):
    """Five-point clusters: short lines of 3/16 m steps along an axis or a diagonal, so that most clusters straddle a cell face.
    One cluster per square of a grid over +-half, far enough from the square's border that clusters stay more than 1 m apart."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n_clusters)))
    cell = 2.0 * half / side
    room = cell / 2.0 - 1.2            # a cluster reaches 0.65 m from its centre
    assert room >= 0.0
    sq = rng.permutation(side * side)[:n_clusters]
    c = np.zeros((n_clusters, 3))
    c[:, 0] = -half + (sq % side + 0.5) * cell + rng.uniform(-room, room, n_clusters)
    c[:, 1] = -half + (sq // side + 0.5) * cell + rng.uniform(-room, room, n_clusters)
    c[:, 2] = rng.uniform(-10.0, 10.0, n_clusters)
    c = _snap(c, 1.0 / 64.0)
    dirs = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, -1, 1], [1, 1, 1]], dtype=np.float64) * 0.1875
    step = dirs[rng.integers(0, len(dirs), n_clusters)]
    pts = c[:, None, :] + step[:, None, :] * (np.arange(5) - 2.0)[None, :, None]
    rel_map = pts.reshape(-1, 3)
    rel_q = c[rng.integers(0, n_clusters, n_queries)] + rng.normal(0.0, 0.3, (n_queries, 3))
    return _exact_cloud(rel_map, np.repeat(np.arange(n_clusters), 5)), _cloud(rel_q)


GATE_KINDS = ("face", "edge", "corner")
GATE_CASES = ("below", "exact", "above")


def gate_edge():
    """54 groups of five points and one query each.  Along the group's primary axis a the four near points sit within 1/16 m
    of the query and the fifth at a float offset of 1 - 2^-24 ("below": sq_dist[4] = 1 - 2^-23 < 1.0), 1.0 ("exact": not
    below the gate) or 1 + 2^-9 with the fifth point two cells away ("above").  kind "edge" moves query and fifth point to
    the two sides of a cell face of the second axis, 2^-13 m apart (the float sum stays the same), "corner" of the third as
    well.  Every group along each of the three axes, mirrored to negative coordinates, 8 m from the next along its second
    axis.  Returns (map, queries, labels): labels[i] = (kind, case) of query i; the map points of group i are rows 5i..5i+4."""
    eps_pair = (1.0 - 2.0 ** -14, 1.0 + 2.0 ** -14)                  # both floats, 2^-13 apart, on the two sides of 1.0
    m, qs, labels = [], [], []
    g = 0
    for kind in GATE_KINDS:
        for case in GATE_CASES:
            for roll in range(3):
                for sign in (1.0, -1.0):
                    g += 1
                    if case == "below":
                        qa, fifth = 0.125 + 2.0 ** -24, 1.125
                        near = [0.125 - 1 / 16, 0.125 - 1 / 32, 0.125 + 1 / 32, 0.125 + 1 / 16]
                    elif case == "exact":
                        qa, fifth = 0.125, 1.125
                        near = [0.125 - 1 / 16, 0.125 - 1 / 32, 0.125 + 1 / 32, 0.125 + 1 / 16]
                    else:
                        qa, fifth = 1.0 - 2.0 ** -10, 2.0 + 2.0 ** -10
                        near = [qa - 1 / 8, qa - 3 / 32, qa - 1 / 16, qa - 1 / 32]
                    qb, fb = (eps_pair if kind in ("edge", "corner") else (0.5, 0.5))
                    qc, fc = (eps_pair if kind == "corner" else (0.5, 0.5))
                    shift = 8.0 * g
                    grp = [[a, qb + shift, qc] for a in near] + [[fifth, fb + shift, fc]]
                    pts = sign * np.roll(np.array(grp + [[qa, qb + shift, qc]]), roll, axis=1)
                    m.append(pts[:5])
                    qs.append(pts[5])
                    labels.append((kind, case))
    return _exact_cloud(np.concatenate(m), np.repeat(np.arange(len(m)), 5)), _exact_cloud(np.array(qs)), labels


def few(n_queries=64, seed=8):
    """[(map, queries)] for maps of 0, 1, 4, 5 and 6 points of one pole; the queries surround it."""
    rng = np.random.default_rng(seed)
    pole = np.zeros((6, 3))
    pole[:, 0], pole[:, 1] = 1.5, -0.5
    pole[:, 2] = 0.125 * np.arange(6)
    rel_q = pole[rng.integers(0, 6, n_queries)] + rng.normal(0.0, 0.05, (n_queries, 3))
    return [(_exact_cloud(pole[:n]), _cloud(rel_q)) for n in (0, 1, 4, 5, 6)]


def sequence_frames(origin, n_frames, seed=9, n_poles=120, pts_per_pole=12, keep=0.6, extra=4, jitter=0.01):
    """Frames of one static world for a run with the true pose at identity: each frame an independent sample (a random `keep`
    of the poles, `jitter` metres of noise on every point) plus `extra` poles that exist in that frame only, so that every
    append creates cells and every eviction empties some.  pts_per_pole = 12 at 0.125 m: n_poles * keep * 12 + extra * 12 edges."""
    rng = np.random.default_rng(seed)
    q = lattice_step(origin)
    o = np.asarray(origin, dtype=np.float64)
    world = _poles_rel(rng, n_poles, pts_per_pole, q).reshape(n_poles, pts_per_pole, 3)
    frames = []
    for _ in range(n_frames):
        sel = rng.permutation(n_poles)[: int(round(keep * n_poles))]
        own = _poles_rel(rng, extra, pts_per_pole, q).reshape(extra, pts_per_pole, 3) + np.array([30.0, 0.0, 0.0]) * rng.choice([-1.0, 1.0])
        pts = np.concatenate([world[sel].reshape(-1, 3), own.reshape(-1, 3)])
        frames.append(_cloud(o + pts + rng.normal(0.0, jitter, pts.shape)))
    return frames


def leaf_aligned(seed=10, leaf=0.4, n_poles=40, pts_per_pole=24):
    """on_faces rescaled to the 0.4 m leaf of the local-map filter: every coordinate is float32(k * 0.4f) for an integer k on
    both sides of 0 — the values floorf(x * (1 / 0.4f)) is decided at.  Poles 0.4 m apart in z, several points per leaf come from
    a second copy of each pole one float above."""
    rng = np.random.default_rng(seed)
    lf = np.float32(leaf)
    k_xy = rng.integers(-20, 20, (n_poles, 2))
    k_z = rng.integers(-6, 0, n_poles)[:, None] + np.arange(pts_per_pole)[None, :]
    k = np.zeros((n_poles, pts_per_pole, 3), np.int64)
    k[:, :, 0], k[:, :, 1], k[:, :, 2] = k_xy[:, None, 0], k_xy[:, None, 1], k_z
    base = (k.reshape(-1, 3).astype(np.float32) * lf).astype(np.float32)
    up = np.nextafter(base, np.float32(np.inf))
    out = np.zeros((2 * len(base), 4), np.float32)
    out[:, :3] = np.concatenate([base, up])
    out[:, 3] = np.arange(len(out)) % 97
    return out[rng.permutation(len(out))]


# ---------------------------------------------------------------------------------------------
# float64 reference and the statistics the tests condition on
# ---------------------------------------------------------------------------------------------
def neighbours_f64(map_xyz, q_xyz, k=6, chunk=None):
    """Plain brute force in float64: indices (ascending distance, then index) and squared distances of the k nearest map points.
    Candidates (k + 10 per query) are picked by |q|^2 + |m|^2 - 2 q.m on coordinates moved by an integer offset (exact for float
    inputs), their distances then computed as sums of squared differences.  (Index order among more than ten points within
    1e-11 m^2 of the k-th distance is not resolved; such queries are not clearly ordered.)"""
    m = np.asarray(map_xyz, dtype=np.float64)[:, :3]
    qq = np.asarray(q_xyz, dtype=np.float64)[:, :3]
    k = min(k, len(m))
    idx = np.zeros((len(qq), k), np.int64)
    dd = np.zeros((len(qq), k))
    if k == 0 or len(qq) == 0:
        return idx, dd
    c = np.round(m.mean(axis=0))
    ml, ql = m - c, qq - c
    m2 = (ml * ml).sum(axis=1)
    kk = min(k + 10, len(m))
    chunk = chunk or max(1, int(2e7 // max(len(m), 1)))
    for a in range(0, len(qq), chunk):
        qa = ql[a:a + chunk]
        approx = (qa * qa).sum(axis=1)[:, None] + m2[None, :] - 2.0 * (qa @ ml.T)
        cand = np.argpartition(approx, kk - 1, axis=1)[:, :kk] if kk < len(m) else np.tile(np.arange(len(m)), (len(qa), 1))
        diff = qa[:, None, :] - ml[cand]
        dc_ = (diff * diff).sum(axis=2)
        o = np.lexsort((cand, dc_), axis=1)[:, :k]
        idx[a:a + chunk] = np.take_along_axis(cand, o, axis=1)
        dd[a:a + chunk] = np.take_along_axis(dc_, o, axis=1)
    return idx, dd


def clearly_ordered(d6, rel=1e-5):
    """Queries whose six smallest float64 squared distances pairwise differ by more than `rel` relative (a hundred times the
    float rounding of a three-term sum).  Fewer than six map points: all that there are."""
    if d6.shape[1] < 2:
        return np.ones(len(d6), bool)
    gap = np.diff(d6, axis=1)
    return (gap > rel * d6[:, 1:]).all(axis=1)


def tie_shares(map_c, q_c):
    """Share of the queries with an exact tie of FLOAT distances (sqdist_f: float differences, x -> y -> z float sum) among the
    six nearest, and between NN0 and NN1."""
    m, qq = map_c[:, :3].astype(np.float32), q_c[:, :3].astype(np.float32)
    idx, _ = neighbours_f64(m, qq, k=8)
    t6 = t01 = 0
    for r in range(len(qq)):
        c = m[idx[r]]
        dx, dy, dz = (qq[r, 0] - c[:, 0]), (qq[r, 1] - c[:, 1]), (qq[r, 2] - c[:, 2])
        d = np.sort(((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32) + (dz * dz).astype(np.float32))[:6]
        t6 += bool((np.diff(d) == 0).any())
        t01 += bool(len(d) > 1 and d[0] == d[1])
    return t6 / max(len(qq), 1), t01 / max(len(qq), 1)


def line_gate(pts5):
    """The reference's line gate (laser_odometry.cc:327-344) in NumPy float64: largest eigenvalue of the five points' scatter
    matrix above three times the second."""
    z = pts5 - pts5.mean(axis=0)
    ev = np.linalg.eigvalsh(z.T @ z)
    return bool(ev[2] > 3.0 * ev[1])


def fifth_sensitive_share(map_c, q_c):
    """Among the queries that pass the distance gate: the share for which replacing one of NN2..NN4 by the sixth neighbour
    changes the line-gate decision."""
    m = map_c[:, :3].astype(np.float64)
    idx, d = neighbours_f64(m, q_c, k=6)
    n = hit = 0
    for r in range(len(idx)):
        if idx.shape[1] < 6 or not d[r, 4] < 1.0:
            continue
        n += 1
        base = line_gate(m[idx[r, :5]])
        for j in (2, 3, 4):
            sel = list(idx[r, :5])
            sel[j] = idx[r, 5]
            if line_gate(m[sel]) != base:
                hit += 1
                break
    return hit / max(n, 1)


WORLDS = {"poles": poles, "poles_snapped": poles_snapped, "on_faces": on_faces, "decoys": decoys}
TIE_WORLDS = ("poles_snapped", "on_faces")
# conditions each test asserts on the oracle's output before it looks at the GPU
MIN_VALID = {"poles": 0.8, "poles_snapped": 0.8, "on_faces": 0.8, "dense": 0.8, "decoys": 0.25, "sparse": 0.5}
MIN_TIED = {"poles_snapped": 0.15, "on_faces": 0.3}
MIN_FIFTH_SENSITIVE = 0.6
MAX_LEFT_OUT = 0.05          # by the float64 leg, on poles / decoys / dense / sparse


def world(name, origin=None, n_queries=3000, **kw):
    if name in WORLDS:
        return WORLDS[name](origin, n_queries, **kw)
    return {"dense": dense, "sparse": sparse}[name](n_queries, **kw)
