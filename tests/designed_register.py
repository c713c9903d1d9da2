"""Designed inputs for liodom_map_register_poses: the smallest maps and edge clouds at which its search, its grid and its edge
loop can go wrong.  NumPy only, seeded, no file I/O; everything is computed once and never modified.

The map is la.Map / orc.Map with MAP_SIZES (10 m cells, 0.05 m leaves), filled by ONE update of hand-placed points at the identity:
points at least 0.1 m apart lie in different leaves, so every point enters the map as it is (tests/test_designed_register.py
asserts it on the oracle's map).  getLocalMap visits the centre cell twice (square, then column), so its points appear twice in a
local map: a correspondence there has NN0 == NN1 and its block is non-finite.  Every structure below stays out of the centre cell
of the start pose (x, y, z in [0, 10)), and inside the z layer [0, 10) the square of cells covers.

world()    segments of 9 points at 0.1 m spacing (designed_solves' world, denser): centres on a 3 m lattice, x, y in -15 .. 12,
           z in 1 .. 8.5, random directions; one edge per segment, 0.03 m along it plus 0.02 m of noise, seen from MOTION.
           The first N edges are the case "n_edges = N"; the registration starts at the identity and has to find MOTION.
knn()      the first 64 segments (a well-posed solve) plus structures of a few points each, every one more than 3 m from anything
           else, and one edge per structure that IS the query at the identity start (the identity maps an edge to itself bit for
           bit).  With max_passes = 1 the returned correspondences are those of the designed queries:
             five_at_1        4 points + a fifth at float squared distance exactly 1.0f          -> invalid (not < 1.0f)
             five_below_1     the same, the fifth one float closer (1 - 2^-23)                     -> valid
             ties             +-0.25, +-0.5, +-0.75 along x: NN0 / NN1 and the fifth place are ties -> the lower indices
             face_voxel       query 5e-4 inside a 1 m voxel face, all five neighbours beyond it     -> valid
             face_cell        the same at x = -10: a face of the map's coarse cells too             -> valid
             negative         x and y negative, the neighbours across the voxel faces at -13 and -8  -> valid
             crowd            a 1 m voxel holding 40 points, the query inside
             nan              an edge with a NaN coordinate                                         -> invalid
small(n)   a map of n = 4 or 5 collinear points that straddles two 1 m voxels whose keys collide in the table of that size
           (map_register_table_size: 8 slots for 4 points, 16 for 5), ten edges beside it.
"""
import numpy as np

MAP_SIZES = dict(xy=10.0, z=10.0, res=0.05)
MAP_CAPS = dict(max_cells=256, cell_capacity=4096, max_modified_cells=64)
MOTION_W = np.array([0.004, -0.003, 0.006])      # rotation vector of the pose the edges were taken from
MOTION_T = np.array([0.08, -0.05, 0.04])
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
SEG_PTS, SPACING = 9, 0.1
_M64 = (1 << 64) - 1
_CACHE = {}


def map_hash(k, mask):
    """map_hash of liodom_map.h."""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    k ^= k >> 33
    return (k & 0xffffffff) & mask


def voxel_key(v):
    B = 1 << 20
    return ((int(v[0]) + B) << 42) | ((int(v[1]) + B) << 21) | (int(v[2]) + B)


def table_size(n):
    t = 8
    while t < 2 * n:
        t <<= 1
    return t


def rot(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _xyzi(p):
    out = np.zeros((len(p), 4), np.float32)
    out[:, :3] = np.asarray(p, np.float64).reshape(-1, 3).astype(np.float32)
    return out


def world():
    """dict(map [9 S, 4], edges [S, 4], truth [7]): S >= 257 segments, one edge each."""
    if "world" in _CACHE:
        return _CACHE["world"]
    rng = np.random.default_rng(20260)
    xs = np.arange(-15.0, 12.5, 3.0)
    zs = np.array([1.0, 3.5, 6.0, 8.5])
    sites = np.stack(np.meshgrid(xs, xs, zs, indexing="ij"), axis=-1).reshape(-1, 3)
    centre_cell = (sites[:, 0] > -1.0) & (sites[:, 0] < 11.0) & (sites[:, 1] > -1.0) & (sites[:, 1] < 11.0)
    sites = sites[~centre_cell & (np.hypot(sites[:, 0], sites[:, 1]) >= 4.0)]
    sites = sites[rng.permutation(len(sites))]
    assert len(sites) >= max(COUNTS)
    R, pts, edges = rot(MOTION_W), [], []
    for c in sites:
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        seg = np.float32(c[None, :] + (np.arange(SEG_PTS)[:, None] - SEG_PTS // 2) * SPACING * d[None, :])
        pts.append(seg)
        d32 = (seg[-1].astype(np.float64) - seg[0].astype(np.float64))
        d32 /= np.linalg.norm(d32)
        on = seg[SEG_PTS // 2].astype(np.float64) + 0.03 * d32 + rng.normal(scale=0.02, size=3)
        edges.append(R.T @ (on - MOTION_T))
    w = dict(map=_xyzi(np.concatenate(pts)), edges=_xyzi(np.array(edges)), n_segments=len(sites))
    _CACHE["world"] = w
    return w


def _line(q, offsets):
    """Points q + (o, 0, 0) for the float offsets o: exact when q's and the sums' bits allow (asserted by the tests)."""
    q = np.float32(q)
    return np.array([[np.float32(q[0] + np.float32(o)), q[1], q[2]] for o in offsets], np.float32)


def knn():
    """dict(map, edges, special: name -> edge index, expect: name -> True / False / None (valid, invalid, whatever the model says))."""
    if "knn" in _CACHE:
        return _CACHE["knn"]
    w = world()
    pts, edges, special, expect = [w["map"][:64 * SEG_PTS, :3]], [w["edges"][:64, :3]], {}, {}

    def add(name, query, points, valid):
        special[name] = sum(len(e) for e in edges)
        expect[name] = valid
        edges.append(np.float32(query).reshape(1, 3))
        pts.append(np.float32(points).reshape(-1, 3))

    below = np.float32(1.0) - np.float32(2.0 ** -24)
    # the fifth neighbour: q.x - p.x = 1.0f exactly, and one float less (both differences are exact in float)
    add("five_at_1", (0.5, -4.5, 2.0), _line((0.5, -4.5, 2.0), [0.125, 0.25, 0.375, 0.46875, -1.0]), False)
    add("five_below_1", (0.5, -7.5, 2.0), _line((0.5, -7.5, 2.0), [0.125, 0.25, 0.375, 0.46875, -below]), True)
    add("ties", (-5.0, -4.5, 7.25), _line((-5.0, -4.5, 7.25), [0.75, -0.75, 0.5, -0.5, 0.25, -0.25]), True)
    add("face_voxel", (-5.5, 4.0005, 7.25), np.float32([[-5.5 + 0.1 * k, 3.95 - 0.01 * k, 7.25] for k in range(-2, 3)]), True)
    add("face_cell", (-9.9995, -13.5, 7.25), np.float32([[-10.05 - 0.1 * k, -13.5, 7.25] for k in range(5)]), True)
    add("negative", (-12.95, -7.95, 7.25), np.float32([[-13.02 - 0.07 * k, -8.02 - 0.07 * k, 7.25] for k in range(5)]), True)
    crowd = np.float32([[-7.9 + 0.2 * i, 13.1 + 0.2 * j, 7.1 + 0.2 * k] for i in range(5) for j in range(4) for k in range(2)])
    add("crowd", (-7.45, 13.45, 7.25), crowd, None)
    add("nan", (np.nan, -4.5, 4.75), np.zeros((0, 3), np.float32), False)
    out = dict(map=_xyzi(np.concatenate(pts)), edges=_xyzi(np.concatenate(edges)), special=special, expect=expect)
    _CACHE["knn"] = out
    return out


def small(n):
    """dict(map [n, 4], edges [10, 4], voxels): n collinear points along x, 0.1 m apart, the first two before a 1 m voxel face, the rest beyond it;
    the two voxels' keys share a slot of the n-point table."""
    key = ("small", n)
    if key in _CACHE:
        return _CACHE[key]
    mask = table_size(n) - 1
    found = None
    for vy in range(-9, -1):
        for vx in range(-9, -1):
            a, b = (vx - 1, vy, 2), (vx, vy, 2)
            if map_hash(voxel_key(a), mask) == map_hash(voxel_key(b), mask):
                found = (a, b)
                break
        if found:
            break
    assert found, "no colliding pair of voxels"
    a, b = found
    x0, y0, z0 = float(b[0]), b[1] + 0.5, b[2] + 0.5
    pts = np.float32([[x0 - 0.15 + 0.1 * k, y0, z0] for k in range(n)])
    assert len(set(np.floor(pts[:, 0]))) == 2
    rng = np.random.default_rng(7 + n)
    edges = np.float32([[x0 - 0.1 + 0.04 * k, y0, z0] for k in range(10)]) + np.float32(rng.normal(scale=0.02, size=(10, 3)))
    out = dict(map=_xyzi(pts), edges=_xyzi(edges), voxels=found)
    _CACHE[key] = out
    return out


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
FAR = np.array([0.0, 0.0, 0.0, 1.0, 1000.0, 1000.0, 0.0])      # no cell of the map within its visit: NO_MAP
