"""Designed inputs for the device map's update (k_map_assign ... k_map_commit of liodom_amd/csrc/liodom_map.h) and a NumPy
restatement of one update.  Plain Python: no library, no GPU.

The restatement (class Restated) is written from the statement in the header of liodom_map.h, not from the kernels:
  transform   world = T * p with every coordinate in FP64, left to right, cast to float32; intensity copied
  cell key    int(floor(x * (1 / size)) * size + size / 2) in FP64 per axis, sizes (xy, xy, z); cells are numbered in the order
              of the first point that touched them
  leaf        floor(float32(p) * (float32(1) / float32(res))) per axis, in float32
  cell cloud  [previous centroids, new points in input order] -> one centroid per occupied leaf in ascending (z, y, x) leaf order;
              a centroid is 0 + m_0 + m_1 + ... over the leaf's members in cloud order, in float32, divided by float32(count)
Restated.update also counts what the update asks of the device's scratch: `cursor` (items in leaves with more than one member)
and `n_multi` (such leaves), cells modified and created, leaves and members at their largest.

Every generator returns a world: dict(name, sizes = (xy, z, res), caps = the smallest liodom_map_config_t capacities that hold
the world, updates = [(points [n, 4] float32, T [3, 4] float64)], ...) plus what its tests need to find their way around.
tests/test_designed_maps.py asserts on the oracle and the restatement that every world reaches what it was designed to reach."""
import numpy as np

F = np.float32
SIZES = (10.0, 10.0, 0.5)          # 25^3 leaf bits per cell with the margins: 256 modified cells cost a few MB
KEY_LIMIT = 1 << 20
IDENTITY = np.eye(4)[:3].copy()


def pose(yaw, t):
    T = np.eye(4)[:3].copy()
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:, 3] = t
    return T


def cloud(xyz, intensity=None, seed=0):
    p = np.zeros((len(xyz), 4), F)
    p[:, :3] = np.asarray(xyz).reshape(-1, 3)
    p[:, 3] = np.random.default_rng(seed).uniform(0.0, 100.0, len(p)) if intensity is None else intensity
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def transform(points, T):
    p = np.asarray(points, F).reshape(-1, 4)
    T = np.asarray(T, np.float64).reshape(3, 4)
    x, y, z = (p[:, a].astype(np.float64) for a in range(3))
    out = p.copy()
    for r in range(3):
        out[:, r] = (T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3]).astype(F)
    return out


def cell_keys(p32, sizes):
    xy, z, _ = sizes
    keys = np.zeros((len(p32), 3), np.int64)
    for a, size in enumerate((xy, xy, z)):
        size = float(size)
        keys[:, a] = np.trunc(np.floor(p32[:, a].astype(np.float64) * (1.0 / size)) * size + size / 2.0).astype(np.int64)
    return keys


def leaf_coords(p32, res):
    inv = F(1.0) / F(res)
    return np.floor(np.asarray(p32, F)[:, :3] * inv).astype(np.int64)


def leaf_centroid(members):
    """0 + m_0 + m_1 + ... in float32, one addition after the other, then / float32(count)."""
    m = np.asarray(members, F).reshape(-1, 4)
    s = np.add.accumulate(np.concatenate([np.zeros((1, 4), F), m]), axis=0, dtype=F)[-1]
    return (s / F(len(m))).astype(F)


def in_key_range(keys):
    return ((keys >= -KEY_LIMIT) & (keys < KEY_LIMIT)).all(axis=1)


class Restated:
    def __init__(self, xy=40.0, z=50.0, res=0.4):
        self.sizes = (float(xy), float(z), float(res))
        self.ids = {}
        self.keys = []          # per cell, creation order
        self.clouds = []        # per cell [n, 4] float32
        self.last = None        # counts and member lists of the last update

    def update(self, points, T=None):
        p = transform(points, IDENTITY if T is None else T)
        new = {}                # cell -> input indices, in input order
        created = []
        for i, k in enumerate(map(tuple, cell_keys(p, self.sizes))):
            c = self.ids.get(k)
            if c is None:
                c = self.ids[k] = len(self.keys)
                self.keys.append(k)
                self.clouds.append(np.zeros((0, 4), F))
                created.append(c)
            new.setdefault(c, []).append(i)
        leaves = []
        for c in sorted(new):
            full = np.concatenate([self.clouds[c], p[new[c]]])
            lf = leaf_coords(full, self.sizes[2])
            order = np.lexsort((lf[:, 0], lf[:, 1], lf[:, 2]))          # stable: cloud order inside a leaf
            lf = lf[order]
            starts = np.concatenate([[0], 1 + np.nonzero((np.diff(lf, axis=0) != 0).any(axis=1))[0], [len(order)]])
            out = np.zeros((len(starts) - 1, 4), F)
            for j in range(len(starts) - 1):
                members = full[order[starts[j]:starts[j + 1]]]
                out[j] = leaf_centroid(members)
                leaves.append(dict(cell=c, pos=j, leaf=tuple(lf[starts[j]]), members=members, n_old=len(self.clouds[c])))
            self.clouds[c] = out
        counts = np.array([len(lv["members"]) for lv in leaves], np.int64)
        self.last = dict(leaves=leaves, modified=sorted(new), created=created, n_points=len(p),
                         cursor=int(counts[counts > 1].sum()), n_multi=int((counts > 1).sum()),
                         max_members=int(counts.max()) if len(counts) else 0,
                         max_leaves=max((len(self.clouds[c]) for c in new), default=0))
        return self.last

    def num_cells(self):
        return len(self.keys)

    def all(self):
        return np.concatenate(self.clouds) if self.clouds else np.zeros((0, 4), F)


def reached(world, updates=None):
    """What the restatement counts over the world's updates: the capacities the world needs and the largest scratch demand."""
    r = Restated(*world["sizes"])
    got = dict(max_cells=0, cell_capacity=0, max_update_points=0, max_modified_cells=0, cursor=0, n_multi=0, max_members=0, created=0)
    for pts, T in (world["updates"] if updates is None else updates):
        st = r.update(pts, T)
        got["max_cells"] = r.num_cells()
        got["cell_capacity"] = max(got["cell_capacity"], st["max_leaves"])
        got["max_update_points"] = max(got["max_update_points"], st["n_points"])
        got["max_modified_cells"] = max(got["max_modified_cells"], len(st["modified"]))
        got["created"] = max(got["created"], len(st["created"]))
        for k in ("cursor", "n_multi", "max_members"):
            got[k] = max(got[k], st[k])
    return got


def _caps(got):
    return {k: max(1, got[k]) for k in ("max_cells", "cell_capacity", "max_update_points", "max_modified_cells")}


# ---------------------------------------------------------------------------------------------
# crowded: leaves with many members, across the rounds of the centroid kernel's member scan (32 lanes)
# ---------------------------------------------------------------------------------------------
CROWDED_COUNTS = (2, 31, 32, 33, 64, 65, 257, 1000)
CROWDED_ORIGINS = ((0.0, 0.0, 0.0), (1000.0, 1000.0, 0.0))
CROWDED_FULL = 4096


def _leaf_points(rng, corner, res, n):
    """n points inside the leaf whose lower corner is `corner`, a tenth of a leaf away from its faces."""
    return np.asarray(corner) + rng.uniform(0.1 * res, 0.9 * res, (n, 3))


def crowded(origin=CROWDED_ORIGINS[0], seed=21):
    """Two adjacent cells (x in [0, 10) and [10, 20) from `origin`), leaf j of CROWDED_COUNTS in cell j % 2.  Update 0 gives the
    leaves their member counts; update 1 puts max_update_points = 4096 points into the first leaf (behind its centroid: 4097
    members); updates 2-4 come back to every leaf with one point fewer, so that an old centroid heads each sum and the member
    counts are those of CROWDED_COUNTS again.  Input order: a fixed permutation, which interleaves leaves and cells."""
    xy, z, res = SIZES
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, np.float64)
    corners = [o + [(j % 2) * xy + res * (3 + 2 * (j // 2)), res * (5 + 3 * (j // 2)), res * (7 + j)] for j in range(len(CROWDED_COUNTS))]

    def one(counts):
        pts = np.concatenate([_leaf_points(rng, c, res, n) for c, n in zip(corners, counts) if n > 0])
        return cloud(pts[rng.permutation(len(pts))], rng.uniform(0.0, 100.0, len(pts)))

    updates = [(one(CROWDED_COUNTS), IDENTITY)]
    updates.append((cloud(_leaf_points(rng, corners[0], res, CROWDED_FULL), rng.uniform(0.0, 100.0, CROWDED_FULL)), IDENTITY))
    for _ in range(3):
        updates.append((one([n - 1 for n in CROWDED_COUNTS]), IDENTITY))
    return dict(name="crowded", sizes=SIZES, updates=updates, origin=tuple(origin),
                caps=dict(max_cells=2, cell_capacity=len(CROWDED_COUNTS) // 2, max_update_points=CROWDED_FULL, max_modified_cells=2))


# ---------------------------------------------------------------------------------------------
# faces: points on leaf and cell faces and on the float32 values beside them
# ---------------------------------------------------------------------------------------------
FACES_SIZES = ((10.0, 10.0, 0.5), (25.0, 30.0, 0.3), (40.0, 50.0, 0.4))


def _beside(v):
    v = F(v)
    return np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))


def faces(sizes=FACES_SIZES[0]):
    """For every axis: the faces k * res (k = -3 .. 3 and the last leaf below the first cell's upper corner) and k * size
    (k = -2 .. 2), each with its float32 neighbour below and above; +0.0, -0.0 and the negative denormal -1.4e-45; the other two
    coordinates well inside a leaf of cell (0, 0, 0) or of cell (-1, -1, -1).  Then the same values on all three axes at once
    (edges and corners), among them the lowest and the highest leaf of cell (0, 0, 0): the two ends of its leaf bitmap.
    Update 1 feeds update 0 again, reversed: every leaf then sums its own centroid and the points that made it."""
    xy, z, res = sizes
    face_list = []          # (axis, value below, on, above) — what the CPU test looks for
    pts = []
    for a, size in enumerate((xy, xy, z)):
        n_leaves = int(round(size / res))
        vals = [k * res for k in range(-3, 4)] + [(n_leaves - 1) * res] + [k * size for k in range(-2, 3)]
        for v in vals:
            tri = _beside(v)
            face_list.append((a,) + tuple(float(t) for t in tri))
            for side, inside in enumerate((0.37, -0.37)):
                for t in tri:
                    p = [inside * xy + 0.05 * res, inside * xy + 0.05 * res, inside * z + 0.05 * res]
                    p[a] = t
                    pts.append(p)
        for special in (F(0.0), F(-0.0), F(-1.4e-45)):
            p = [0.37 * xy, 0.37 * xy, 0.37 * z]
            p[a] = special
            pts.append(p)
    for k in (-2, -1, 0, 1, 2):
        for i in range(3):
            pts.append([_beside(k * xy)[i], _beside(k * xy)[(i + 1) % 3], _beside(k * z)[(i + 2) % 3]])
            pts.append([_beside(k * res)[i], _beside(k * res)[(i + 1) % 3], _beside(k * res)[(i + 2) % 3]])
    ends = [[_beside(0.0)[2]] * 3, [_beside(xy)[0], _beside(xy)[0], _beside(z)[0]]]
    pts += ends
    p0 = cloud(np.array(pts, np.float64).astype(F), seed=31)
    p0 = p0[np.random.default_rng(32).permutation(len(p0))]
    p1 = p0[::-1].copy()
    p1[:, 3] = np.random.default_rng(33).uniform(0.0, 100.0, len(p1))
    w = dict(name="faces", sizes=tuple(sizes), updates=[(p0, IDENTITY), (p1, IDENTITY)], faces=face_list,
             ends=np.array(ends, np.float64).astype(F))
    w["caps"] = _caps(reached(w))
    return w


# ---------------------------------------------------------------------------------------------
# far: world coordinates of +-1.0e6 m (float32 spacing 0.0625 m), cell keys just inside +-2^20
# ---------------------------------------------------------------------------------------------
def far(seed=41):
    """Sensor-frame points within +-3 m (several to a leaf) under poses with yaw 0.3 rad and translations of 1.0e6 m on either side of 0: the FP64
    transform decides which of the 0.0625 m float32 steps a point lands on.  Update 2 returns to the cells of update 0.  Update 3
    also carries points 60 km further out, whose cell keys lie beyond +-2^20: world["out_of_range"] flags them."""
    rng = np.random.default_rng(seed)

    def local(n):
        return cloud(rng.uniform(-3.0, 3.0, (n, 3)) * [1.0, 1.0, 0.2], rng.uniform(0.0, 100.0, n))

    Ta, Tb = pose(0.3, [1.0e6, -1.0e6, 3.0]), pose(0.3, [-1.0e6, 1.0e6, -1.0e6])
    updates = [(local(600), Ta), (local(600), Tb), (local(400), Ta)]
    last = local(500)
    last[::5, 0] += 60000.0 * np.cos(0.3)
    last[::5, 1] -= 60000.0 * np.sin(0.3)          # (rotated by Ta: 60 km along world +x)
    updates.append((last, Ta))
    out = ~in_key_range(cell_keys(transform(last, Ta), SIZES))
    w = dict(name="far", sizes=SIZES, updates=updates, out_of_range=out)
    w["caps"] = _caps(reached(w, updates[:3] + [(last[~out], Ta)]))
    return w


# ---------------------------------------------------------------------------------------------
# many_cells: as many new and modified cells in one update as the lists of the assign kernel hold
# ---------------------------------------------------------------------------------------------
MANY = 256


def many_cells(seed=51):
    """Update 0: 4096 points, 16 in each of 256 new cells (a 16 x 16 square of cells).  The cells are dealt to two halves by a
    fixed permutation; the first half's points fill the input indices below 2048 in shuffled order, the second half's the rest,
    so that every cell of the second half first appears above index 1024 and the creation order follows neither the keys nor
    anything computed from them.  Update 1 returns to the same 256 cells.  Update 2 touches them and one cell more (257)."""
    xy, z, res = SIZES
    rng = np.random.default_rng(seed)
    cells = np.array([(i, j) for i in range(16) for j in range(16)])[rng.permutation(MANY)]

    def points_in(cell_list, per):
        c = np.repeat(cell_list, per, axis=0)
        p = np.zeros((len(c), 3))
        p[:, :2] = (c - 8) * xy + rng.uniform(0.2, xy - 0.2, (len(c), 2))
        p[:, 2] = rng.uniform(0.2, z - 0.2, len(c))
        return p[rng.permutation(len(p))]

    u0 = np.concatenate([points_in(cells[:MANY // 2], 16), points_in(cells[MANY // 2:], 16)])
    u1 = points_in(cells, 3)
    u2 = np.concatenate([points_in(cells, 1), [[8 * xy + 1.0, 1.0, 1.0]]])
    updates = [(cloud(u, seed=52 + k), IDENTITY) for k, u in enumerate((u0, u1, u2))]
    w = dict(name="many_cells", sizes=SIZES, updates=updates)
    w["caps"] = dict(max_cells=MANY + 1, cell_capacity=reached(w)["cell_capacity"], max_update_points=len(u0), max_modified_cells=MANY)
    return w


# ---------------------------------------------------------------------------------------------
# brim: one cell filled to its capacity, every leaf of it fed again
# ---------------------------------------------------------------------------------------------
def brim(seed=61):
    """max_modified_cells = 1, cell_capacity = 64, max_update_points = 128.  Update 0: 128 points, two in each of 64 leaves: the
    cell holds exactly cell_capacity leaves.  Update 1: one more point for each of the 64 leaves — no new leaf, nothing overflows,
    and the member lists hold 64 old + 64 new = 128 items in 64 leaves.  Update 2: a 65th leaf arrives."""
    xy, z, res = SIZES
    rng = np.random.default_rng(seed)
    corners = np.array([[res * (2 + 2 * (j % 8)), res * (2 + 2 * (j // 8)), res * 3] for j in range(64)])
    u0 = np.concatenate([_leaf_points(rng, c, res, 2) for c in corners])
    u1 = np.concatenate([_leaf_points(rng, c, res, 1) for c in corners])
    u2 = _leaf_points(rng, [res * 2, res * 2, res * 9], res, 1)
    updates = [(cloud(u[rng.permutation(len(u))], seed=62 + k), IDENTITY) for k, u in enumerate((u0, u1, u2))]
    return dict(name="brim", sizes=SIZES, updates=updates,
                caps=dict(max_cells=4, cell_capacity=64, max_update_points=128, max_modified_cells=1))


# ---------------------------------------------------------------------------------------------
# thousands: more cells than one plan of a concatenation holds (4096), made on the host
# ---------------------------------------------------------------------------------------------
def thousands(n_cells):
    """n_cells cells of one point each, as the list of cell clouds api.build_map_state takes (creation order = a fixed
    permutation of a 72-wide strip of cells)."""
    xy, z, res = SIZES
    rng = np.random.default_rng(71)
    idx = rng.permutation(n_cells)
    p = np.zeros((n_cells, 3))
    p[:, 0] = (idx % 72 - 36) * xy + rng.uniform(0.2, xy - 0.2, n_cells)
    p[:, 1] = (idx // 72 - 28) * xy + rng.uniform(0.2, xy - 0.2, n_cells)
    p[:, 2] = rng.uniform(0.2, z - 0.2, n_cells)
    c = cloud(p, seed=72)
    return dict(name="thousands", sizes=SIZES, cells=[c[i:i + 1] for i in range(n_cells)],
                caps=dict(max_cells=n_cells, cell_capacity=4, max_update_points=16, max_modified_cells=4))


WORLDS = {
    "crowded-0": lambda: crowded(CROWDED_ORIGINS[0]),
    "crowded-1000": lambda: crowded(CROWDED_ORIGINS[1]),
    "faces-10-0.5": lambda: faces(FACES_SIZES[0]),
    "faces-25-0.3": lambda: faces(FACES_SIZES[1]),
    "faces-40-0.4": lambda: faces(FACES_SIZES[2]),
    "far": far,
    "many_cells": many_cells,
    "brim": brim,
}
_made = {}


def world(name):
    """The world `name`, generated once and shared (read-only) by every test that asks for it."""
    if name not in _made:
        _made[name] = WORLDS[name]()
    return _made[name]
