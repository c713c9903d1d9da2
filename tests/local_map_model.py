"""A NumPy restatement of Map::getLocalMap's visit and the designed worlds of the local-map tests.  Plain Python: no library, no
GPU.  Independent of the kernels: tests/test_gpu_designed_local.py compares k_map_local_plan + k_map_gather and k_map_local_rows
against it, tests/test_local_map_model.py holds it bit-equal to the CPU oracle (orc.Map.local).

The visit (src/map.cc:141-189 of the reference, as restated in oracle/liodom_oracle.cc getLocalMap):
  centre   the translation is truncated to int first; an axis' key is int(floor(x * (1 / size)) * size + size / 2), in FP64
  square   int i from int(vx - cells_xy * xy) while i <= int(vx + cells_xy * xy), advancing by i = int(i + xy); j likewise inside;
           keys (i, j, vz), x outer and y inner
  column   int k from int(vz - cells_z * xy) while k <= int(vz + cells_z * xy) (the extent is taken from the XY size), advancing by
           k = int(k + z); keys (vx, vy, k).  Where the column's steps land on vz the centre cell is visited a second time.
int() truncates towards zero, as the C cast does, so a loop steps unevenly at non-integer sizes and differently on either side of 0.

A world is a dict(name, sizes = (xy, z, res), state = a model state of tests/map_paging_model.py (keys, corner_leaf, cells, status)
in creation order, caps = the smallest liodom_map_config_t capacities that hold it); blob(world) is its map-state blob and
feed(orc_map, world) puts the same points into an orc.Map through update.  Every cell's points are distinct leaf centres inside the
cell in ascending (z, y, x) leaf order, which is what a VoxelGrid leaves of them, bit for bit: a sum of one point divided by 1."""
import functools
import math

import numpy as np

from liodom_amd import api
from map_paging_model import blob_of

F = np.float32
VISIT_MAX = 65536          # the planners' loop guard (kMapVisitMax of liodom_map.h)
ENTRIES_MAX = 4096         # kMapLocalEntriesMax
ROWS_KEYS_MAX = 1024       # kMapRowsKeysMax
ROWS_GRID_X = 16           # kMapRowsGridX
ROWS_THREADS = 256         # kMapRowsThreads


def pose(t, yaw=0.0):
    T = np.eye(4)[:3].copy()
    c, s = math.cos(yaw), math.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:, 3] = t
    return T


def same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# the visit
# ---------------------------------------------------------------------------------------------
def axis_key(x, size):
    """The key of the int coordinate x: int(floor(x * (1 / size)) * size + size / 2)."""
    size = float(size)
    return int(math.floor(float(x) * (1.0 / size)) * size + size / 2.0)


@functools.lru_cache(maxsize=None)
def axis_steps(centre, extent, step):
    """The values one loop takes: from int(centre - extent) while <= int(centre + extent), i = int(i + step)."""
    init, end = int(centre - extent), int(centre + extent)
    out, i = [], init
    while i <= end:
        out.append(i)
        i = int(i + step)
    return tuple(out)


def centre_of(T34, sizes):
    T = np.asarray(T34, np.float64).reshape(3, 4)
    return (axis_key(int(T[0, 3]), sizes[0]), axis_key(int(T[1, 3]), sizes[0]), axis_key(int(T[2, 3]), sizes[1]))


def _loops(T34, sizes, cells_xy, cells_z):
    xy, z = float(sizes[0]), float(sizes[1])
    vx, vy, vz = centre_of(T34, sizes)
    return (vx, vy, vz), axis_steps(vx, cells_xy * xy, xy), axis_steps(vy, cells_xy * xy, xy), axis_steps(vz, cells_z * xy, z)


def visit(T34, sizes, cells_xy, cells_z):
    """-> list of (kx, ky, kz) in the reference's order."""
    (vx, vy, vz), xs, ys, zs = _loops(T34, sizes, cells_xy, cells_z)
    return [(i, j, vz) for i in xs for j in ys] + [(vx, vy, k) for k in zs]


def visit_size(T34, sizes, cells_xy, cells_z):
    """len(visit(...)) without building the list."""
    _, xs, ys, zs = _loops(T34, sizes, cells_xy, cells_z)
    return len(xs) * len(ys) + len(zs)


def visit_cut(T34, sizes, cells_xy, cells_z, limit=VISIT_MAX):
    """-> (keys, cut): the visit as the device's planners walk it, which count every iteration of the inner and of the outer loops
    and stop all three at `limit`; cut = keys were left out."""
    (vx, vy, vz), xs, ys, zs = _loops(T34, sizes, cells_xy, cells_z)
    out, guard = [], 0
    for i in xs:
        if guard >= limit:
            return out, True
        for j in ys:
            if guard >= limit:
                return out, True
            out.append((i, j, vz))
            guard += 1
        guard += 1
    for k in zs:
        if guard >= limit:
            return out, True
        out.append((vx, vy, k))
        guard += 1
    return out, False


def found(state, keys):
    """The visited keys that are cells of the state, in visit order, as indices into the state's lists (duplicates stay)."""
    ids = {tuple(k): c for c, k in enumerate(state["keys"])}
    return [ids[k] for k in keys if k in ids]


def entries(state, T34, sizes, cells_xy, cells_z):
    """The plan of a local map: [(cell, offset, count)] of the found cells in visit order; the total is offset + count of the last."""
    out, total = [], 0
    for c in found(state, visit(T34, sizes, cells_xy, cells_z)):
        n = state["cells"][c].shape[0]
        out.append((c, total, n))
        total += n
    return out


def _concat(state, cells):
    return np.concatenate([state["cells"][c] for c in cells]).astype(F) if cells else np.zeros((0, 4), F)


def local(state, T34, sizes, cells_xy, cells_z):
    """-> [n, 4] float32: the found cells' points, concatenated in visit order."""
    return _concat(state, found(state, visit(T34, sizes, cells_xy, cells_z)))


def local_device(state, T34, sizes, cells_xy, cells_z):
    """-> (points, overflow): what the device's planners make of a visit beyond their limits — the loops cut at VISIT_MAX, then the
    first ENTRIES_MAX found cells; overflow = either limit was met (LIODOM_MAP_RESULT_OVERFLOW)."""
    keys, cut = visit_cut(T34, sizes, cells_xy, cells_z)
    cells = found(state, keys)
    return _concat(state, cells[:ENTRIES_MAX]), cut or len(cells) > ENTRIES_MAX


def rows_bound(sizes, cells_xy, cells_z):
    """nx * nx + nz of map_rows_fit (liodom_map_host.h), restated; None where it declines (a size below 1, a negative extent)."""
    xy, z = float(sizes[0]), float(sizes[1])
    if not (xy >= 1.0) or not (z >= 1.0) or cells_xy < 0 or cells_z < 0:
        return None
    nx = math.floor((2.0 * cells_xy * xy + 2.0) / math.floor(xy)) + 1.0
    nz = math.floor((2.0 * cells_z * xy + 2.0) / math.floor(z)) + 1.0
    return nx * nx + nz


def rows_fit(sizes, cells_xy, cells_z):
    b = rows_bound(sizes, cells_xy, cells_z)
    return b is not None and b <= ROWS_KEYS_MAX


def rows_slices(total, cap):
    """[(lo, hi)] of the workgroups of one k_map_local_rows row: n = min(total, cap) points dealt to min(16, ceil(cap / 256))
    workgroups in contiguous slices of ceil(n / workgroups)."""
    n = min(total, cap)
    gx = max(1, min(ROWS_GRID_X, (cap + ROWS_THREADS - 1) // ROWS_THREADS))
    per = (n + gx - 1) // gx
    out = []
    for b in range(gx):
        lo = min(n, b * per)
        out.append((lo, min(n, lo + per)))
    return out


# ---------------------------------------------------------------------------------------------
# worlds
# ---------------------------------------------------------------------------------------------
def _leaf_points(corner, res, leaves, shape):
    """The centres of the leaves with linear indices `leaves` (ascending: x fastest, then y, then z) of a cell at `corner`."""
    lin = np.asarray(sorted(leaves), np.int64)
    l3 = np.stack([lin % shape[0], (lin // shape[0]) % shape[1], lin // (shape[0] * shape[1])], axis=1)
    return np.asarray(corner, np.float64) + (l3 + 0.5) * res


def _world(name, sizes, clouds):
    """clouds: [n, 3] float64 arrays, one per cell in creation order.  Intensity = the point's running index."""
    xy, z, res = sizes
    state = dict(keys=[], corner_leaf=[], cells=[], status=0)
    first = 0
    for xyz in clouds:
        c = np.zeros((len(xyz), 4), F)
        c[:, :3] = xyz
        c[:, 3] = np.arange(first, first + len(xyz))
        first += len(xyz)
        assert np.array_equal(c[:, :3].astype(np.float64), xyz)          # leaf centres are float32 values
        keys = {tuple(api.map_cell_key(p, xy, z)) for p in c[:, :3]}
        assert len(keys) == 1, (name, keys)                              # ... of one cell
        state["keys"].append(keys.pop())
        state["corner_leaf"].append(tuple(api.map_cell_corner_leaf(c[0, :3], xy, z, res)))
        state["cells"].append(c)
    assert len(set(state["keys"])) == len(state["keys"]) and first < (1 << 24)
    caps = dict(max_cells=len(clouds), cell_capacity=max(4, max(len(c) for c in clouds)), max_update_points=16, max_modified_cells=4)
    return dict(name=name, sizes=tuple(float(s) for s in sizes), state=state, caps=caps)


def blob(world):
    return blob_of(world["state"], world["sizes"])


def feed(orc_map, world):
    """The world's points into an orc.Map, cell after cell in creation order."""
    for c in world["state"]["cells"]:
        orc_map.update(c)
    return orc_map


_oracle = {}


def oracle_map(orc, name):
    """The world `name` in an orc.Map, fed once and never modified."""
    if name not in _oracle:
        w = world(name)
        mo = feed(orc.Map(*w["sizes"]), w)
        assert mo.num_cells() == len(w["state"]["keys"]) and same(mo.all(), np.concatenate(w["state"]["cells"]))
        _oracle[name] = mo
    return _oracle[name]


COUNTS_SIZES = (4.0, 5.0, 0.25)
COUNT_SET = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000)
COUNTS_HOLES = (10, 23, 45)          # places of the 7 x 7 square, in visit order, that hold no cell
COUNTS_CENTRE = 24                   # the centre's place; the two after it hold 1 and 1000 points


def counts_deal():
    """Points per place of the 7 x 7 square in visit order at the origin (x outer, y inner); 0: no cell."""
    n = [COUNT_SET[(5 * i + 3) % len(COUNT_SET)] for i in range(49)]
    n[COUNTS_CENTRE], n[COUNTS_CENTRE + 1], n[COUNTS_CENTRE + 2] = 257, 1, 1000
    for i in COUNTS_HOLES:
        n[i] = 0
    return n


def counts(seed=81):
    """7 x 7 cells of 4 x 4 x 5 m at the z layer of the origin and the cells above and below the centre; per-cell counts dealt by
    counts_deal (65 above, 513 below); creation order: a fixed permutation."""
    xy, z, res = COUNTS_SIZES
    rng = np.random.default_rng(seed)
    shape = (16, 16, 20)
    n_leaves = shape[0] * shape[1] * shape[2]
    cells = [((i // 7 - 3, i % 7 - 3, 0), n) for i, n in enumerate(counts_deal()) if n > 0] + [((0, 0, 1), 65), ((0, 0, -1), 513)]
    clouds = []
    for k in rng.permutation(len(cells)):
        (a, b, c), n = cells[k]
        clouds.append(_leaf_points([a * xy, b * xy, c * z], res, rng.choice(n_leaves, n, replace=False), shape))
    return _world("counts", COUNTS_SIZES, clouds)


ONES_SIZES = (1.0, 1.0, 0.25)


def ones(nx=70, ny=60, seed=82):
    """nx x ny one-point cells of 1 x 1 x 1 m at x in [0, nx), y in [0, ny), z in [0, 1); creation order: a fixed permutation."""
    rng = np.random.default_rng(seed)
    clouds = [np.array([[k // ny + 0.625, k % ny + 0.375, 0.125]]) for k in rng.permutation(nx * ny)]
    return _world("ones-%dx%d" % (nx, ny), ONES_SIZES, clouds)


def ones_pose(nx=70, ny=60):
    """A pose in the middle of the block: get_local(., 40, 0) from here finds every cell of it, and the centre cell a second time
    (nx * ny + 1 entries: 4201 of `ones`, and exactly 4096 of the 65 x 63 block)."""
    return pose([nx // 2 + 0.2, ny // 2 + 0.7, 0.3], 0.4)


GUARD_POSE = pose([500.4, 500.6, 0.2], -0.2)
GUARD_OFFSETS = [(dx, dy) for dx in (-128, -127, 0, 127, 128) for dy in (-128, -127, 0, 127, 128)] + \
                [(126, -128), (126, -125), (126, -124), (126, 0), (125, 128), (3, -77), (-90, 41), (-128, 5), (64, 64), (1, 1)]


def guard_world(seed=83):
    """A few dozen one-point cells of 1 x 1 x 1 m around GUARD_POSE (all coordinates positive), out to +-128 cells on x and y.
    cells_xy = 127 visits 255 x 255 + 1 keys in 65281 loop iterations: under the planners' guard of 65536.  cells_xy = 128 visits
    257 x 257 + 1: the guard cuts the visit in the row of x offset 126 after y offset -125 — (126, -124) and everything behind it,
    the column's second visit of the centre included, is left out."""
    rng = np.random.default_rng(seed)
    clouds = [np.array([[500 + GUARD_OFFSETS[k][0] + 0.625, 500 + GUARD_OFFSETS[k][1] + 0.375, 0.125]]) for k in rng.permutation(len(GUARD_OFFSETS))]
    return _world("guard", ONES_SIZES, clouds)


FRAC_SIZES = (2.5, 1.5, 0.25)
FRAC_CELLS_Z = 1


def frac(seed=84):
    """One-point cells of 2.5 x 2.5 x 1.5 m: 31 x 31 around the origin at the z layer of 0 and a column of 8 through the centre
    (without the layer [-1.5, 0): its key int(-0.75) is 0, the key of the layer above it).  At these sizes the loops step by 2 and
    3 (1 and 2) in turn, so only some visited keys are cell keys: which ones is the test."""
    xy, z, res = FRAC_SIZES
    rng = np.random.default_rng(seed)
    cells = [(a, b, 0) for a in range(-15, 16) for b in range(-15, 16)] + [(0, 0, c) for c in range(-4, 5) if c not in (0, -1)]
    clouds = [np.array([[cells[k][0] * xy + 0.625, cells[k][1] * xy + 0.375, cells[k][2] * z + 0.125]]) for k in rng.permutation(len(cells))]
    return _world("frac", FRAC_SIZES, clouds)


def frac_cells_xy():
    """The largest cells_xy that map_rows_fit admits at FRAC_SIZES with cells_z = 1, by the restated bound."""
    c = 0
    while rows_fit(FRAC_SIZES, c + 1, FRAC_CELLS_Z):
        c += 1
    return c


FRAC_POSES = [pose([0.0, 0.0, 0.0]), pose([-0.9, 0.9, -0.9], 0.3), pose([2.5 + 1e-6, -2.5 - 1e-6, 1.6]), pose([-7.0, 5.0, -3.0], 1.0),
              pose([11.2, -13.9, 0.7]), pose([-4.9999, 4.9999, 2.9999])]

_made = {}


def world(name):
    """The world `name`, generated once and shared (read-only) by every test that asks for it."""
    if name not in _made:
        _made[name] = {"counts": counts, "ones": ones, "ones-65x63": lambda: ones(65, 63), "guard": guard_world, "frac": frac}[name]()
    return _made[name]


# ---------------------------------------------------------------------------------------------
# poses and extents of the host-call tests on `counts`, and the capacities of the step tests
# ---------------------------------------------------------------------------------------------
COUNTS_EXTENTS = [(0, 0), (1, 0), (2, 1), (3, 2)]
COUNTS_POSES = [
    pose([0.0, 0.0, 0.0]),                      # 0  the origin
    pose([0.9, 0.0, 0.0], 0.3),                 # 1-6  +-0.9 on each axis: truncated to 0, where floor would go to -1
    pose([-0.9, 0.0, 0.0], -0.3),
    pose([0.0, 0.9, 0.0], 1.2),
    pose([0.0, -0.9, 0.0], -1.2),
    pose([0.0, 0.0, 0.9], 2.0),
    pose([0.0, 0.0, -0.9], -2.0),
    pose([4.0 + 1e-6, -4.0 - 1e-6, 0.0]),       # 7, 8  a cell boundary +- 1e-6
    pose([4.0 - 1e-6, -4.0 + 1e-6, 5.0 + 1e-6]),
    pose([14.5, -5.5, 1.5], 0.7),               # 9  the square hangs half outside the block
    pose([1000.0, -1000.0, 0.0]),               # 10  nothing there
    pose([0.9, 0.0, 0.0], 0.3),                 # 11  = 1: two equal poses in one batch
]
STEP_EXTENTS = (3, 0)          # the readers of the step tests: the whole square, and the centre cell a second time


LOCKSTEP_EXTENTS = (1, 0)      # the first stream of the lock-step test: 3 x 3 places around the centre (one a hole), the centre twice


def lockstep_cap(world_counts):
    """recv_capacity of the lock-step test: the size of the origin's local map with LOCKSTEP_EXTENTS."""
    en = entries(world_counts["state"], COUNTS_POSES[0], world_counts["sizes"], *LOCKSTEP_EXTENTS)
    return en[-1][1] + en[-1][2]


STEP_CAP_NAMES = ("one", "256", "257", "entry_end", "entry_end+1", "in_first_copy", "in_second_copy", "total-1", "total", "total+1")


def step_caps(world_counts, T34=None):
    """{name: recv_capacity} of the step tests, from the plan of the local map at T34 (the origin) with STEP_EXTENTS."""
    T = COUNTS_POSES[0] if T34 is None else T34
    en = entries(world_counts["state"], T, world_counts["sizes"], *STEP_EXTENTS)
    total = en[-1][1] + en[-1][2]
    centre = [e for e in en if world_counts["state"]["keys"][e[0]] == centre_of(T, world_counts["sizes"])]
    end = en[2][1] + en[2][2]          # the end of the third entry
    return {"one": 1, "256": 256, "257": 257, "entry_end": end, "entry_end+1": end + 1, "in_first_copy": centre[0][1] + 100,
            "in_second_copy": centre[1][1] + 100, "total-1": total - 1, "total": total, "total+1": total + 1}
