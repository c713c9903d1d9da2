"""liodom_map_prune and the auto-prune of liodom_attach_mapper_ex.  The definition under test: after a prune the map is what
liodom_map_import_state would make of its own blob with the dropped cells' records and points taken out.  The expected blobs
are written by api.build_map_state from the designed cells (or filtered out of a parsed blob), so the prune kernels are pinned
independently of the pack and unpack kernels."""
import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
from mapper_lag_common import EPR, H, K, P, R, W, T_of, same, scans_of
from test_gpu_map_state import P as PTS, cell_points, clustered_update, pose

pytestmark = pytest.mark.gpu

SIZES = [(10.0, 10.0, 0.25), (40.0, 50.0, 0.4)]
KEEP = 20            # keep box of the designed maps: 41 x 41 cells of one z layer around cell (0, 0, 0)


def _inside(i):
    """i-th place inside the keep box (cell indices), walking the 41 x 41 square row by row."""
    return (i % 41 - KEEP, (i // 41) % 41 - KEEP, 0)


def _outside(i):
    """i-th place outside it: beyond the box in x, in y, or in the next z layer (keep_z = 0), in turn."""
    r = i // 3
    return ((KEEP + 1 + r, -(r % 7), 0), (r % 9 - 4, -(KEEP + 1) - r, 0), (r % 41 - KEEP, (r // 41) % 41 - KEEP, 1 + (r // 1681) % 2 * -2))[i % 3]


def _case(name):
    """-> (n_cells, set of removed ids, counts per cell, capacities).  Counts differ from cell to cell."""
    cnt = lambda n: [1 + (7 * i) % 12 for i in range(n)]      # noqa: E731
    small = dict(max_cells=80, cell_capacity=64)
    table = {
        "none": (6, set(), cnt(6), small),
        "all": (6, set(range(6)), cnt(6), small),
        "first only": (6, {0}, cnt(6), small),
        "last only": (6, {5}, cnt(6), small),
        "alternating": (9, set(range(0, 9, 2)), cnt(9), small),
        "ids change": (8, {0, 3}, cnt(8), small),
        "at capacity": (4, {0}, [5, 9, 300, 300], dict(max_cells=8, cell_capacity=300)),
        "1 cell kept": (1, set(), [7], small),
        "1 cell dropped": (1, {0}, [7], small),
        "63 cells": (63, set(range(1, 63, 2)), cnt(63), small),
        "64 cells": (64, set(range(0, 64, 2)), cnt(64), small),
        "65 cells": (65, set(range(0, 65, 3)) | {64}, cnt(65), small),
        "300 cells": (300, set(range(2, 300, 3)), cnt(300), dict(max_cells=320, cell_capacity=64)),
        "1025 cells": (1025, set(range(0, 1025, 2)) - {1024} | {1023}, cnt(1025), dict(max_cells=1100, cell_capacity=64)),
    }
    return table[name]


CASES = ["none", "all", "first only", "last only", "alternating", "ids change", "at capacity", "1 cell kept", "1 cell dropped",
         "63 cells", "64 cells", "65 cells", "300 cells", "1025 cells"]


def _designed_map(sizes, name):
    """The map of a case, and its cells as the test knows them.  The blob of the designed cells is imported (every cell in slab
    0); then every third cell below capacity takes one more point through liodom_map_update, in a leaf behind all of its leaves,
    which moves those cells to slab 1: current slabs are mixed, the case an in-place move gets wrong."""
    xy, z, res = sizes
    n, removed, counts, caps = _case(name)
    rng = np.random.default_rng(len(name) * 1000 + n)
    place, n_in, n_out = [], 0, 0
    for i in range(n):
        if i in removed:
            place.append(_outside(n_out)); n_out += 1
        else:
            place.append(_inside(n_in)); n_in += 1
    corners = [(kx * xy, ky * xy, kz * z) for kx, ky, kz in place]
    cells = [cell_points(rng, counts[i], corners[i], res) for i in range(n)]
    m = la.Map(xy, z, res, max_update_points=256, max_modified_cells=256, **caps)
    m.import_state(api.build_map_state(xy, z, res, cells))
    extra = [i for i in range(n) if i % 3 == 1 and counts[i] < caps["cell_capacity"]]
    for lo in range(0, len(extra), 200):
        ids = extra[lo:lo + 200]
        x = np.zeros((len(ids), 4), np.float32)
        for r, i in enumerate(ids):
            x[r] = (corners[i][0] + res * 1.5, corners[i][1] + res * 1.5, corners[i][2] + res * 30.5, 500.0 + i)
            cells[i] = np.concatenate([cells[i], x[r:r + 1]])
        m.update(x)
    assert m.status() == 0 and m.num_cells() == n
    assert m.export_state() == api.build_map_state(xy, z, res, cells)       # the test's picture of the map is right
    return m, cells, removed


@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_designed_maps(sizes, name):
    xy, z, res = sizes
    m, cells, removed = _designed_map(sizes, name)
    before = m.export_state()
    T = pose(0.4, [xy * 0.3, xy * 0.6, z * 0.5])                           # somewhere in cell (0, 0, 0)
    n_removed = m.prune(T, KEEP, 0)
    assert n_removed == len(removed), name
    kept = [c for i, c in enumerate(cells) if i not in removed]
    assert m.num_cells() == len(kept) and m.status() == 0
    after = m.export_state()
    assert after == api.build_map_state(xy, z, res, kept), name
    if not removed:
        assert after == before
    # every survivor is found through the rebuilt hash, no dropped cell is
    for i in list(range(len(cells)))[:: max(1, len(cells) // 40)]:
        c = cells[i]
        got = m.local(pose(0.0, [float(int(c[0, 0])), float(int(c[0, 1])), float(int(c[0, 2]))]), 0, 0)
        assert (got.shape[0] == 0) if i in removed else same(got[:len(c)], c), (name, i)
    assert m.prune(T, KEEP, 0) == 0 and m.export_state() == after          # pruning again changes nothing
    if name == "all":                                                      # equals reset; and the map goes on working
        f = la.Map(xy, z, res, max_cells=8, cell_capacity=64)
        assert after == f.export_state() and m.all().shape == (0, 4)
        m.update(cells[0]); f.update(cells[0])
        assert m.export_state() == f.export_state() and m.num_cells() == 1
        f.close()
    m.close()


@pytest.mark.parametrize("sizes", SIZES)
def test_all_keeps_the_status(sizes):
    xy, z, res = sizes
    m = la.Map(xy, z, res, max_cells=4, cell_capacity=64, max_update_points=256, max_modified_cells=4)
    x = np.zeros((200, 4), np.float32)
    x[:, 0] = np.linspace(0.01, 0.99 * xy, 200)
    x[:, 1] = res * (0.5 + np.arange(200) % 3)                             # three rows of leaves along x: > 64 distinct leaves in one cell
    m.update(x)
    assert m.status() & 8 and m.num_cells() == 1
    assert m.prune(pose(0.0, [5 * xy, 0.0, 0.0]), 1, 1) == 1
    assert m.num_cells() == 0 and m.status() & 8
    assert m.export_state() == api.build_map_state(xy, z, res, [], status=m.status())
    m.close()


# translation -> cell index of the centre: the reference truncates toward zero FIRST (map.cc:144-151), so -0.5 is cell 0, not -1
EDGE_POSES = [(-0.5, 0), (39.9, 0), (40.0, 1), (-40.0, -1)]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("t,centre", EDGE_POSES)
@pytest.mark.parametrize("keep", [0, 1, 2])
def test_box_edges(axis, t, centre, keep):
    """A line of cells along one axis (40 m cells in xy, 40 m in z here, so that the four translations mean the same on every
    axis): the cell exactly keep * size away from the centre cell is kept, the next one out is dropped."""
    xy = z = 40.0
    res = 0.4
    idx = list(range(-5, 6))
    rng = np.random.default_rng(3)
    cells = []
    for i in idx:
        corner = [0.0, 0.0, 0.0]
        corner[axis] = i * 40.0
        cells.append(cell_points(rng, 3, corner, res))
    m = la.Map(xy, z, res, max_cells=16, cell_capacity=16, max_update_points=16, max_modified_cells=4)
    m.import_state(api.build_map_state(xy, z, res, cells))
    tr = [3.0, 3.0, 3.0]
    tr[axis] = t
    # the other two axes keep 0 cells: every cell of the line shares them with the centre
    kxy, kz = (keep, 0) if axis < 2 else (0, keep)
    n_removed = m.prune(pose(0.0, tr), kxy, kz)
    kept = [c for i, c in zip(idx, cells) if abs(i - centre) <= keep]
    assert len(kept) == 2 * keep + 1 and n_removed == len(cells) - len(kept)
    assert m.export_state() == api.build_map_state(xy, z, res, kept), (axis, t, keep)
    m.close()


def _filtered(blob, sizes, T, keep_xy, keep_z):
    """The blob with the records and points of the cells outside the keep box taken out (pure Python)."""
    xy, z, res = sizes
    st = api.parse_map_state(blob, sizes=sizes)
    v = api.map_cell_key([float(int(T[0][3])), float(int(T[1][3])), float(int(T[2][3]))], xy, z)
    lim = (keep_xy * xy, keep_xy * xy, keep_z * z)
    keep = [all(abs(float(k[a]) - float(v[a])) <= lim[a] for a in range(3)) for k in st["keys"]]
    cells = [c for c, kp in zip(st["cells"], keep) if kp]
    dropped = [tuple(int(q) for q in k) for k, kp in zip(st["keys"], keep) if not kp]
    return api.build_map_state(xy, z, res, cells, status=st["status"]), dropped


@pytest.mark.parametrize("sizes", SIZES)
def test_continuation_equals_the_imported_filtered_blob(sizes):
    xy, z, res = sizes
    rng = np.random.default_rng(21)
    caps = dict(max_cells=512, cell_capacity=8192, max_update_points=1024, max_modified_cells=128)
    m = la.Map(xy, z, res, **caps)
    for k in range(8):
        m.update(*clustered_update(rng, k, res))
    T = pose(0.1, [3.0, -2.0, 0.5])
    keep = (1, 0) if xy < 20 else (0, 0)
    want, dropped = _filtered(m.export_state(), sizes, T, *keep)
    if xy < 20:
        assert len(dropped) > 2 and m.num_cells() - len(dropped) > 2
    assert m.prune(T, *keep) == len(dropped)
    assert m.export_state() == want
    f = la.Map(xy, z, res, max_cells=300, cell_capacity=4096, max_update_points=1024, max_modified_cells=128)
    f.import_state(want)
    recreated = set()
    for k in range(8, 18):
        x, Tk = clustered_update(rng, k, res)
        m.update(x, Tk); f.update(x, Tk)
        assert same(m.all(), f.all()) and m.num_cells() == f.num_cells() and m.status() == f.status(), k
        for Tq in (Tk, T):
            assert same(m.local(Tq, 2, 1), f.local(Tq, 2, 1)) and same(m.local(Tq, 1, 0), f.local(Tq, 1, 0)), k
        recreated |= set(tuple(int(q) for q in key) for key in api.parse_map_state(m.export_state())["keys"]) & set(dropped)
    if xy < 20:
        assert recreated                       # pruned keys came back as new cells
    assert m.export_state() == f.export_state() and m.status() == 0
    m.close(); f.close()


def test_prune_frees_room_after_cells_full():
    xy, z, res = 40.0, 50.0, 0.4
    m = la.Map(xy, z, res, max_cells=4, cell_capacity=64, max_update_points=256, max_modified_cells=8)
    line = PTS(*[(xy * i + 5.0, 5.0, 5.0, float(i)) for i in range(8)])
    m.update(line)                                   # 8 cells into a map of 4: the last four get "no room" slots
    assert m.status() & 2 and m.num_cells() == 4 and same(m.all(), line[:4])
    m.update(line[6:7])
    assert m.num_cells() == 4 and m.all().shape[0] == 4          # still no room
    assert m.prune(pose(0.0, [45.0, 0.0, 0.0]), 0, 0) == 3       # keeps cell 1
    assert m.num_cells() == 1 and same(m.all(), line[1:2]) and m.status() & 2
    m.update(line[5:8])                              # keys that had been marked "no room" are created now
    assert m.num_cells() == 4 and same(m.all(), np.concatenate([line[1:2], line[5:8]]))
    assert m.export_state() == api.build_map_state(xy, z, res, [line[1:2], line[5:6], line[6:7], line[7:8]], status=m.status())
    assert m.status() & 2                            # sticky
    m.close()


def test_rejections_leave_the_map_untouched():
    m = la.Map(40.0, 50.0, 0.4, max_cells=8, cell_capacity=64)
    m.update(PTS((1.0, 1.0, 1.0, 1.0), (100.0, 1.0, 1.0, 2.0)))
    before = m.export_state()
    L = la.load()
    T = np.ascontiguousarray(np.eye(4)[:3], np.float64).reshape(12)
    Tp = T.ctypes.data_as(api.C.POINTER(api.C.c_double))
    assert L.liodom_map_prune(m.h, None, 1, 1, None) == api.ERR_INVALID_ARG
    assert L.liodom_map_prune(None, Tp, 1, 1, None) == api.ERR_INVALID_ARG
    assert L.liodom_map_prune(m.h, Tp, -1, 1, None) == api.ERR_INVALID_ARG
    assert L.liodom_map_prune(m.h, Tp, 1, -1, None) == api.ERR_INVALID_ARG
    with pytest.raises(la.LiodomError) as ei:
        m.prune(None, 0, -3)
    assert ei.value.code == api.ERR_INVALID_ARG
    assert m.export_state() == before
    assert L.liodom_map_prune(m.h, Tp, 0, 0, None) == 0          # n_removed is optional
    assert m.num_cells() == 1
    m.close()


# ---------------------------------------------------------------------------------------------
# attached maps: liodom_map_prune on the handle's stream, and the auto-prune
# ---------------------------------------------------------------------------------------------
MAP_SZ = (20.0, 25.0, 0.4)        # keep_z * voxel_zsize = 25 >= cells_z * voxel_xysize = 20: the z condition holds
MAP_CAPS = dict(max_cells=512, cell_capacity=8192, max_modified_cells=256)
KEEP_BOX_CELLS = (2 * 2 + 1) ** 2 * (2 * 1 + 1)


def _handle():
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                     la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))


@pytest.mark.parametrize("lag", [1, 0])
def test_auto_prune_equals_prune_on_the_attached_map(synth, lag):
    scans = scans_of(synth)
    gA, mA, gB, mB = _handle(), la.Map(*MAP_SZ, **MAP_CAPS), _handle(), la.Map(*MAP_SZ, **MAP_CAPS)
    gA.attach_mapper(mA, 2, 1, lag=lag, prune_period=3, keep_cells_xy=2, keep_cells_z=1)
    gB.attach_mapper(mB, 2, 1, lag=lag)
    removed = 0
    for k in range(K):
        pa, _ = gA.process_scan(scans[k], H, W)
        pb, _ = gB.process_scan(scans[k], H, W)
        grown = mB.num_cells()
        if (k + 1) % 3 == 0:
            removed += mB.prune(T_of(pb), 2, 1)      # on the attached map, after the same scans
            assert mA.num_cells() <= KEEP_BOX_CELLS, k
        assert np.array_equal(pa, pb), k
        assert same(gA.received_map(), gB.received_map()), k
        assert mA.export_state() == mB.export_state(), k
        assert mA.num_cells() <= grown
    assert removed > 0 and mA.num_cells() > 0 and len(gA.received_map()) > 0
    assert mA.status() == mB.status() == 0
    for g, m in ((gA, mA), (gB, mB)):
        g.attach_mapper(None)
        g.close(); m.close()


def test_options_that_break_an_auto_prune_condition_are_rejected(synth):
    scans = scans_of(synth, count=P + 2)
    g, m, other = _handle(), la.Map(*MAP_SZ, **MAP_CAPS), la.Map(40.0, 30.0, 0.4, max_cells=16, cell_capacity=64)
    g.attach_mapper(m, 2, 1, lag=1)
    bad = [(m, dict(cells_xy=2, cells_z=1, prune_period=3, keep_cells_xy=1, keep_cells_z=1)),       # keep_xy < cells_xy
           (m, dict(cells_xy=2, cells_z=2, prune_period=3, keep_cells_xy=2, keep_cells_z=1)),       # 1 * 25 < 2 * 20
           (other, dict(cells_xy=2, cells_z=1, prune_period=1, keep_cells_xy=2, keep_cells_z=1)),   # 1 * 30 < 1 * 40
           (m, dict(lag=2)), (m, dict(prune_period=-1)), (m, dict(keep_cells_z=-1)), (m, dict(cells_xy=-1))]
    for mp, kw in bad:
        with pytest.raises(la.LiodomError):
            g.attach_mapper(mp, **kw)
    assert g.modes()["mapper_lag"] == "1"
    for x in scans:                                  # the earlier attachment stays: m goes on receiving what leaves the window
        g.process_scan(x, H, W)
    assert m.num_cells() > 0 and len(g.received_map()) > 0 and other.num_cells() == 0
    other.update(PTS((1.0, 1.0, 1.0, 1.0)))          # ... and the rejected map is still its own
    assert other.num_cells() == 1
    g.attach_mapper(m, 2, 1, lag=1, prune_period=2, keep_cells_xy=2, keep_cells_z=1)      # both conditions met (equality)
    g.attach_mapper(None)
    g.close(); m.close(); other.close()
