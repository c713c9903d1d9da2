"""Paging of the device map: liodom_map_evict (prune whose dropped cells come out as a blob), liodom_map_merge_state (import that
appends) and liodom_amd.pager.MapPager on top of them.  Expected blobs are written in Python (api.build_map_state /
api.join_map_state, map_paging_model.py), independent of the kernels under test.  The designed maps are those of
test_gpu_map_prune: their cells sit in mixed current slabs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
from liodom_amd.pager import MapPager
import map_paging_model as mm
from mapper_lag_common import EPR, H, P, R, W, T_of, same
from test_gpu_map_prune import CASES, KEEP, SIZES, _designed_map, _inside, _outside
from test_gpu_map_state import P as PTS, cell_points, clustered_update, pose

pytestmark = pytest.mark.gpu

EMPTY = lambda sizes: api.build_map_state(*sizes, [])      # noqa: E731   the 64-byte blob of 0 cells


def _centre_pose(sizes):
    xy, z, _ = sizes
    return pose(0.4, [xy * 0.3, xy * 0.6, z * 0.5])                            # somewhere in cell (0, 0, 0)


def _mixed_map(sizes, places, counts, **caps):
    """A map whose cells sit at the cell indices `places` with `counts` points, imported (slab 0); every third cell below capacity
    then takes one more point through liodom_map_update, in a leaf behind all of its leaves, which moves it to slab 1."""
    xy, z, res = sizes
    rng = np.random.default_rng(len(places))
    corners = [(kx * xy, ky * xy, kz * z) for kx, ky, kz in places]
    cells = [cell_points(rng, counts[i], corners[i], res) for i in range(len(places))]
    m = la.Map(xy, z, res, max_update_points=256, max_modified_cells=256, **caps)
    m.import_state(api.build_map_state(xy, z, res, cells))
    extra = [i for i in range(len(places)) if i % 3 == 1 and counts[i] < caps["cell_capacity"]]
    for lo in range(0, len(extra), 200):
        ids = extra[lo:lo + 200]
        x = np.zeros((len(ids), 4), np.float32)
        for r, i in enumerate(ids):
            x[r] = (corners[i][0] + res * 1.5, corners[i][1] + res * 1.5, corners[i][2] + res * 30.5, 500.0 + i)
            cells[i] = np.concatenate([cells[i], x[r:r + 1]])
        m.update(x)
    assert m.status() == 0 and m.export_state() == api.build_map_state(xy, z, res, cells)
    return m, cells


# ---------------------------------------------------------------------------------------------
# evict
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("name", CASES)
def test_evict_designed_maps(sizes, name):
    xy, z, res = sizes
    m, cells, removed = _designed_map(sizes, name)
    T = _centre_pose(sizes)
    blob, n = m.evict(T, KEEP, 0)
    gone = [c for i, c in enumerate(cells) if i in removed]
    kept = [c for i, c in enumerate(cells) if i not in removed]
    assert n == len(removed), name
    assert blob == api.build_map_state(xy, z, res, gone), name                 # the dropped cells, creation order, status 0
    after = m.export_state()
    assert after == api.build_map_state(xy, z, res, kept), name                # what liodom_map_prune would have left
    assert m.num_cells() == len(kept) and m.status() == 0
    blob2, n2 = m.evict(T, KEEP, 0)
    assert n2 == 0 and len(blob2) == 64 and blob2 == EMPTY(sizes) and m.export_state() == after
    if name == "all":                                                          # equals reset; and the map goes on working
        f = la.Map(xy, z, res, max_cells=8, cell_capacity=64)
        assert after == f.export_state()
        m.update(cells[0]); f.update(cells[0])
        assert m.export_state() == f.export_state() and m.num_cells() == 1
        f.close()
    m.close()


def test_evict_across_chunk_carries_and_a_full_cell():
    """2100 cells, every other one outside: more than 1024 dropped and more than 1024 kept, so the scan over the dropped cells
    (evict plan) and the one over the kept cells (prune plan) both carry from chunk to chunk.  Dropped cell 0 is at cell_capacity."""
    sizes = SIZES[0]
    xy, z, res = sizes
    n = 2100
    places = [(_outside(i // 2) if i % 2 == 0 else _inside(i // 2)) for i in range(n)]
    assert len(set(places)) == n
    counts = [64] + [1 + (7 * i) % 12 for i in range(1, n)]
    m, cells = _mixed_map(sizes, places, counts, max_cells=2200, cell_capacity=64)
    blob, n_ev = m.evict(_centre_pose(sizes), KEEP, 0)
    assert n_ev == 1050
    assert blob == api.build_map_state(xy, z, res, cells[0::2])
    assert m.export_state() == api.build_map_state(xy, z, res, cells[1::2])
    assert len(api.parse_map_state(blob)["cells"][0]) == 64
    m.close()


def test_evict_capacity_reply_leaves_buffer_and_map_untouched():
    sizes = SIZES[1]
    m, cells, removed = _designed_map(sizes, "alternating")
    before = m.export_state()
    L = la.load()
    T = np.ascontiguousarray(_centre_pose(sizes), np.float64).reshape(12)
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    want = api.build_map_state(*sizes, [c for i, c in enumerate(cells) if i in removed])
    need, n = C.c_int64(-1), C.c_int32(-1)
    assert L.liodom_map_evict(m.h, Tp, KEEP, 0, None, 0, C.byref(need), C.byref(n)) == api.ERR_CAPACITY      # the size query
    assert need.value == len(want) and m.export_state() == before
    buf = (C.c_ubyte * len(want))(*([0xAB] * len(want)))
    need.value = -1
    assert L.liodom_map_evict(m.h, Tp, KEEP, 0, buf, len(want) - 1, C.byref(need), C.byref(n)) == api.ERR_CAPACITY
    assert need.value == len(want) and bytes(buf) == b"\xab" * len(want) and m.export_state() == before
    assert L.liodom_map_evict(m.h, Tp, KEEP, 0, buf, len(want), C.byref(need), None) == 0                     # n_evicted is optional
    assert bytes(buf) == want and need.value == len(want)
    after = m.export_state()
    assert after != before
    # invalid arguments: nothing happens
    for args in ((None, Tp, 1, 1, buf, len(want), C.byref(need), None), (m.h, None, 1, 1, buf, len(want), C.byref(need), None),
                 (m.h, Tp, 1, 1, buf, len(want), None, None), (m.h, Tp, -1, 1, buf, len(want), C.byref(need), None),
                 (m.h, Tp, 1, -1, buf, len(want), C.byref(need), None)):
        assert L.liodom_map_evict(*args) == api.ERR_INVALID_ARG
    assert m.export_state() == after
    m.close()


# ---------------------------------------------------------------------------------------------
# merge
# ---------------------------------------------------------------------------------------------
def _tile(sizes, n, layer=3, seed=9, count=lambda i: 1 + (5 * i) % 11):
    """n cells in z layer `layer` (no designed map has cells there), walking a 64-wide grid."""
    xy, z, res = sizes
    rng = np.random.default_rng(seed + n)
    return [cell_points(rng, count(i), ((i % 64 - 32) * xy, (i // 64 - 8) * xy, layer * z), res) for i in range(n)]


@pytest.mark.parametrize("sizes", SIZES)
def test_merge_into_an_empty_map_equals_import(sizes):
    xy, z, res = sizes
    blob = api.build_map_state(xy, z, res, _tile(sizes, 70), status=8)
    a, b = (la.Map(xy, z, res, max_cells=96, cell_capacity=64) for _ in range(2))
    taken = a.merge_state(blob)
    b.import_state(blob)
    assert taken.dtype == np.int32 and taken.tolist() == [1] * 70
    assert a.export_state() == b.export_state() == blob and a.status() == 8
    x = PTS((-31.7 * xy, -7.7 * xy, 3.2 * z, 1.0), (50.3 * xy, 0.0, 0.0, 2.0))      # into the tile's first cell, and a new cell
    a.update(x); b.update(x)
    assert a.export_state() == b.export_state() and a.num_cells() == 71
    # a blob of 0 cells is a no-op
    before = a.export_state()
    assert a.merge_state(EMPTY(sizes)).shape == (0,) and a.export_state() == before
    a.close(); b.close()


@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1030])
def test_merge_appends_behind_a_designed_map(sizes, n):
    xy, z, res = sizes
    places = [_inside(i) for i in range(7)]
    m, cells = _mixed_map(sizes, places, [3 + i for i in range(7)], max_cells=1040, cell_capacity=64)
    tile = _tile(sizes, n)
    taken = m.merge_state(api.build_map_state(xy, z, res, tile))
    assert taken.tolist() == [1] * n and m.num_cells() == 7 + n and m.status() == 0
    assert m.export_state() == api.build_map_state(xy, z, res, cells + tile)
    for c in (tile[0], tile[-1], tile[n // 2], cells[1], cells[6]):            # found through the hash
        assert same(m.local(pose(0.0, [float(int(c[0, 0])), float(int(c[0, 1])), float(int(c[0, 2]))]), 0, 0)[:len(c)], c)
    m.close()


@pytest.mark.parametrize("sizes", SIZES)
def test_merge_onto_ids_a_prune_left_in_slab_1(sizes):
    """Cells 4 .. 7 are moved to slab 1 by an update, then pruned away: ids 4 .. 7 keep cell_buf = 1.  The merged cells get those
    ids; their points go to slab 0, so cell_buf has to be written."""
    xy, z, res = sizes
    rng = np.random.default_rng(8)
    base = [cell_points(rng, 4 + i, (i * xy, 0.0, 0.0), res) for i in range(4)] + [cell_points(rng, 6, ((30 + i) * xy, 0.0, 0.0), res) for i in range(4)]
    m = la.Map(xy, z, res, max_cells=8, cell_capacity=64, max_update_points=64, max_modified_cells=8)
    m.import_state(api.build_map_state(xy, z, res, base))
    m.update(PTS(*[((30 + i) * xy + res * 1.5, res * 1.5, res * 30.5, 9.0) for i in range(4)]))       # cells 4 .. 7 -> slab 1
    assert m.prune(pose(0.0, [1.0, 1.0, 1.0]), 5, 0) == 4
    tile = [cell_points(rng, 9 + i, (0.0, (2 + i) * xy, 0.0), res) for i in range(4)]
    assert m.merge_state(api.build_map_state(xy, z, res, tile)).tolist() == [1, 1, 1, 1]
    want = api.build_map_state(xy, z, res, base[:4] + tile)
    assert m.export_state() == want
    for c in tile:
        assert same(m.local(pose(0.0, [float(int(c[0, 0])), float(int(c[0, 1])), float(int(c[0, 2]))]), 0, 0)[:len(c)], c)
    # an update into a merged cell filters against the merged points: same leaf as its first point -> centroid of two, no new point
    f = la.Map(xy, z, res, max_cells=8, cell_capacity=64, max_update_points=64, max_modified_cells=8)
    f.import_state(want)
    x = tile[1][:1].copy(); x[0, :3] += res * 0.25; x[0, 3] = 77.0
    m.update(x); f.update(x)
    got = api.parse_map_state(m.export_state())
    assert m.export_state() == f.export_state() and got["counts"][5] == len(tile[1])
    assert np.array_equal(got["cells"][5][0], ((tile[1][0] + x[0]) / np.float32(2.0)).astype(np.float32))
    assert np.array_equal(got["cells"][5][1:], tile[1][1:])
    m.close(); f.close()


@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("hits", ["first", "last", "alternating"])
def test_merge_skips_the_keys_the_map_holds(sizes, hits):
    xy, z, res = sizes
    places = [_inside(i) for i in range(9)]
    m, cells = _mixed_map(sizes, places, [2 + i for i in range(9)], max_cells=32, cell_capacity=64)
    n = 11
    hit = {"first": [0], "last": [n - 1], "alternating": list(range(0, n, 2))}[hits]
    rng = np.random.default_rng(12)
    tile = _tile(sizes, n)
    for j, i in enumerate(hit):                                                # the tile's own version of device cells 1, 2, ...
        tile[i] = cell_points(rng, 20 + j, tuple(p * s for p, s in zip(places[1 + j], (xy, xy, z))), res)
    before = api.parse_map_state(m.export_state())
    taken = m.merge_state(api.build_map_state(xy, z, res, tile, status=4))
    assert taken.tolist() == [0 if i in hit else 1 for i in range(n)]
    assert m.export_state() == api.build_map_state(xy, z, res, cells + [t for i, t in enumerate(tile) if i not in hit], status=4)
    after = api.parse_map_state(m.export_state())
    assert all(same(a, b) for a, b in zip(before["cells"], after["cells"]))   # the colliding device cells are as they were
    assert m.status() == 4
    m.close()


def test_merge_rejections_leave_the_map_untouched():
    sizes = SIZES[1]
    xy, z, res = sizes
    m, cells = _mixed_map(sizes, [_inside(i) for i in range(6)], [3] * 6, max_cells=8, cell_capacity=64)
    before = m.export_state()
    good = api.build_map_state(xy, z, res, _tile(sizes, 2))

    def code(blob):
        with pytest.raises(la.LiodomError) as ei:
            m.merge_state(blob)
        assert m.export_state() == before
        return ei.value.code

    # not enough free ids: 6 + 3 > 8 ...
    three = _tile(sizes, 3)
    assert code(api.build_map_state(xy, z, res, three)) == api.ERR_CAPACITY
    assert code(api.build_map_state(xy, z, res, _tile(sizes, 9))) == api.ERR_CAPACITY                  # more cells than max_cells
    assert code(api.build_map_state(xy, z, res, [cell_points(np.random.default_rng(1), 65, (0.0, 0.0, 3 * z), res)])) == api.ERR_CAPACITY
    for bad in (b"", good[:63], good[:-1], good + b"\0" * 16, b"LIODOMST" + good[8:], api.build_map_state(xy, z, 0.5, _tile(sizes, 1)),
                api.build_map_state(xy, 25.0, res, [])):
        assert code(bad) == api.ERR_INVALID_ARG
    L = la.load()
    assert L.liodom_map_merge_state(None, good, len(good), None, None) == api.ERR_INVALID_ARG
    assert L.liodom_map_merge_state(m.h, None, len(good), None, None) == api.ERR_INVALID_ARG
    assert m.export_state() == before
    # ... but with one of the three already there the other two fit exactly
    three[1] = cells[2] + np.float32(0.01)
    assert m.merge_state(api.build_map_state(xy, z, res, three)).tolist() == [1, 0, 1] and m.num_cells() == 8
    assert m.export_state() == api.build_map_state(xy, z, res, cells + [three[0], three[2]])
    n = C.c_int32(-1)
    assert L.liodom_map_merge_state(m.h, good, len(good), None, C.byref(n)) == api.ERR_CAPACITY       # taken is optional
    m.close()


def test_merge_takes_over_slots_an_overfull_update_left_behind():
    """One update that touches more new cells than it can create (kMapNewCellsMax = 256) leaves the keys of the others in the cell
    hash without a cell.  Such a key is not a cell of the map: a merge takes it, through the slot it already has."""
    sizes = SIZES[1]
    xy, z, res = sizes
    line = PTS(*[(xy * i + 5.0, 5.0, 5.0, float(i)) for i in range(300)])
    m = la.Map(xy, z, res, max_cells=400, cell_capacity=64, max_update_points=512, max_modified_cells=256)
    m.update(line)
    assert m.status() & 2 and m.num_cells() == 256
    have = set(tuple(int(q) for q in k) for k in api.parse_map_state(m.export_state())["keys"])
    stuck = [i for i in range(300) if tuple(api.map_cell_key(line[i, :3], xy, z)) not in have]
    assert len(stuck) == 44
    m.update(line[stuck[0]:stuck[0] + 1])
    assert m.num_cells() == 256                                                # the key sits in the hash, no cell can be created for it
    rng = np.random.default_rng(3)
    tile = [cell_points(rng, 5, (xy * stuck[0], 0.0, 0.0), res), cell_points(rng, 6, (xy * 1000, 0.0, 0.0), res), cell_points(rng, 7, (xy * stuck[-1], 0.0, 0.0), res)]
    before = api.parse_map_state(m.export_state())
    assert m.merge_state(api.build_map_state(xy, z, res, tile)).tolist() == [1, 1, 1] and m.num_cells() == 259
    want = api.build_map_state(xy, z, res, list(before["cells"]) + tile, status=m.status())
    assert m.export_state() == want
    for c in tile:
        assert same(m.local(pose(0.0, [float(int(c[0, 0])), float(int(c[0, 1])), float(int(c[0, 2]))]), 0, 0)[:len(c)], c)
    f = la.Map(xy, z, res, max_cells=400, cell_capacity=64, max_update_points=512, max_modified_cells=256)
    f.import_state(want)
    x = PTS((xy * stuck[0] + 7.0, 7.0, 7.0, 1.0), (xy * stuck[-1] + 7.0, 7.0, 7.0, 2.0), (xy * stuck[1] + 7.0, 7.0, 7.0, 3.0))
    m.update(x); f.update(x)
    got, ref = api.parse_map_state(m.export_state()), api.parse_map_state(f.export_state())
    # the two merged cells took their points; stuck[1]'s key is still without a cell here, while the imported twin (a rebuilt
    # hash) creates it
    assert m.num_cells() == 259 and f.num_cells() == 260
    assert all(same(a, b) for a, b in zip(got["cells"], ref["cells"][:259]))
    assert len(got["cells"][256]) == 6 and len(got["cells"][258]) == 8
    m.close(); f.close()


# ---------------------------------------------------------------------------------------------
# round trip and continuation
# ---------------------------------------------------------------------------------------------
def _by_key(m):
    return mm.by_key(mm.state_of(m.export_state()))


def test_evict_merge_back_and_continue_like_a_map_never_evicted():
    sizes = SIZES[0]
    xy, z, res = sizes
    caps = dict(max_cells=512, cell_capacity=8192, max_update_points=1024, max_modified_cells=128)
    rng = np.random.default_rng(21)
    ups = [clustered_update(rng, k, res) for k in range(18)]
    m, f = la.Map(xy, z, res, **caps), la.Map(xy, z, res, **caps)
    for x, T in ups[:8]:
        m.update(x, T); f.update(x, T)
    T = pose(0.1, [3.0, -2.0, 0.5])
    blob, n = m.evict(T, 1, 0)
    tile = mm.state_of(blob, sizes)
    kept_keys = set(_by_key(m))
    assert n > 2 and len(kept_keys) > 2 and m.num_cells() == f.num_cells() - n
    assert m.merge_state(blob).tolist() == [1] * n
    assert _by_key(m) == _by_key(f)
    start = _by_key(f)
    for k, (x, Tk) in enumerate(ups[8:]):
        m.update(x, Tk); f.update(x, Tk)
        assert m.num_cells() == f.num_cells() and m.status() == f.status() == 0, k
        for Tq in (Tk, T, pose(0.0, [-9.0, 11.0, 1.0])):
            assert same(m.local(Tq, 2, 1), f.local(Tq, 2, 1)) and same(m.local(Tq, 1, 0), f.local(Tq, 1, 0)), k
    end = _by_key(m)
    assert end == _by_key(f)
    changed = {k for k in start if end[k] != start[k]}
    assert changed & set(tile["keys"]) and changed & kept_keys and set(end) - set(start)       # a merged, a kept and a new cell were touched
    m.close(); f.close()


# ---------------------------------------------------------------------------------------------
# the pager on a live handle: a paged run equals the unbounded run
# ---------------------------------------------------------------------------------------------
# A circle of radius 30 m, 1 m and 1.91 deg per scan (188 scans a lap), 225 scans: the run comes back to where it began.  The CPU
# oracle's lagged loop holds this circle (per-scan translation <= 1.06 m, 3.3 m off the ground truth at worst).
SPEED, YAW_RATE, N_SCANS = 1.0, 1.91, 225
MAX_RANGE = 40.0                    # horizontal, as the extractor filters; 41.5 m along a beam 15 degrees up
STEP_BOUND = 1.1                    # per-scan translation the derivation assumes; asserted on the unbounded run
RUN_SZ = (12.0, 50.0, 0.4)
CELLS_XY, CELLS_Z = 3, 1
RUN_CAPS = dict(cell_capacity=4096, max_modified_cells=256)


def _load_xy(period):
    """max_range + window travel of the lagged frame + travel per pager period + 1 m + one cell."""
    need = MAX_RANGE + P * STEP_BOUND + (period * STEP_BOUND + 1.0) + RUN_SZ[0]
    return max(int(np.ceil(need / RUN_SZ[0])), CELLS_XY + 1)


LOAD_Z = 2                          # 41.5 sin(15 deg) + 0.2 (z travel) + 1 + 50 = 62 <= 2 * 50; and 2 * 50 >= CELLS_Z * 12
_RUN = {}


def _circle_scans(synth):
    if "scans" not in _RUN:
        cfg = synth.make_cfg(H, W, 0, yaw_rate_deg=YAW_RATE, speed=SPEED)
        _RUN["scans"] = [synth.scan(cfg, 0, k)[0] for k in range(N_SCANS)]
    return _RUN["scans"]


def _run_handle():
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1, max_range=MAX_RANGE),
                     la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))


def _unbounded_run(synth):
    """Handle A: an unbounded map, no pruning.  Computed once, shared by both paged runs."""
    if "A" not in _RUN:
        g, m = _run_handle(), la.Map(*RUN_SZ, max_cells=512, **RUN_CAPS)
        g.attach_mapper(m, CELLS_XY, CELLS_Z, lag=1)
        out = []
        for x in _circle_scans(synth):
            p, info = g.process_scan(x, H, W)
            out.append((p.copy(), g.received_map(), [info.lm[i].termination for i in (0, 1)]))
        _RUN["A"] = dict(scans=out, cells=m.num_cells(), state=mm.state_of(m.export_state()), status=m.status())
        g.attach_mapper(None)
        g.close(); m.close()
    return _RUN["A"]


@pytest.mark.parametrize("period", [1, 3])
def test_paged_run_equals_the_unbounded_run(synth, period):
    A = _unbounded_run(synth)
    load_xy = _load_xy(period)
    assert (period, load_xy) in ((1, 5), (3, 6)) and CELLS_XY + 1 <= load_xy <= CELLS_XY + 3
    keep_xy = load_xy + (1 if period == 1 else 0)                              # with and without hysteresis
    # premises of the comparison
    steps = [float(np.linalg.norm(A["scans"][k][0][4:] - A["scans"][k - 1][0][4:])) for k in range(1, N_SCANS)]
    assert max(steps) <= STEP_BOUND and A["status"] == 0
    assert max(len(r) for _, r, _ in A["scans"]) < (1 << 16) and len(A["scans"][-1][1]) > 1000
    g, m = _run_handle(), la.Map(*RUN_SZ, max_cells=320, **RUN_CAPS)
    g.attach_mapper(m, CELLS_XY, CELLS_Z, lag=1)
    pg = MapPager(m, keep_xy, LOAD_Z, load_xy, LOAD_Z)
    ever_evicted, reloaded, max_cells = set(), set(), 0
    for k, x in enumerate(_circle_scans(synth)):
        p, info = g.process_scan(x, H, W)
        pa, ra, ta = A["scans"][k]
        assert np.array_equal(p, pa), k
        assert same(g.received_map(), ra), k
        assert [info.lm[i].termination for i in (0, 1)] == ta, k
        max_cells = max(max_cells, m.num_cells())
        if (k + 1) % period == 0:
            T = T_of(p)
            pg.step(T)
            c = pg.centre(T)
            assert not any(pg.in_box(key, c, load_xy, LOAD_Z) for key in pg.last_evicted), k      # every evicted key is outside the load box
            reloaded |= set(pg.last_loaded) & ever_evicted
            ever_evicted |= set(pg.last_evicted)
    print("period %d: load_xy %d keep_xy %d, max step %.3f m, evicted %d loaded %d (%d of them evicted earlier) conflicts %d, cells max %d (unbounded %d), stored %d" % (
        period, load_xy, keep_xy, max(steps), pg.evicted, pg.loaded, len(reloaded), pg.conflicts, max_cells, A["cells"], len(pg.store)))
    assert pg.conflicts == 0 and m.status() == 0
    assert pg.evicted > 0 and pg.loaded > 0 and reloaded                       # the run did come back to cells it had left
    assert max_cells < A["cells"]
    assert mm.by_key(mm.state_of(pg.export_all(), RUN_SZ)) == mm.by_key(A["state"])
    g.attach_mapper(None)
    g.close(); m.close()


def test_forced_conflict_is_resolved_by_reobserving_the_stored_cell():
    sizes = SIZES[0]
    xy, z, res = sizes
    caps = dict(max_cells=64, cell_capacity=1024, max_update_points=64, max_modified_cells=16)
    rng = np.random.default_rng(5)
    near = np.concatenate([cell_points(rng, 20, (i * xy, 0.0, 0.0), res) for i in range(3)])
    far = cell_points(rng, 150, (20 * xy, 0.0, 0.0), res)                     # more than two chunks of max_update_points
    far[:, :3] += rng.uniform(0, res * 0.2, (150, 3)).astype(np.float32)
    fresh = cell_points(rng, 30, (20 * xy, 0.0, 0.0), res)
    fresh[:15] += np.float32(res * 0.3)                                        # 15 points in leaves the stored cell holds too,
    fresh[15:] += np.float32(res)                                              # 15 in leaves of their own
    T0, Tfar = pose(0.0, [1.0, 1.0, 1.0]), pose(0.0, [20 * xy + 1.0, 1.0, 1.0])
    m, f = la.Map(xy, z, res, **caps), la.Map(xy, z, res, **caps)
    for mp in (m, f):
        mp.update(near)
        for lo in range(0, 150, 64):
            mp.update(far[lo:lo + 64])
    pg = MapPager(m, 2, 0, 1, 0)
    assert pg.step(T0) == (1, 0) and len(pg.store) == 1
    stored = next(iter(pg.store.values()))[1].copy()
    blob, n = f.evict(T0, 2, 0)                                                # the twin: the same steps by hand
    assert n == 1 and same(api.parse_map_state(blob)["cells"][0], stored)
    m.update(fresh); f.update(fresh)                                           # the device re-creates the stored key
    pg.step(Tfar)
    assert f.prune(Tfar, 2, 0) == 3
    for lo in range(0, len(stored), 64):
        f.update(stored[lo:lo + 64], np.eye(4)[:3])
    assert pg.conflicts == 1 and pg.loaded == 0 and pg.evicted == 4 and len(pg.store) == 3
    assert _by_key(m) == _by_key(f) and m.num_cells() == 1 and m.status() == 0
    assert len(api.parse_map_state(m.export_state())["cells"][0]) == 165       # 150 stored leaves + the 15 new ones
    m.close(); f.close()


# ---------------------------------------------------------------------------------------------
# host mirror: liodom::MapPager behind liodom_replay map_pager=
# ---------------------------------------------------------------------------------------------
def test_replay_with_the_pager_writes_the_same_poses_and_the_whole_map(synth, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "liodom_amd", "host", "liodom_replay")
    assert os.path.exists(exe), "liodom_replay not built (run __graft_entry__.build())"
    scans = _circle_scans(synth)
    scan_dir = tmp_path / "scans"
    scan_dir.mkdir()
    for k, x in enumerate(scans):
        x.astype(np.float32).tofile(str(scan_dir / ("%06d.bin" % k)))
    load_xy = _load_xy(1)
    common = ["scan_lines=%d" % H, "scan_regions=%d" % R, "edges_per_region=%d" % EPR, "prev_frames=%d" % P, "max_range=%g" % MAX_RANGE,
              "mapping=true", "voxel_xysize=%g" % RUN_SZ[0], "voxel_zsize=%g" % RUN_SZ[1], "resolution=%g" % RUN_SZ[2],
              "cells_xy=%d" % CELLS_XY, "cells_z=%d" % CELLS_Z, "mapper_lag=1"]
    out = {}
    for name, more in (("plain", []), ("paged", ["map_pager=%d,%d,%d,%d" % (load_xy + 1, LOAD_Z, load_xy, LOAD_Z)])):
        od = tmp_path / name
        od.mkdir()
        r = subprocess.run([exe, str(scan_dir), str(od) + "/"] + common + more + ["map_state_out=" + str(od / "map.state")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[name] = ((od / "poses.txt").read_bytes(), mm.state_of((od / "map.state").read_bytes(), RUN_SZ), r.stdout)
    assert out["plain"][0] == out["paged"][0] and len(out["plain"][0].splitlines()) == N_SCANS
    assert "pager:" in out["paged"][2] and " 0 conflicts" in out["paged"][2]
    # the Python pager on the same run
    g, m = _run_handle(), la.Map(*RUN_SZ, max_cells=320, **RUN_CAPS)
    g.attach_mapper(m, CELLS_XY, CELLS_Z, lag=1)
    pg = MapPager(m, load_xy + 1, LOAD_Z, load_xy, LOAD_Z)
    for x in scans:
        pg.step(T_of(g.process_scan(x, H, W)[0]))
    want = mm.by_key(mm.state_of(pg.export_all(), RUN_SZ))
    assert pg.evicted > 0 and pg.loaded > 0
    assert mm.by_key(out["paged"][1]) == want == mm.by_key(out["plain"][1])
    g.attach_mapper(None)
    g.close(); m.close()
