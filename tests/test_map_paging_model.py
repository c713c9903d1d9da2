"""Paging without a device: api.join_map_state, the pure-Python model of evict / merge (map_paging_model.py) and
liodom_amd.pager.MapPager on a fake Map built on that model — hysteresis, the conflict rule and its counter, export_all."""
import numpy as np
import pytest

from liodom_amd import api
from liodom_amd.pager import MapPager
import map_paging_model as mm

SIZES = [(10.0, 10.0, 0.25), (40.0, 50.0, 0.4)]


def cell_at(idx, sizes, n=3, tag=0.0):
    """n points of the cell with cell indices idx (one per leaf)."""
    xy, z, res = sizes
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = idx[0] * xy + res * (1.5 + 3 * np.arange(n))
    p[:, 1] = idx[1] * xy + res * 1.5
    p[:, 2] = idx[2] * z + res * 1.5
    p[:, 3] = tag + np.arange(n)
    return p


def pose_at(idx, sizes, frac=0.4):
    T = np.eye(4)[:3].copy()
    T[:, 3] = [(idx[0] + frac) * sizes[0], (idx[1] + frac) * sizes[0], (idx[2] + frac) * sizes[1]]
    return T


def line_blob(sizes, lo, hi, n=3):
    """Cells lo .. hi - 1 along x."""
    xy, z, res = sizes
    return api.build_map_state(xy, z, res, [cell_at((i, 0, 0), sizes, n + i % 3, 10.0 * i) for i in range(lo, hi)])


@pytest.mark.parametrize("sizes", SIZES)
def test_join_after_parse_is_the_identity(sizes):
    xy, z, res = sizes
    rng = np.random.default_rng(5)
    cells = [cell_at((int(i), int(j), int(k)), sizes, int(n)) for i, j, k, n in
             zip(rng.permutation(40) - 20, rng.integers(-9, 9, 40), rng.integers(-2, 2, 40), rng.integers(1, 9, 40))]
    for cs, status in ((cells, 0), (cells[:1], 8), ([], 0), ([], 66)):
        blob = api.build_map_state(xy, z, res, cs, status=status)
        st = api.parse_map_state(blob, sizes=sizes)
        assert api.join_map_state(xy, z, res, st["keys"], st["corner_leaf"], st["cells"], status=st["status"]) == blob
        assert mm.blob_of(mm.state_of(blob, sizes), sizes) == blob
    with pytest.raises(ValueError):
        api.join_map_state(xy, z, res, [(0, 0, 0)], [], [])
    # corner_leaf travels as given: it is not re-derived from the points
    odd = api.join_map_state(xy, z, res, [(5, 5, 5)], [(7, -7, 70)], [cells[0]])
    assert [tuple(r) for r in api.parse_map_state(odd)["corner_leaf"]] == [(7, -7, 70)]
    # an empty cell is a legal record
    st = api.parse_map_state(api.join_map_state(xy, z, res, [(5, 5, 5), (15, 5, 5)], [(0, 0, 0), (1, 1, 1)], [np.zeros((0, 4)), cells[0]]))
    assert list(st["counts"]) == [0, len(cells[0])]


@pytest.mark.parametrize("sizes", SIZES)
def test_model_keep_rule_order_and_taken_flags(sizes):
    xy, z, res = sizes
    full = mm.state_of(line_blob(sizes, -6, 7), sizes)
    full["status"] = 8
    T = pose_at((1, 0, 0), sizes)
    kept, removed = mm.evict(full, T, sizes, 2, 0)
    want_kept = [k for k in full["keys"] if abs(k[0] - mm.centre_cell(T, sizes)[0]) <= 2 * xy]
    assert kept["keys"] == want_kept and len(want_kept) == 5
    assert removed["keys"] == [k for k in full["keys"] if k not in want_kept]              # relative creation order
    assert kept["status"] == 8 and removed["status"] == 0
    # truncation toward zero first: -0.5 is cell 0
    T0 = np.eye(4)[:3].copy(); T0[0, 3] = -0.5
    assert mm.centre_cell(T0, sizes) == api.map_cell_key([0.0, 0.0, 0.0], xy, z)
    # evict then merge back: kept ++ removed
    merged, taken = mm.merge(kept, removed)
    assert taken.tolist() == [1] * len(removed["keys"])
    assert merged["keys"] == kept["keys"] + removed["keys"] and merged["status"] == 8
    assert mm.by_key(merged) == mm.by_key(full)
    assert mm.blob_of(merged, sizes) == api.join_map_state(xy, z, res, kept["keys"] + removed["keys"], kept["corner_leaf"] + removed["corner_leaf"],
                                                           kept["cells"] + removed["cells"], status=8)
    # collisions: first, last, alternating
    for hit in ([0], [len(full["keys"]) - 1], list(range(0, len(full["keys"]), 2))):
        have = mm._pick(full, hit, 0)
        have["cells"] = [c + 1.0 for c in have["cells"]]                                   # the map's version differs from the tile's
        merged, taken = mm.merge(have, full)
        assert taken.tolist() == [0 if i in hit else 1 for i in range(len(full["keys"]))]
        assert merged["keys"] == have["keys"] + [k for i, k in enumerate(full["keys"]) if i not in hit]
        assert all(np.array_equal(a, b) for a, b in zip(merged["cells"][:len(hit)], have["cells"]))
    # capacity: map untouched
    assert mm.merge(kept, removed, max_cells=len(full["keys"]) - 1)[0] is None
    assert mm.merge(kept, mm.empty_state())[0] is kept


def test_pager_argument_check():
    m = mm.FakeMap(10.0, 10.0, 0.25)
    for bad in ((1, 1, 2, 1), (2, 0, 2, 1), (-1, 0, -1, 0)):
        with pytest.raises(ValueError):
            MapPager(m, *bad)
    MapPager(m, 2, 1, 2, 1)


@pytest.mark.parametrize("sizes", SIZES)
def test_pager_pages_out_and_back_without_loss(sizes):
    m = mm.FakeMap(*sizes)
    m.import_state(line_blob(sizes, -8, 9))
    full = mm.by_key(m.state)
    pg = MapPager(m, 2, 0, 1, 0)
    assert pg.step(pose_at((0, 0, 0), sizes)) == (12, 0)
    assert m.num_cells() == 5 and len(pg.store) == 12 and pg.evicted == 12 and pg.loaded == 0
    assert mm.by_key(mm.state_of(pg.export_all(), sizes)) == full
    # export_all: device cells first
    assert mm.state_of(pg.export_all(), sizes)["keys"] == m.state["keys"] + list(pg.store)
    # drive to the far end and back: every cell is seen again exactly as it was left
    for i in list(range(1, 9)) + list(range(7, -9, -1)):
        pg.step(pose_at((i, 0, 0), sizes))
        assert m.num_cells() <= 5 and mm.by_key(mm.state_of(pg.export_all(), sizes)) == full
        c = mm.centre_cell(pose_at((i, 0, 0), sizes), sizes)
        assert all(mm.keeps(k, c, sizes, 2, 0) for k in m.state["keys"])
        assert not any(mm.keeps(k, c, sizes, 1, 0) for k in pg.store)                      # everything inside the load box is on the device
        assert all(not mm.keeps(k, c, sizes, 1, 0) for k in pg.last_evicted)
    assert pg.conflicts == 0 and pg.loaded > 10 and pg.evicted - pg.loaded == len(pg.store)
    assert len(pg.store) + m.num_cells() == len(full)


@pytest.mark.parametrize("sizes", SIZES)
def test_hysteresis_keep_above_load_does_not_thrash(sizes):
    """The pose oscillates across one cell border.  With keep = load every crossing moves cells; with keep = load + 1 only the
    first crossing does."""
    moved = {}
    for keep in (1, 2):
        m = mm.FakeMap(*sizes)
        m.import_state(line_blob(sizes, -8, 9))
        pg = MapPager(m, keep, 0, 1, 0)
        pg.step(pose_at((0, 0, 0), sizes))
        e0, l0 = pg.evicted, pg.loaded
        for k in range(10):
            pg.step(pose_at((k % 2, 0, 0), sizes, frac=0.02 if k % 2 else 0.98))
        moved[keep] = (pg.evicted - e0, pg.loaded - l0)
        assert pg.conflicts == 0
    assert moved[1][0] >= 9 and moved[1][1] >= 9
    assert moved[2] == (1, 0)                    # the first crossing drops the cell behind; nothing is ever loaded


@pytest.mark.parametrize("sizes", SIZES)
def test_conflicts_are_counted_and_resolved_by_reobserving(sizes):
    xy, z, res = sizes
    m = mm.FakeMap(*sizes, max_update_points=4)
    m.import_state(line_blob(sizes, 0, 8, n=5))
    pg = MapPager(m, 1, 0, 1, 0)
    pg.step(pose_at((0, 0, 0), sizes))
    assert sorted(k[0] for k in pg.store) == sorted(api.map_cell_key([i * xy + 0.1, 0.1, 0.1], xy, z)[0] for i in range(2, 8))
    # 1. the device re-creates a stored key inside the load box of the next step: the merge reports taken = 0
    fresh = cell_at((3, 0, 0), sizes, 2, 900.0)
    key3 = tuple(api.map_cell_key(fresh[0, :3], xy, z))
    stored3 = pg.store[key3][1].copy()
    assert len(stored3) > 4                                                                # more than one chunk of max_update_points
    m.update(fresh)
    m.calls.clear()
    pg.step(pose_at((3, 0, 0), sizes))
    assert pg.conflicts == 1 and key3 not in pg.store
    i = m.state["keys"].index(key3)
    assert np.array_equal(m.state["cells"][i], np.concatenate([fresh, stored3]))           # re-observed behind the device's points
    assert [c for c in m.calls if c[0] == "update"] == [("update", 4), ("update", len(stored3) - 4)]
    # 2. the device re-creates a stored key OUTSIDE the keep box: it is evicted onto a stored cell
    fresh7 = cell_at((7, 0, 0), sizes, 2, 700.0)
    key7 = tuple(api.map_cell_key(fresh7[0, :3], xy, z))
    stored7 = pg.store[key7][1].copy()
    m.update(fresh7)
    pg.step(pose_at((3, 0, 0), sizes))
    assert pg.conflicts == 2 and key7 not in pg.store
    i = m.state["keys"].index(key7)
    assert np.array_equal(m.state["cells"][i], np.concatenate([fresh7, stored7]))
    pg.step(pose_at((3, 0, 0), sizes))                                                     # ... and leaves with the next step, once
    assert pg.conflicts == 2 and key7 in pg.store and key7 not in m.state["keys"]
    assert np.array_equal(pg.store[key7][1], np.concatenate([fresh7, stored7]))
    # nothing is lost or doubled
    st = mm.state_of(pg.export_all(), sizes)
    assert len(set(st["keys"])) == len(st["keys"]) == 8
    assert sum(len(c) for c in st["cells"]) == sum(5 + i % 3 for i in range(8)) + 4


@pytest.mark.parametrize("sizes", SIZES)
def test_a_saved_map_larger_than_the_device_map_is_paged_in(sizes):
    site = line_blob(sizes, -20, 21)
    m = mm.FakeMap(*sizes, max_cells=7)
    pg = MapPager(m, 3, 0, 2, 0)
    pg.store_state(site)
    assert m.num_cells() == 0 and len(pg.store) == 41
    with pytest.raises(ValueError):
        pg.store_state(site)
    for i in (0, 1, 5, 18, 20, -20):
        pg.step(pose_at((i, 0, 0), sizes))
        c = mm.centre_cell(pose_at((i, 0, 0), sizes), sizes)
        assert 3 <= m.num_cells() <= 7 and all(mm.keeps(k, c, sizes, 3, 0) for k in m.state["keys"])
        assert sum(mm.keeps(k, c, sizes, 2, 0) for k in m.state["keys"]) == min(5, 3 + min(20 - i, 20 + i))
    assert pg.conflicts == 0 and mm.by_key(mm.state_of(pg.export_all(), sizes)) == mm.by_key(mm.state_of(site, sizes))
