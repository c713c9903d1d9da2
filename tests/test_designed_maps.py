"""The conditions of tests/designed_maps.py, asserted on the CPU oracle (orc.Map) and on the NumPy restatement alone, so that no
case of tests/test_gpu_designed_map.py passes by being empty: the two statements of an update agree bit for bit on every world,
and every world reaches what it was designed to reach.  CPU only."""
import numpy as np
import pytest

import designed_maps as dm
from liodom_amd import api


def run_both(orc, w, updates=None):
    """Feeds the world to the oracle and to the restatement, comparing after every update; returns the restatement and its
    per-update counts."""
    mo, mr = orc.Map(*w["sizes"]), dm.Restated(*w["sizes"])
    stats = []
    for k, (pts, T) in enumerate(w["updates"] if updates is None else updates):
        mo.update(pts, T)
        stats.append(mr.update(pts, T))
        assert mr.num_cells() == mo.num_cells(), (w["name"], k)
        assert dm.same_bits(mr.all(), mo.all()), (w["name"], k)
    return mr, stats


@pytest.mark.parametrize("name", list(dm.WORLDS))
def test_oracle_and_restatement_agree_bit_for_bit(orc, name):
    w = dm.world(name)
    updates = w["updates"]
    if name == "far":       # the reference has no key range: the flagged points are fed to neither (the device drops them)
        pts, T = updates[-1]
        assert 50 <= int(w["out_of_range"].sum()) < len(pts) - 50
        updates = updates[:-1] + [(pts[~w["out_of_range"]], T)]
    mr, stats = run_both(orc, w, updates)
    assert mr.num_cells() > 0 and sum(st["n_multi"] for st in stats) > 0
    # the capacities a world states are the smallest that hold it (brim and many_cells state theirs: checked below)
    if name not in ("brim", "many_cells"):
        got = dm.reached(w, updates)
        assert {k: got[k] for k in w["caps"]} == w["caps"], (got, w["caps"])


@pytest.mark.parametrize("origin", dm.CROWDED_ORIGINS)
def test_crowded_member_counts_and_summation_order(orc, origin):
    """Every listed member count occurs, without and with an old centroid at the head of the sum, and the order of the float32
    additions decides the bits: for at least half of the leaves with 33 or more members, summing the members in reverse order
    changes the centroid in some channel.  (Measured: 21 of 21 such leaves at the origin, 20 of 21 at 1000 m — the 1000 m
    placement reaches the bar as well, so one bar serves both.)"""
    w = dm.crowded(origin)
    mr, stats = run_both(orc, w)
    fresh = sorted(len(lv["members"]) for lv in stats[0]["leaves"])
    assert fresh == sorted(dm.CROWDED_COUNTS) and all(lv["n_old"] == 0 for lv in stats[0]["leaves"])
    assert stats[1]["max_members"] == dm.CROWDED_FULL + 1 and stats[1]["n_points"] == w["caps"]["max_update_points"]
    for st in stats[2:]:
        assert sorted(len(lv["members"]) for lv in st["leaves"]) == sorted(dm.CROWDED_COUNTS)
    assert len(stats) == 5 and mr.num_cells() == 2
    # both cells and all their leaves take part in every update; the input order interleaves them
    pts = w["updates"][0][0]
    cell_of = dm.cell_keys(pts, w["sizes"])[:, 0]
    leaf_of = dm.leaf_coords(pts, w["sizes"][2])[:, 2]
    assert (np.diff(cell_of[:200]) != 0).sum() > 50 and (np.diff(leaf_of[:200]) != 0).sum() > 50
    assert float(pts[:, 3].min()) >= 0.0 and float(pts[:, 3].max()) <= 100.0
    big, moved = 0, 0
    for st in stats:
        for lv in st["leaves"]:
            if len(lv["members"]) >= 33:
                big += 1
                moved += 0 if dm.same_bits(dm.leaf_centroid(lv["members"]), dm.leaf_centroid(lv["members"][::-1])) else 1
    print("crowded %s: %d of %d leaves with >= 33 members change bits under the reverse order" % (origin, moved, big))
    assert big >= 20 and 2 * moved >= big, (moved, big)


def test_crowded_old_centroid_heads_the_sum(orc):
    w = dm.world("crowded-0")
    mr = dm.Restated(*w["sizes"])
    for k, (pts, T) in enumerate(w["updates"]):
        before = [c.copy() for c in mr.clouds]
        st = mr.update(pts, T)
        if k == 0:
            continue
        for lv in st["leaves"]:
            assert lv["n_old"] == 4 and (len(lv["members"]) >= 2 or k == 1)      # (update 1 feeds one leaf of one cell)
            assert dm.same_bits(lv["members"][0], before[lv["cell"]][lv["pos"]])      # ... and it stayed in its leaf


@pytest.mark.parametrize("sizes", dm.FACES_SIZES)
def test_faces_have_points_on_and_beside_them(orc, sizes):
    xy, z, res = sizes
    w = dm.faces(sizes)
    mr, stats = run_both(orc, w)
    pts = w["updates"][0][0]
    assert len(w["faces"]) >= 3 * 13
    for a, below, on, above in w["faces"]:
        col = pts[:, a]
        assert np.float32(below) < np.float32(on) < np.float32(above)
        assert np.nextafter(np.float32(on), np.float32(-np.inf)) == np.float32(below) and np.nextafter(np.float32(on), np.float32(np.inf)) == np.float32(above)
        for v in (below, on, above):
            assert (col == np.float32(v)).any(), (a, v)
    for a, size in enumerate((xy, xy, z)):
        on = {f[2] for f in w["faces"] if f[0] == a}
        assert {float(np.float32(k * res)) for k in range(-3, 4)} <= on and {float(np.float32(k * size)) for k in range(-2, 3)} <= on
        assert float(np.float32((int(round(size / res)) - 1) * res)) in on          # the last leaf below the cell's upper corner
        col = pts[:, a].view(np.uint32)
        assert (col == 0).any() and (col == 0x80000000).any() and (col == 0x80000001).any()      # +0.0, -0.0, the negative denormal
    keys = np.array(mr.keys)
    assert (keys < 0).any(axis=0).all() and (keys > 0).any(axis=0).all()
    # the faces separate: more than one cell and more than one leaf along every axis, and update 1 doubles every leaf
    assert all(len(set(keys[:, a])) >= 5 for a in range(3))
    assert all(len(lv["members"]) >= 2 for lv in stats[1]["leaves"]) and len(stats[1]["modified"]) == mr.num_cells()
    # the two ends of cell (0, 0, 0)'s leaf bitmap: its lowest and its highest leaf.  In the device's dense grid (margin of 2
    # leaves on every side, 32 leaves to a word) they lie in the first and in the last round of 4096 words of the prefix kernel.
    lo, hi = dm.leaf_coords(w["ends"], res)
    assert list(dm.cell_keys(w["ends"], sizes)[0]) == list(dm.cell_keys(w["ends"], sizes)[1]) == api.map_cell_key([1.0, 1.0, 1.0], xy, z)
    assert list(lo) == [0, 0, 0] and all(hi[a] >= int(np.floor(s / res)) - 1 for a, s in enumerate((xy, xy, z)))
    inv = np.float32(1.0) / np.float32(res)
    gx = int(np.ceil(np.float32(xy) * inv)) + 5
    gz = int(np.ceil(np.float32(z) * inv)) + 5
    words = (gx * gx * gz + 31) // 32
    word_of = lambda lf: ((lf[0] + 2) + (lf[1] + 2) * gx + (lf[2] + 2) * gx * gx) // 32      # noqa: E731
    assert word_of(lo) < 4096 and word_of(hi) // 4096 == (words - 1) // 4096
    if sizes == dm.FACES_SIZES[2]:
        assert words > 4096          # the prefix kernel loops


def test_far_reaches_a_million_metres_on_either_side(orc):
    w = dm.world("far")
    worlds = [dm.transform(p, T) for p, T in w["updates"]]
    allp = np.concatenate(worlds[:3])[:, :3]
    assert allp.max() >= 1.0e6 and allp.min() <= -1.0e6
    assert np.abs(np.array(dm.cell_keys(np.concatenate(worlds[:3]), w["sizes"]))).max() < dm.KEY_LIMIT
    assert np.spacing(np.float32(1.0e6)) == np.float32(0.0625)
    keys = dm.cell_keys(worlds[3], w["sizes"])
    assert (np.abs(keys[w["out_of_range"]]).max(axis=1) >= dm.KEY_LIMIT).all() and dm.in_key_range(keys[~w["out_of_range"]]).all()
    assert all(abs(T[0, 1]) > 0.29 and np.abs(T[:2, 3]).min() >= 1.0e6 for _, T in w["updates"])      # yaw 0.3 rad


def test_many_cells_fills_the_lists_of_one_update(orc):
    w = dm.world("many_cells")
    mr, stats = run_both(orc, w)
    assert len(stats[0]["created"]) == dm.MANY == w["caps"]["max_modified_cells"] and stats[0]["n_points"] == 4096
    keys = [mr.keys[c] for c in stats[0]["created"]]
    assert keys != sorted(keys) and keys != sorted(keys, reverse=True)
    packed = [((int(k[0]) + dm.KEY_LIMIT) << 42) | ((int(k[1]) + dm.KEY_LIMIT) << 21) | (int(k[2]) + dm.KEY_LIMIT) for k in keys]
    assert packed != sorted(packed) and [h & 1023 for h in map(_map_hash, packed)] != sorted(h & 1023 for h in map(_map_hash, packed))
    first = {}
    for i, k in enumerate(map(tuple, dm.cell_keys(w["updates"][0][0], w["sizes"]))):
        first.setdefault(k, i)
    assert sum(1 for i in first.values() if i > 1024) >= dm.MANY // 2
    assert len(stats[1]["modified"]) == dm.MANY and not stats[1]["created"]
    assert len(stats[2]["modified"]) == dm.MANY + 1 and len(stats[2]["created"]) == 1 and mr.num_cells() == w["caps"]["max_cells"]
    got = dm.reached(w)
    assert got["cell_capacity"] == w["caps"]["cell_capacity"] and got["max_update_points"] == w["caps"]["max_update_points"]


def _map_hash(k):
    """The 64-bit finaliser the device hashes packed cell keys with (map_hash of liodom_map.h)."""
    m = (1 << 64) - 1
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & m; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & m; k ^= k >> 33
    return k


def test_brim_fills_the_member_lists_without_overflow(orc):
    """Update 1 asks for 128 member-list items in 64 multi-point leaves of ONE modified cell of 64 points: more than
    max_modified_cells * cell_capacity = 64 items and than 64 / 2 + 1 = 33 leaves, the sizes these lists had before they were
    sized by old and new points together."""
    w = dm.world("brim")
    caps = w["caps"]
    assert caps == dict(max_cells=4, cell_capacity=64, max_update_points=128, max_modified_cells=1)
    mr, stats = run_both(orc, w)
    assert stats[0]["max_leaves"] == 64 and stats[0]["n_points"] == 128
    assert stats[1]["cursor"] == 128 and stats[1]["n_multi"] == 64 and stats[1]["max_leaves"] == 64 and not stats[1]["created"]
    assert stats[1]["cursor"] > caps["max_modified_cells"] * caps["cell_capacity"]
    assert stats[1]["n_multi"] > caps["max_modified_cells"] * caps["cell_capacity"] // 2 + 1
    items_max = caps["max_modified_cells"] * caps["cell_capacity"] + caps["max_update_points"]
    assert stats[1]["cursor"] <= items_max and stats[1]["n_multi"] <= (items_max + 1) // 2
    assert all(len(st["modified"]) == 1 for st in stats) and mr.num_cells() == 1
    assert stats[2]["max_leaves"] == 65 and stats[2]["n_points"] == 1          # one leaf more than the cell holds


@pytest.mark.parametrize("name", list(dm.WORLDS))
def test_scratch_bound_holds_on_every_world(name):
    """cursor <= max_modified_cells * cell_capacity + max_update_points and n_multi <= half of it, by the restatement's count."""
    w = dm.world(name)
    caps = w["caps"]
    r = dm.Restated(*w["sizes"])
    items_max = caps["max_modified_cells"] * caps["cell_capacity"] + caps["max_update_points"]
    for pts, T in w["updates"]:
        st = r.update(pts, T)
        if len(st["modified"]) <= caps["max_modified_cells"] and st["max_leaves"] <= caps["cell_capacity"]:
            assert st["cursor"] <= items_max and st["n_multi"] <= (items_max + 1) // 2


def test_thousands_is_a_blob_of_single_point_cells():
    for n in (4096, 4097):
        w = dm.thousands(n)
        blob = api.build_map_state(*w["sizes"], w["cells"])
        st = api.parse_map_state(blob, sizes=w["sizes"])
        assert len(st["keys"]) == n and list(st["counts"]) == [1] * n and st["points"].shape == (n, 4)
        assert dm.same_bits(st["points"], np.concatenate(w["cells"]))
        assert w["caps"]["max_cells"] == n and w["caps"]["cell_capacity"] == 4
        keys = [tuple(k) for k in st["keys"]]
        assert keys != sorted(keys)
