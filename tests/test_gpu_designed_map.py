"""The device map's update (k_map_assign ... k_map_commit) on the designed worlds of tests/designed_maps.py, through
liodom_map_update and — one case — through the lagged mapper of a handle.  tests/test_designed_maps.py asserts on the CPU that
the worlds reach what they were designed to reach.

Bar, after every update: num_cells(), all() and local() equal the oracle's (orc.Map) bit for bit, status() == 0 wherever the world
stays inside the map's capacities.  On top, the plain high-precision leg: all() is split into cells with the records of
export_state(), and every channel c of every output point of a modified cell satisfies
    |c - mean64(members)| <= n * 2^-24 * max|member|
with the leaf's n members taken from the NumPy restatement — the bound of a sequential float32 sum of n terms followed by one
division; nothing measured is in it.  At the clamps (key range, max_modified_cells, cell_capacity) only what is documented is
asserted: the status bit, that the call returns, and that liodom_map_reset gives back a map that is exact again.

Every map has the smallest capacities that hold its world.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import designed_maps as dm
import liodom_amd as la
from liodom_amd import api

pytestmark = pytest.mark.gpu

KEY_RANGE, MODIFIED_FULL, CELL_OVERFLOW = 32, 4, 8


def open_map(w, **at_least):
    caps = dict(w["caps"])
    for k, v in at_least.items():
        caps[k] = max(caps[k], v)
    return la.Map(*w["sizes"], **caps)


def split_cells(mg):
    """all() cut into cells by the counts of export_state()'s records."""
    st = api.parse_map_state(mg.export_state(), sizes=mg.sizes)
    a = mg.all()
    ends = np.cumsum(st["counts"].astype(np.int64))
    assert a.shape[0] == (int(ends[-1]) if len(ends) else 0)
    return [a[int(e - n):int(e)] for e, n in zip(ends, st["counts"])]


def check_float64(mg, stats, what):
    cells = split_cells(mg)
    for lv in stats["leaves"]:
        m = lv["members"].astype(np.float64)
        n = len(m)
        got = cells[lv["cell"]][lv["pos"]].astype(np.float64)
        bound = n * 2.0 ** -24 * np.abs(m).max(axis=0)
        assert (np.abs(got - m.mean(axis=0)) <= bound).all(), (what, lv["cell"], lv["pos"], n, got, m.mean(axis=0), bound)


def check_update(mg, mo, mr, pts, T, what, pts_ref=None):
    """One update on the device, the oracle and the restatement (the last two without the points the device must drop)."""
    ref = pts if pts_ref is None else pts_ref
    mg.update(pts, T)
    mo.update(ref, T)
    stats = mr.update(ref, T)
    assert mg.num_cells() == mo.num_cells(), what
    a, b = mg.all(), mo.all()
    assert dm.same_bits(a, b), (what, a.shape, b.shape)
    at = dm.transform(ref, T)[:, :3].astype(np.float64).mean(axis=0)
    for Tq in (T, dm.pose(0.3, at)):          # the update's pose, and a pose in the middle of what it brought
        assert dm.same_bits(mg.local(Tq, 2, 1), mo.local(Tq, 2, 1)), what
    assert len(mo.local(dm.pose(0.3, at), 2, 1)) > 0, what
    check_float64(mg, stats, what)
    return stats


def replay_after_reset(orc, mg, limit=None):
    """liodom_map_reset, then crowded's first update (`limit`: what of it a small map takes — the first points of its first
    cell): exact again, status 0."""
    w = dm.world("crowded-0")
    pts, T = w["updates"][0]
    if limit is not None:
        keys = dm.cell_keys(pts, w["sizes"])
        pts = pts[(keys == keys[0]).all(axis=1)][:limit]
    mg.reset()
    assert mg.num_cells() == 0 and mg.status() == 0 and mg.all().shape == (0, 4)
    stats = check_update(mg, orc.Map(*w["sizes"]), dm.Restated(*w["sizes"]), pts, T, "replay after reset")
    assert mg.status() == 0 and stats["n_multi"] >= 3
    return stats


@pytest.mark.parametrize("name", ["crowded-0", "crowded-1000", "faces-10-0.5", "faces-25-0.3", "faces-40-0.4"])
def test_world_is_bit_exact_after_every_update(orc, name):
    w = dm.world(name)
    mg, mo, mr = open_map(w), orc.Map(*w["sizes"]), dm.Restated(*w["sizes"])
    for k, (pts, T) in enumerate(w["updates"]):
        check_update(mg, mo, mr, pts, T, (name, k))
        assert mg.status() == 0, (name, k, mg.status())
    mg.close()


def test_far_and_the_key_range(orc):
    w = dm.world("far")
    first = dm.world("crowded-0")["updates"][0][0]
    mg = open_map(w, max_update_points=len(first))
    mo, mr = orc.Map(*w["sizes"]), dm.Restated(*w["sizes"])
    for k, (pts, T) in enumerate(w["updates"][:-1]):
        check_update(mg, mo, mr, pts, T, ("far", k))
        assert mg.status() == 0, ("far", k, mg.status())
    pts, T = w["updates"][-1]
    out = w["out_of_range"]
    check_update(mg, mo, mr, pts, T, ("far", "key range"), pts_ref=pts[~out])      # the rest of the update is the oracle's
    assert mg.status() & KEY_RANGE
    replay_after_reset(orc, mg)
    mg.close()


def test_many_cells_and_the_modified_list(orc):
    w = dm.world("many_cells")
    mg, mo, mr = open_map(w), orc.Map(*w["sizes"]), dm.Restated(*w["sizes"])
    for k, (pts, T) in enumerate(w["updates"][:2]):
        st = check_update(mg, mo, mr, pts, T, ("many_cells", k))
        assert len(st["modified"]) == dm.MANY and mg.status() == 0, ("many_cells", k, mg.status())
    assert mg.num_cells() == dm.MANY
    pts, T = w["updates"][2]
    mg.update(pts, T)                         # 257 cells: the call returns and says so
    assert mg.status() & MODIFIED_FULL
    replay_after_reset(orc, mg)
    mg.close()


def test_brim_and_the_cell_capacity(orc):
    w = dm.world("brim")
    mg, mo, mr = open_map(w), orc.Map(*w["sizes"]), dm.Restated(*w["sizes"])
    for k, (pts, T) in enumerate(w["updates"][:2]):
        st = check_update(mg, mo, mr, pts, T, ("brim", k))
        assert st["max_leaves"] == w["caps"]["cell_capacity"] and mg.status() == 0, ("brim", k, mg.status())
    assert st["cursor"] == 128 and st["n_multi"] == 64
    pts, T = w["updates"][2]
    mg.update(pts, T)                         # a 65th leaf
    assert mg.status() & CELL_OVERFLOW
    replay_after_reset(orc, mg, limit=w["caps"]["max_update_points"])
    mg.close()


@pytest.mark.parametrize("n_cells", [4096, 4097])
def test_thousands_of_cells_come_back_whole(n_cells):
    w = dm.thousands(n_cells)
    blob = api.build_map_state(*w["sizes"], w["cells"])
    want = api.parse_map_state(blob, sizes=w["sizes"])["points"]
    mg = open_map(w)
    mg.import_state(blob)
    assert mg.num_cells() == n_cells
    a = mg.all()
    assert a.shape == (n_cells, 4) and dm.same_bits(a, want)
    assert mg.status() == 0
    assert mg.export_state() == blob
    mg.close()


def test_lagged_mapper_leaves_the_bits_of_update(orc):
    """The k_map_assign<false> path: crowded's updates as frames of a one-stream mapping handle with a lagged mapper
    (liodom_attach_mapper_ex, lag = 1), then P far-away frames that push them out of the window.  Whatever leaves the window
    enters the attached map as it is; the same frames through liodom_map_update with the identity pose, and through the oracle,
    leave the same map bit for bit.
    The pose is not held at the identity by construction: updates 2-4 return to the leaves of update 0, so a frame can find
    correspondences in the map and its solve may move it.  The reference maps are therefore fed the frames the handle's window
    reports as leaving (the first is the designed update bit for bit: nothing precedes it).  On an MI355X updates 0 and 1 enter
    the map as designed and updates 2-4 moved."""
    H, R, EPR, P = 64, 8, 16, 3               # edge capacity 64 * 8 * 17 = 8704 >= 4096
    w = dm.world("crowded-0")
    frames = [pts for pts, _ in w["updates"]]
    frames += [dm.cloud([[500.0 + 7.0 * k + 0.01 * i, 500.0, 3.0 + 0.01 * i] for i in range(8)], seed=80 + k) for k in range(P)]
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                  la.make_config(n_streams=1, max_points=H * 1024, max_width=1024, recv_capacity=1 << 17))
    caps = dict(w["caps"], max_cells=64, cell_capacity=4096, max_modified_cells=16)      # (a moved frame may spill into other leaves)
    mA, mB, mo = la.Map(*w["sizes"], **caps), la.Map(*w["sizes"], **caps), orc.Map(*w["sizes"])
    g.attach_mapper(mA, 2, 1, lag=1)
    assert g.modes()["mapper_lag"] == "1"
    held = []
    for j, f in enumerate(frames):
        win, nf = g.window()
        leaving = win[:len(frames[j - P])].copy() if nf == P else None
        assert (leaving is not None) == (j >= P)
        _, info = g.odometry_step(f)
        assert info.status == 0 and info.n_edges == len(f), (j, info.status)
        if leaving is None:
            assert mA.num_cells() == 0, j
            continue
        held.append(dm.same_bits(leaving, frames[j - P]))
        mB.update(leaving, dm.IDENTITY)
        mo.update(leaving, dm.IDENTITY)
        a = mA.all()
        assert mA.num_cells() == mB.num_cells() == mo.num_cells(), j
        assert dm.same_bits(a, mB.all()) and dm.same_bits(a, mo.all()), j
    print("lagged mapper: frames that entered the map as designed (pose held at the identity):", held)
    assert len(held) == len(w["updates"]) and held[0]
    assert mA.status() == 0 and mB.status() == 0 and mA.num_cells() >= 2
    assert mA.export_state() == mB.export_state()
    g.attach_mapper(None)
    g.close(); mA.close(); mB.close()
