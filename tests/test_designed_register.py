"""tests/designed_register.py holds what it was designed to hold — checked on the CPU oracle alone, so that the GPU tests built on it
(tests/test_gpu_register.py) test the kernels and not the generator."""
import numpy as np
import pytest

import designed_register as dr
import register_model as rm


def _map(orc, points):
    mo = orc.Map(dr.MAP_SIZES["xy"], dr.MAP_SIZES["z"], dr.MAP_SIZES["res"])
    mo.update(points, None)
    return mo


def _same_set(a, b):
    return sorted(map(bytes, np.ascontiguousarray(a[:, :3]))) == sorted(map(bytes, np.ascontiguousarray(b[:, :3])))


def test_every_point_enters_the_map_as_it_is_and_once(orc):
    for pts in (dr.world()["map"], dr.knn()["map"], dr.small(4)["map"], dr.small(5)["map"]):
        mo = _map(orc, pts)
        local = mo.local(None, 2, 1)
        assert local.shape[0] == pts.shape[0] and _same_set(local, pts)      # nothing merged, nothing in the centre cell (twice)


@pytest.mark.parametrize("n_edges", dr.COUNTS)
def test_world_by_edge_count(orc, n_edges):
    w = dr.world()
    local = _map(orc, w["map"]).local(None, 2, 1)
    r = rm.register(orc, None, w["edges"][:n_edges], dr.IDENTITY, local=local)
    print(n_edges, r["termination"], r["passes"], r["matches"], ["%.1e/%.1e" % mv for mv in r["moves"]])
    if n_edges < 6:
        assert r["termination"] == rm.FEW_MATCHES and r["matches"] == n_edges
        return
    assert r["termination"] == rm.CONVERGED and r["matches"] == n_edges
    # the registration finds the motion the edges were taken from, to the noise of the edges
    assert np.linalg.norm(r["pose"][4:] - dr.MOTION_T) < 0.02 and np.linalg.norm(2.0 * r["pose"][:3] - dr.MOTION_W) < 0.005
    for mt, mr in r["moves"]:      # no verdict within a factor 10 of the default thresholds 1e-4 / 1e-5
        assert not (1e-5 < mt < 1e-3) or mr > 1e-4 or mr < 1e-6, (mt, mr)
        assert not (1e-6 < mr < 1e-4) or mt > 1e-3 or mt < 1e-5, (mt, mr)


def test_neighbourhoods(orc):
    k = dr.knn()
    local = _map(orc, k["map"]).local(None, 2, 1)
    r = rm.register(orc, None, k["edges"], dr.IDENTITY, local=local, max_passes=1)
    for name, e in k["special"].items():
        if k["expect"][name] is not None:
            assert (r["corr"][e, 0] >= 0) == k["expect"][name], name
    q = np.zeros((len(k["special"]), 4), np.float32)
    names = [n for n in k["special"] if n != "nan"]
    q = k["edges"][[k["special"][n] for n in names]]
    idx, d = orc.knn5(local, q, mode=0)
    d = dict(zip(names, d))
    idx = dict(zip(names, idx))
    assert d["five_at_1"][4] == np.float32(1.0) and d["five_at_1"][3] < 0.25
    # the offset is one float below 1: its square rounds to 1 - 2^-23, the largest squared distance below 1.0f an offset can give
    assert d["five_below_1"][4] == np.float32(1.0 - 2.0 ** -23)
    assert d["ties"][0] == d["ties"][1] and d["ties"][2] == d["ties"][3] and idx["ties"][0] < idx["ties"][1]
    sixth = np.sort(np.sum((local[:, :3].astype(np.float64) - q[names.index("ties"), :3]) ** 2, axis=1))[5]
    assert sixth == d["ties"][4]                                               # the fifth place is a tie as well
    for name, axis, face in (("face_voxel", 1, 4.0), ("face_cell", 0, -10.0)):
        e = k["edges"][k["special"][name]]
        assert abs(e[axis] - face) <= 1e-3 and np.floor(e[axis]) != np.floor(local[idx[name][0], axis])
        assert len(set(np.floor(local[idx[name], axis]))) == 1                 # all five beyond the face
    assert (local[idx["negative"], :2] < 0).all() and (k["edges"][k["special"]["negative"], :2] < 0).all()
    e = k["edges"][k["special"]["crowd"]]
    assert int(np.sum(np.all(np.floor(local[:, :3]) == np.floor(e[:3]), axis=1))) == 40


@pytest.mark.parametrize("n", [4, 5])
def test_small_maps_collide_in_their_table(orc, n):
    s = dr.small(n)
    a, b = s["voxels"]
    mask = dr.table_size(n) - 1
    assert dr.table_size(n) == (8 if n == 4 else 16)
    assert dr.map_hash(dr.voxel_key(a), mask) == dr.map_hash(dr.voxel_key(b), mask)
    vox = {tuple(int(c) for c in np.floor(p[:3])) for p in s["map"]}
    assert vox == {tuple(a), tuple(b)}
    local = _map(orc, s["map"]).local(None, 2, 1)
    r = rm.register(orc, None, s["edges"], dr.IDENTITY, local=local, min_matches=100)
    assert r["termination"] == rm.FEW_MATCHES and r["matches"] == (0 if n == 4 else 10)
