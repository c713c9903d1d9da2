"""filter_local_map (kernels_filter.h: VoxelGrid(0.4) of the full window) on designed clouds: leaves of more than 512 points (the
branch of k_voxel_centroid that ranks in global memory), of exactly 512, points exactly on leaf faces on both sides of 0, a
single leaf, single-point leaves, pole worlds at kilometre scale.

Bar: liodom_get_local_map reports `filtered` and is BIT-EQUAL to orc.voxel_grid(window, 0.4) in PCL's output order; on top,
every centroid lies within cnt * 2^-23 * max|coord| of the float64 mean of its leaf's points computed in NumPy (the bound of
a float sum of cnt terms; derived, not tuned).  Then one more step: the search runs on the filtered cloud and must give the
oracle's correspondences exactly (tests/test_gpu_designed_knn.py).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import liodom_amd as la
import designed_clouds as dc
from test_gpu_designed_knn import EDGE_CAP, EPR, H, R, _Env, check_pass

pytestmark = pytest.mark.gpu

LEAF = np.float32(0.4)
N_Q = 400


def one_leaf(seed=21, n=300):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 4), np.float32)
    x[:, :3] = rng.uniform(0.41, 0.79, (n, 3)) * [1.0, -1.0, 1.0] + [0.0, 0.0, 0.4]
    x[:, 3] = rng.uniform(0, 100, n)
    return x


def single_point_leaves(seed=22, n=1000):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(-15, 15, (3 * n, 3)), axis=0)
    k = k[rng.permutation(len(k))[:n]]
    x = np.zeros((len(k), 4), np.float32)
    x[:, :3] = (k + 0.5) * 0.4
    x[:, 3] = rng.uniform(0, 100, len(k))
    return x


def crowded_leaves(seed=23):
    """Three leaves of 513, 512 and 1500 random float points with random intensities: the order of a float sum matters."""
    rng = np.random.default_rng(seed)
    parts = []
    for n, corner in ((513, (0.4, 0.4, 0.4)), (512, (-0.8, 0.4, 0.0)), (1500, (2.0, -2.0, -0.4))):
        x = np.zeros((n, 4), np.float32)
        x[:, :3] = np.asarray(corner) + rng.uniform(0.01, 0.39, (n, 3))
        x[:, 3] = rng.uniform(0, 100, n)
        parts.append(x)
    x = np.concatenate(parts)
    return x[rng.permutation(len(x))]


def _queries(cloud, seed):
    rng = np.random.default_rng(seed)
    q = cloud[rng.integers(0, len(cloud), N_Q)].copy()
    q[:, :3] += rng.normal(0.0, 0.05, (N_Q, 3)).astype(np.float32)
    return q


def clouds():
    """(name, cloud, queries, group of every point or None).  The intensities of the designed worlds are redrawn at random:
    their coordinates are short dyadic fractions whose float sums are exact in any order, the intensity sums are not."""
    out = [("leaf_aligned", dc.leaf_aligned(), _queries(dc.leaf_aligned(), 31), None),
           ("one_leaf", one_leaf(), _queries(one_leaf(), 32), None),
           ("single_point_leaves", single_point_leaves(), _queries(single_point_leaves(), 33), None),
           ("crowded_leaves", crowded_leaves(), _queries(crowded_leaves(), 34), None)]
    for name, (m, q) in [("dense", dc.dense(N_Q))] + [("poles-" + dc.origin_id(o), dc.poles(o, N_Q)) for o in dc.ORIGINS]:
        grp = dc.groups_of(m)
        m = m.copy()
        m[:, 3] = np.random.default_rng(35).uniform(0, 100, len(m))
        out.append((name, m, q, grp))
    return out


def leaves_of(win):
    """PCL's leaf index of every window point (float multiply by 1 / 0.4f, floor), the points grouped by ascending leaf
    index in window order: (order, start of every leaf in `order`, count of every leaf)."""
    inv = np.float32(1.0) / LEAF
    ijk = np.floor(win[:, :3] * inv).astype(np.int64)
    mn = ijk.min(axis=0)
    div = ijk.max(axis=0) - mn + 1
    # PCL 1.10 refuses a leaf grid of more than INT_MAX cells and passes the cloud through; neither the oracle nor
    # k_voxel_insert models that: the designed clouds stay below it
    assert int(div[0]) * int(div[1]) * int(div[2]) < 2 ** 31
    idx = (ijk[:, 0] - mn[0]) + (ijk[:, 1] - mn[1]) * div[0] + (ijk[:, 2] - mn[2]) * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    ids, start, count = np.unique(idx[order], return_index=True, return_counts=True)
    return order, start, count, ids


def leaf_ids(win):
    return leaves_of(win)[3].astype(np.int32)


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(P):
        if P not in made:
            with _Env({}):
                g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, filter_local_map=1),
                              la.make_config(n_streams=1, max_points=H * 1024, max_width=1024, debug_buffers=1))
            modes = g.modes()
            assert modes["filter_local_map"] == "1" and modes["knn_instance"] == "256", modes
            made[P] = g
        made[P].reset()
        return made[P]

    yield get
    for g in made.values():
        g.close()


@pytest.mark.parametrize("which", range(len(clouds())), ids=[c[0] for c in clouds()])
@pytest.mark.parametrize("P", [1, 4])
def test_filtered_local_map_on_designed_clouds(orc, handles, P, which):
    name, cloud, queries, grp = clouds()[which]
    g = handles(P)
    po = orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, knn_mode=0, filter_local_map=True)
    # P frames that cannot match each other, so that every solve leaves the pose at the identity and the window is the cloud bit
    # for bit: the groups (poles, runs: more than 1 m apart) dealt out over the frames, or the whole cloud between empty frames
    for f in range(P):
        frame = cloud[grp % P == f] if grp is not None else (cloud if f == min(1, P - 1) else cloud[:0])
        assert len(frame) <= EDGE_CAP
        _, info = g.odometry_step(frame)
        assert info.status == 0, (name, f, info.status)
    win, nf = g.window()
    assert nf == P and len(win) == len(cloud)
    assert sorted(map(bytes, win)) == sorted(map(bytes, cloud)), name      # the window is the cloud bit for bit, in window order
    lm, filtered = g.local_map()
    assert filtered, name
    ref = orc.voxel_grid(win, 0.4)
    assert lm.shape == ref.shape and np.array_equal(lm.view(np.uint32), ref.view(np.uint32)), \
        (name, lm.shape, ref.shape, np.nonzero((lm.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0][:10] if lm.shape == ref.shape else None)
    # the plain high-precision leg: float64 mean of every leaf
    order, start, count, _ = leaves_of(win)
    assert len(count) == len(lm), name
    w64 = win.astype(np.float64)[order]
    mean = np.add.reduceat(w64, start, axis=0) / count[:, None]
    big_xyz = np.maximum.reduceat(np.abs(w64[:, :3]).max(axis=1), start)
    big_i = np.maximum.reduceat(np.abs(w64[:, 3]), start)
    err = np.abs(lm.astype(np.float64) - mean)
    assert (err[:, :3] <= (count * 2.0 ** -23 * big_xyz)[:, None]).all(), (name, float((err[:, :3] / (count * big_xyz)[:, None]).max()))
    assert (err[:, 3] <= count * 2.0 ** -23 * big_i).all(), name
    if name in ("dense", "crowded_leaves"):
        assert count.max() > 512 and (count == 512).any(), (name, count.max())      # the crowded branch really ran
    if name == "one_leaf":
        assert len(count) == 1
    if name == "single_point_leaves":
        assert count.max() == 1 and sorted(map(bytes, lm)) == sorted(map(bytes, win))
    # the search on the filtered cloud (liodom_get_correspondences reports PCL's leaf indices there)
    leaf_index = leaf_ids(win)
    assert len(leaf_index) == len(lm)
    _, info = g.odometry_step(queries)
    assert info.status == 0 and info.map_points == len(lm), (name, info.status, info.map_points)
    for it in (0, 1):
        check_pass(orc, po, g, it, 0, lm, "%s P=%d filtered" % (name, P), index_of=leaf_index)
