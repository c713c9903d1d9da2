"""The place descriptor's contract on the CPU (tests/place_model.py: the NumPy restatement the GPU tests hold the kernels equal
to): bits written out by hand for small clouds, the properties of the distance, the sign of a match's pose, the designed clouds of
place_designed.py, and the recognition figures on the project's circle.  No GPU, no library call."""
import math

import numpy as np
import pytest

from liodom_amd import api
import place_designed as pd
import place_model as pm

B = lambda *bits: sum(1 << b for b in bits)      # noqa: E731


def _only(desc, word, *bits):
    want = np.zeros(len(desc), np.uint64)
    want[word] = np.uint64(B(*bits))
    return np.array_equal(desc, want)


def test_tables_of_the_default_geometry():
    t = api.place_tables(pm.DEFAULT)
    assert list(t["R2"]) == [np.float32(25.0 * i * i) for i in range(1, 17)]             # rings of 5 m: exact
    assert list(t["Z"]) == [-4.0, 0.0, 4.0, 8.0, 12.0]
    assert t["C"].dtype == np.float32 and t["C"][7] == t["S"][7] == np.float32(math.sqrt(0.5))       # 45 degrees
    assert (np.diff(t["C"]) < 0).all() and (np.diff(t["S"]) > 0).all()
    for bad in ((0, 4, 80, -4, 12), (16, 5, 80, -4, 12), (16, 4, 0, -4, 12), (16, 4, 80, 12, 12), (16, 4, float("nan"), -4, 12), (65, 1, 80, -4, 12)):
        with pytest.raises(ValueError):
            api.place_tables(bad)


def test_single_points_by_hand():
    """Default geometry: rings of 5 m, layers [-4, 0), [0, 4), [4, 8), [8, 12); word = ring * 4 + layer."""
    nz = np.float32(-0.0)
    cases = [((1, 0, 0), 1, 0),                    # +x axis: j = 0, sector 0; z = 0 = Z_1: layer 1
             ((0, 1, 0), 1, 15),                   # +y axis: |y| C >= 0 for all 15: sector 15
             ((nz, 1, 0), 1, 15),                  # -0 is not below 0
             ((-1, 0, 0), 1, 31), ((-1, nz, 0), 1, 31),
             ((-1, -1e-3, 0), 1, 32), ((0, -1, 0), 1, 48), ((nz, -1, 0), 1, 48),      # x = +-0, y < 0: the quadrant "x >= 0, y < 0": 63 - 15
             ((1, -1e-3, 0), 1, 63),
             ((1, 1, 0), 1, 8),                    # 45 degrees: C_8 == S_8 in float, the comparison holds: j = 8
             ((0, 0, 0), 1, 15),                   # the origin: 0 >= 0 fifteen times
             ((1, 0, -4), 0, 0), ((1, 0, -0.001), 0, 0), ((1, 0, 3.999), 1, 0), ((1, 0, 4), 2, 0), ((1, 0, 11.99), 3, 0),
             ((5, 0, 0), 5, 0),                    # r2 == R2_1: ring 1
             ((4.999, 0, 0), 1, 0), ((0, 79.9, 0), 61, 15), ((3, 4, 0), 5, 9)]        # 3-4-5: r2 = 25; atan2(4, 3) = 53.1 deg = 9.4 sectors
    for p, word, sector in cases:
        desc, bits = pm.describe(np.array([p], np.float32))
        assert bits == 1 and _only(desc, word, sector), (p, word, sector, np.nonzero(desc), desc[np.nonzero(desc)])
    for p in ((80, 0, 0), (0, -80, 0), (60, 60, 0), (1, 0, -4.001), (1, 0, 12), (1, 0, 1e9), (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (1e30, 0, 0)):
        desc, bits = pm.describe(np.array([p], np.float32))
        assert bits == 0 and not desc.any(), p


def test_a_small_cloud_by_hand():
    cloud = np.array([[1, 0, 0, 9], [1, 0.01, 1, 9], [-1, 0, 0, 9], [6, 0, 5, 9], [0, 6, 5, 9], [np.nan, 1, 1, 9], [100, 0, 0, 9]], np.float32)
    desc, bits = pm.describe(cloud)
    want = np.zeros(64, np.uint64)
    want[1] = np.uint64(B(0, 31))                  # two points share bit 0
    want[6] = np.uint64(B(0, 15))                  # ring 1, layer 2
    assert np.array_equal(desc, want) and bits == 4
    assert pm.describe(np.zeros((0, 4), np.float32))[1] == 0
    # other geometries: one word; 64 rings of 1 m
    assert _only(pm.describe(cloud, pd.GEOMETRIES["1x1"])[0], 0, 0, 31)                   # z in [-1, 3): the first three points
    d = pm.describe(cloud, pd.GEOMETRIES["64x1"])[0]                                     # z in [-2, 2): rings 1, 1, 1
    assert np.array_equal(np.nonzero(d)[0], [1]) and d[1] == np.uint64(B(0, 31))


def test_the_sector_walks_once_around_the_circle():
    t = api.place_tables(pm.DEFAULT)
    a = (np.arange(64) + 0.5) * 2.0 * math.pi / 64.0
    assert list(pm.sectors(np.cos(a), np.sin(a), t)) == list(range(64))
    fine = (np.arange(6400) + 0.5) * 2.0 * math.pi / 6400.0
    s = pm.sectors(7.0 * np.cos(fine), 7.0 * np.sin(fine), t)
    assert (np.diff(s) >= 0).all() and s[0] == 0 and s[-1] == 63 and (np.bincount(s, minlength=64) == 100).all()


def test_distance_of_a_rotated_copy():
    rng = np.random.default_rng(1)
    q = pd.random_desc(rng, 1, 64)[0]
    for s in range(64):
        dist, shift = pm.match(pm.rotl(q, s), q[None, :])
        assert (int(dist[0]), int(shift[0])) == (0, (64 - s) % 64), s
    d = pm.distances(q, q[None, :])[0]
    assert d[0] == 0 and (d[1:] > 0).all() and d.max() <= 2 * int(np.bitwise_count(q).sum())
    # period 32 and 1: the lowest shift wins
    for period, lowest in ((32, 0), (1, 0)):
        p = pd.periodic_desc(rng, 4, period)
        assert np.array_equal(pm.rotl(p, period), p)
        assert [int(v) for v in pm.match(pm.rotl(p, 5), p[None, :])[1]] == [(period - 5) % period + lowest]
    assert pm.topk(np.zeros(4, np.uint64), np.zeros((1, 4), np.uint64), 2) == [(0, 0, 0), (-1, 0, 0)]
    # ties go to the lowest index
    places = np.stack([pm.rotl(q, 3), q, pm.rotl(q, 3), q])
    assert pm.topk(q, places, 4) == [(0, 0, 3), (1, 0, 0), (2, 0, 3), (3, 0, 0)]
    assert pm.topk(q, np.zeros((0, 64), np.uint64), 3) == [(-1, 0, 0)] * 3


@pytest.mark.parametrize("m", [0, 1, 5, 16, 31, 32, 50, 63])
def test_the_pose_of_a_match_has_the_right_sign(m):
    """A cloud of bin centres, turned by +a = m sectors about z in the sensor frame, is what a sensor sees whose heading is the key
    frame's turned by -a: the match's pose must say so."""
    geom = pm.DEFAULT
    rng = np.random.default_rng(2)
    cloud = np.array([pd.bin_centre(geom, int(rng.integers(0, 16)), int(rng.integers(0, 4)), int(rng.integers(0, 64))) for _ in range(60)], np.float32)
    a = m * 2.0 * math.pi / 64.0
    k, _ = pm.describe(cloud, geom)
    q, _ = pm.describe(pm.rot_z(cloud, a), geom)
    assert np.array_equal(q, pm.rotl(k, m))
    place = np.array([0.0, 0.0, math.sin(0.35), math.cos(0.35), 3.0, -2.0, 1.0])          # heading 0.7 rad
    (idx, dist, shift), = pm.topk(q, k[None, :], 1)
    assert (idx, dist, shift) == (0, 0, (64 - m) % 64)
    pose = pm.match_pose(place, shift)
    assert pm.angle_diff(pm.yaw_of(pose), 0.7 - a) < 1e-12 and np.array_equal(pose[4:], place[4:])
    assert abs(np.linalg.norm(pose[:4]) - 1.0) < 1e-15
    # an unnormalised place quaternion is normalised first
    assert np.allclose(pm.match_pose(np.concatenate([place[:4] * (1 + 5e-7), place[4:]]), shift), pose, atol=1e-15, rtol=0)


@pytest.mark.parametrize("name", list(pd.GEOMETRIES))
def test_designed_clouds_on_the_model(name):
    geom = pd.GEOMETRIES[name]
    W = pm.words(geom)
    full = pm.describe(pd.one_point_per_bit(geom), geom)
    assert full[1] == 64 * W and (full[0] == pm.ALL).all() and len(pd.one_point_per_bit(geom)) == 64 * W
    one = pm.describe(pd.all_in_one_bit(geom), geom)
    assert one[1] == 1 and one[0][W - 1] == np.uint64(1 << 37)
    pts = pd.single_points(geom)
    got = {n: pm.describe(np.array([p], np.float32), geom) for n, p in pts}
    assert all(b <= 1 for _, b in got.values())
    for quad, base, sign in (("q1", 0, 1), ("q2", 31, -1), ("q3", 32, 1), ("q4", 63, -1)):
        for i in range(1, 16):
            # on the tangent and above it the comparison holds (j counts i); one float below it does not
            below, on, above = (got["tangent %s %d %d" % (quad, i, n)][0] for n in range(3))
            assert int(above[0]).bit_length() - 1 == base + sign * i, (quad, i)
            assert int(below[0]).bit_length() - 1 in (base + sign * i, base + sign * (i - 1)), (quad, i)
            assert int(got["tangent %s %d equal" % (quad, i)][0][0]).bit_length() - 1 == base + sign * i, (quad, i)
        assert any(int(got["tangent %s %d 0" % (quad, i)][0][0]).bit_length() - 1 == base + sign * (i - 1) for i in range(1, 16))
    for n in ("nan in x", "+inf in y", "-inf in z", "r_max", "2 r_max", "r2 overflows", "far below", "far above", "layer %d 1" % geom[1], "layer 0 0"):
        assert got[n][1] == 0, n
    assert got["layer 0 1"][1] == 1 and got["r2 underflows"][1] == 1 and got["axis -0 -0"][1] == 1


def test_recognition_on_the_circle(orc, synth):
    """47 key frames (scans 0, 4, .., 184 at their ground-truth poses), 111 queries (scans 188 .. 224, each as it is and turned by
    1.0 and 2.5 rad): every query has a key frame within 4 m among its 3 best, at most 3 miss at rank 1, and the yaw of the nearest
    such match is within 0.15 rad of the truth (half a sector of 0.098 rad plus up to two scans of heading)."""
    run = pm.circle(orc, synth)
    assert len(run["keys"]) == 47 and len(run["queries"]) == 111
    assert 300 < np.mean([len(e) for _, _, e, _ in run["queries"]]) < 600
    for label, geom in (("default", pm.DEFAULT), ("40 m", api.place_geometry(16, 4, 40.0, -2.0, 6.0))):
        M = pm.circle_model(orc, synth, geom)
        miss1, worst = 0, 0.0
        for (k, a, e, true), top in zip(run["queries"], M["top3"]):
            near = [r for r, (i, d, s) in enumerate(top) if i >= 0 and np.linalg.norm(run["keys"][i][2][4:] - true[4:]) <= 4.0]
            assert near, (label, k, a, top)
            miss1 += near[0] != 0
            i, d, s = top[near[0]]
            worst = max(worst, pm.angle_diff(pm.yaw_of(pm.match_pose(run["keys"][i][2], s)), pm.yaw_of(true)))
        print("circle, %s geometry: rank-1 misses %d of 111, worst yaw error %.3f rad" % (label, miss1, worst))
        assert miss1 <= 3 and worst <= 0.15, (label, miss1, worst)
