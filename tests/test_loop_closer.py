"""LoopCloser's bookkeeping (liodom_amd/loop.py) with a stub database, a stub map and a stub graph: which scans become key frames,
the odometry edges, the lagged insertion into the database (a query never sees the recent past), which matches become loop edges.
No GPU, no library call."""
import math

import numpy as np
import pytest

import graph_model as gm
from liodom_amd import api, loop


class StubPlaces:
    def __init__(self):
        self.ids, self.poses, self.seen_at_query = [], [], []

    def add(self, edges, pose7, id=0):
        self.ids.append(int(id)); self.poses.append(np.array(pose7, np.float64))
        return len(self.ids) - 1

    def query(self, edges_list, k=1):
        """The k places nearest to the position the cloud's first point carries, nearest first."""
        at = np.asarray(edges_list[0], np.float64)[0, :3]
        self.seen_at_query.append(list(self.ids))
        out = np.zeros((1, k), api.PLACE_MATCH_DTYPE)
        out["index"] = -1
        order = sorted(range(len(self.ids)), key=lambda i: (np.linalg.norm(self.poses[i][4:] - at), i))
        for r, i in enumerate(order[:k]):
            out[0, r]["index"], out[0, r]["id"] = i, self.ids[i]
            out[0, r]["pose"], out[0, r]["place_pose"] = self.poses[i], self.poses[i]
        return out


class StubMap:
    """search_pose finds the position the cloud's first point carries if the centre is within `reach` of it: all edges hit."""

    def __init__(self, reach):
        self.reach, self.calls = reach, 0

    def search_pose(self, edges, centre, **grid):
        self.calls += 1
        at = np.asarray(edges, np.float64)[0, :3]
        centre = np.array(centre, np.float64)
        n = len(edges)
        if np.linalg.norm(centre[4:] - at) <= self.reach:
            return dict(pose=np.concatenate([centre[:4], at]), hits_r=n, hits_0=n)
        return dict(pose=centre, hits_r=n // 10, hits_0=0)


class StubGraph:
    def __init__(self):
        self.nodes, self.fixed, self.edge_list = [], [], []

    def add_nodes(self, poses, fixed=None):
        first = len(self.nodes)
        for p, f in zip(np.asarray(poses).reshape(-1, 7), fixed):
            self.nodes.append(np.array(p)); self.fixed.append(int(f))
        return first

    def add_edges(self, edges):
        self.edge_list += [e.copy() for e in edges]


def _cloud(position, n=50):
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = np.asarray(position, np.float32)
    return c


def _walk():
    """Out along x for 80 m and back on the same line, 1 m per scan, turned round at the far end."""
    poses = [gm.from_axis_angle((0, 0, 1), 0.0, (float(x), 0.0, 0.0)) for x in range(0, 81)]
    poses += [gm.from_axis_angle((0, 0, 1), math.pi, (float(x), 0.0, 0.0)) for x in range(79, -1, -1)]
    return poses


def test_key_frames_lagged_insertion_and_loop_edges():
    db, mp, gr = StubPlaces(), StubMap(reach=3.0), StubGraph()
    lc = loop.LoopCloser(mp, db, [dict(step_xy=0.4)], graph=gr, min_dist=4.0, min_gap=5, k=3, min_fraction=0.5)
    poses = _walk()
    keys, all_loops = [], []
    for n, p in enumerate(poses):
        r = lc.feed(p, _cloud(p[4:]))
        if r["key_frame"]:
            assert r["node"] == len(keys)
            keys.append(n)
            # exactly the key frames with min_gap newer ones behind them are places, in order
            assert db.ids == list(range(max(0, len(keys) - 5)))
            all_loops += r["loops"]
        else:
            assert r["node"] is None and r["loops"] == []
    # a key frame every 4 m, measured from the last key frame; the turn at the far end is no key frame by itself (min_yaw is off)
    assert keys[:4] == [0, 4, 8, 12] and len(keys) == 41
    assert gr.fixed == [1] + [0] * 40
    odo = [e for e in gr.edge_list if e["kind"] == 0]
    assert [(int(e["i"]), int(e["j"])) for e in odo] == [(k, k + 1) for k in range(40)]
    for e in odo:
        want = gm.between(gr.nodes[int(e["i"])], gr.nodes[int(e["j"])])
        assert np.max(np.abs(e["z"] - want)) <= 1e-15 and np.array_equal(e["info"], loop.ODOMETRY_INFO)
    # no query ever saw a key frame younger than the gap
    assert len(db.seen_at_query) == len(keys) - 5
    for seen, node in zip(db.seen_at_query, range(5, len(keys))):
        assert all(node - i >= 5 for i in seen)
    # on the way out nothing is near: no loop edge; on the way back every key frame lies on one of the way out
    loops = [e for e in gr.edge_list if e["kind"] == 1]
    assert loops and len(loops) == len(all_loops) == len(lc.loops)
    for e, l in zip(loops, all_loops):
        i, j = int(e["i"]), int(e["j"])
        assert (i, j) == (l["place"], l["node"]) and j - i >= 5 and j > 20
        assert np.linalg.norm(gr.nodes[i][4:] - gr.nodes[j][4:]) <= 3.0 and l["fraction"] == 1.0
        want = gm.between(gr.nodes[i], np.concatenate([gr.nodes[i][:4], gr.nodes[j][4:]]))      # the stub finds the position, keeps the match's heading
        assert np.max(np.abs(e["z"] - want)) <= 1e-15 and np.array_equal(e["info"], loop.LOOP_INFO)
    assert {int(e["j"]) for e in loops} >= set(range(26, 41))


def test_a_far_match_is_no_loop_edge_and_the_arguments_are_checked():
    db, mp, gr = StubPlaces(), StubMap(reach=0.5), StubGraph()
    lc = loop.LoopCloser(mp, db, [dict(step_xy=0.4)], graph=gr, min_dist=4.0, min_gap=2, k=2, min_fraction=0.5)
    for x in range(0, 40):
        r = lc.feed(gm.from_axis_angle((0, 0, 1), 0.0, (float(x), 0.0, 0.0)), _cloud((float(x), 0.0, 0.0)))
        assert r["loops"] == []
    assert mp.calls > 0 and all(e["kind"] == 0 for e in gr.edge_list)
    with pytest.raises(ValueError):
        loop.LoopCloser(mp, db, [], graph=gr, min_gap=0)
    with pytest.raises(ValueError):
        loop.LoopCloser(mp, db, [], graph=gr).close()


def test_pose_helpers_equal_the_model():
    rng = np.random.default_rng(3)
    for _ in range(5):
        X, Y = gm.random_pose(rng), gm.random_pose(rng)
        assert np.max(np.abs(loop.compose(X, Y) - gm.compose(X, Y))) <= 1e-13
        assert np.max(np.abs(loop.between(X, Y) - gm.between(X, Y))) <= 1e-13
        assert np.max(np.abs(loop.compose(X, loop.inverse(X)) - [0, 0, 0, 1, 0, 0, 0])) <= 1e-13
