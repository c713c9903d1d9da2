"""LoopCloser(odometry_info="solve", odometry_source=(handle, stream)) with the stubs of tests/test_loop_closer.py and a stub
handle: the graph receives the information the handle's call returns for the interval (the previous key frame's scan, this key
frame's scan); the constant stands, and is counted, where no scan index was fed, where it did not increase, where the call is
refused and where the record is not exactly VALID; a LoopCloser built as before does what it did.  No GPU, no library call."""
import numpy as np
import pytest

import graph_model as gm
from liodom_amd import api, loop
from test_loop_closer import StubGraph, StubMap, StubPlaces, _cloud


class StubHandle:
    """odometry_edges answers with Omega = (100 + from) I + to E_00, flags as scripted per `to`, and keeps the calls."""

    def __init__(self, flags=None, refuse=()):
        self.calls, self.flags, self.refuse = [], dict(flags or {}), set(refuse)

    def odometry_edges(self, stream, scan_from, scan_to, **options):
        self.calls.append((stream, list(scan_from), list(scan_to), dict(options)))
        if scan_to[0] in self.refuse:
            e = api.LiodomError("refused")
            e.code = api.ERR_INVALID_ARG
            raise e
        out = np.zeros(1, api.ODOM_EDGE_DTYPE)
        out["scan_from"], out["scan_to"] = scan_from[0], scan_to[0]
        out["flags"] = self.flags.get(scan_to[0], api.ODOM_EDGE_VALID)
        out["information"][0] = self.omega(scan_from[0], scan_to[0])
        return out

    @staticmethod
    def omega(a, b):
        om = (100.0 + a) * np.eye(6)
        om[0, 0] += b
        return om


def _closer(handle, **kw):
    gr = StubGraph()
    lc = loop.LoopCloser(StubMap(reach=0.5), StubPlaces(), [dict(step_xy=0.4)], graph=gr, min_dist=4.0, min_gap=50, k=1,
                         odometry_info="solve", odometry_source=(handle, 1), **kw)
    return lc, gr


def _pose(x):
    return gm.from_axis_angle((0, 0, 1), 0.0, (float(x), 0.0, 0.0))


def test_the_graph_receives_the_calls_information():
    h = StubHandle()
    lc, gr = _closer(h, odometry_options=dict(inflation=40.0, floor_translation=1e-3))
    keys = []
    for n in range(0, 33):                                         # 1 m per scan, a key frame every 4 m; scan index = 2 n + 7
        if lc.feed(_pose(n), _cloud((n, 0, 0)), scan=2 * n + 7)["key_frame"]:
            keys.append(2 * n + 7)
    assert len(keys) == 9 and lc.odometry_fallbacks == 0
    assert h.calls == [(1, [a], [b], dict(inflation=40.0, floor_translation=1e-3)) for a, b in zip(keys[:-1], keys[1:])]
    odo = [e for e in gr.edge_list if e["kind"] == 0]
    assert len(odo) == 8
    for e, a, b in zip(odo, keys[:-1], keys[1:]):
        assert np.array_equal(e["info"], StubHandle.omega(a, b))
        want = gm.between(gr.nodes[int(e["i"])], gr.nodes[int(e["j"])])
        assert np.max(np.abs(e["z"] - want)) <= 1e-15             # Z stays between(the fed poses)


def test_every_fallback_is_counted():
    # key frames at n = 0, 4, 8, ...: node k's scan is scripted below
    scans = {0: 10, 4: 14, 8: None, 12: 22, 16: 22, 20: 21, 24: 30, 28: 34, 32: 38, 36: 42, 40: 46}
    h = StubHandle(flags={34: api.ODOM_EDGE_VALID | api.ODOM_EDGE_GAPS, 38: api.ODOM_EDGE_NOT_PD, 42: api.ODOM_EDGE_NO_POSE}, refuse={46})
    lc, gr = _closer(h)
    for n in range(0, 41):
        lc.feed(_pose(n), _cloud((n, 0, 0)), scan=scans.get(n, 1000 + n))
    odo = [e for e in gr.edge_list if e["kind"] == 0]
    assert len(odo) == 10
    want = [StubHandle.omega(10, 14),        # 10 -> 14: the call's
            loop.ODOMETRY_INFO,              # scan None
            loop.ODOMETRY_INFO,              # the key frame before had no scan
            loop.ODOMETRY_INFO,              # 22 -> 22: not increased
            loop.ODOMETRY_INFO,              # 22 -> 21: decreased (a stream seeded again)
            StubHandle.omega(21, 30),        # and on from there
            loop.ODOMETRY_INFO,              # VALID | GAPS
            loop.ODOMETRY_INFO,              # NOT_PD
            loop.ODOMETRY_INFO,              # NO_POSE
            loop.ODOMETRY_INFO]              # the call refused
    for e, w in zip(odo, want):
        assert np.array_equal(e["info"], w), (int(e["i"]), int(e["j"]))
    assert lc.odometry_fallbacks == 8
    assert [(c[1][0], c[2][0]) for c in h.calls] == [(10, 14), (21, 30), (30, 34), (34, 38), (38, 42), (42, 46)]
    # feed without the keyword at all: the constant, counted
    lc2, gr2 = _closer(StubHandle())
    for n in range(0, 9):
        lc2.feed(_pose(n), _cloud((n, 0, 0)))
    assert lc2.odometry_fallbacks == 2 and all(np.array_equal(e["info"], loop.ODOMETRY_INFO) for e in gr2.edge_list)


def test_the_defaults_are_untouched():
    h = StubHandle()
    gr = StubGraph()
    lc = loop.LoopCloser(StubMap(reach=0.5), StubPlaces(), [dict(step_xy=0.4)], graph=gr, min_dist=4.0, min_gap=50, k=1)
    given = 7.0 * np.eye(6)
    gr2 = StubGraph()
    lc2 = loop.LoopCloser(StubMap(reach=0.5), StubPlaces(), [dict(step_xy=0.4)], graph=gr2, min_dist=4.0, min_gap=50, k=1, odometry_info=given)
    for n in range(0, 13):
        lc.feed(_pose(n), _cloud((n, 0, 0)))
        lc2.feed(_pose(n), _cloud((n, 0, 0)), scan=n)              # a scan index without "solve" changes nothing
    assert len(gr.edge_list) == 3 and all(np.array_equal(e["info"], loop.ODOMETRY_INFO) for e in gr.edge_list)
    assert len(gr2.edge_list) == 3 and all(np.array_equal(e["info"], given) for e in gr2.edge_list)
    assert lc.odometry_fallbacks == 0 and lc2.odometry_fallbacks == 0 and not lc.odometry_from_solve and h.calls == []
    assert np.array_equal(loop.ODOMETRY_INFO, np.diag([400.0, 400.0, 400.0, 100.0, 100.0, 100.0]))
    for bad in (dict(odometry_info="solve"), dict(odometry_info="chain", odometry_source=(h, 0)), dict(odometry_source=(h, 0)),
                dict(odometry_options=dict(inflation=2.0))):
        with pytest.raises(ValueError):
            loop.LoopCloser(StubMap(reach=0.5), StubPlaces(), [], graph=StubGraph(), **bad)
