"""The covariance entry points of the pose graph (liodom_graph_cov_options_default, _solve_columns, _covariance, _gate_edges,
_cov_counters): exported by libliodom_hip.so and listed, the header still a C11 header with the signatures given and the status
numbers, the new structs' sizes and the old ones unchanged, the argument errors that need no device; and LoopCloser's gate with
a stub graph: what is added, what is refused, what gate=None leaves alone.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import graph_model as gm
import liodom_amd as la
from liodom_amd import api, loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_graph_cov_options_default", "liodom_graph_solve_columns", "liodom_graph_covariance", "liodom_graph_gate_edges",
       "liodom_graph_cov_counters")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("solve_columns", "covariance", "gate_edges", "cov_counters"):
        assert callable(getattr(api.PoseGraph, name))
    assert api.GRAPH_COV_STATUSES == ("ok", "not_converged", "breakdown", "unanchored", "not_pd")
    assert any(p.endswith(os.sep + "graph_marginals.h") for p in api._SRC)          # a change to it rebuilds the library


def test_header_is_c11_and_the_structs_have_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  void (*od)(liodom_graph_cov_options_t*) = liodom_graph_cov_options_default;\n'
                   '  int (*sc)(liodom_graph_t*, const int32_t*, int, const liodom_graph_cov_options_t*, double*, liodom_graph_cov_status_t*) = liodom_graph_solve_columns;\n'
                   '  int (*cv)(liodom_graph_t*, const int32_t*, const int32_t*, int, const liodom_graph_cov_options_t*, double*, int32_t*) = liodom_graph_covariance;\n'
                   '  int (*ge)(liodom_graph_t*, const liodom_graph_edge_t*, int, const liodom_graph_cov_options_t*, double*, int32_t*) = liodom_graph_gate_edges;\n'
                   '  int (*cc)(liodom_graph_t*, int64_t*, int64_t*) = liodom_graph_cov_counters;\n'
                   '  return od && sc && cv && ge && cc && LIODOM_GRAPH_COV_OK == 0 && LIODOM_GRAPH_COV_NOT_CONVERGED == 1 &&\n'
                   '         LIODOM_GRAPH_COV_BREAKDOWN == 2 && LIODOM_GRAPH_COV_UNANCHORED == 3 && LIODOM_GRAPH_COV_NOT_PD == 4; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                     'sizeof(liodom_graph_cov_options_t), sizeof(liodom_graph_cov_status_t), sizeof(liodom_graph_options_t), '
                     'sizeof(liodom_graph_report_t), sizeof(liodom_graph_edge_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [16, 16, 32, 48, 360]
    assert C.sizeof(api.GraphCovOptions) == 16 and api.GRAPH_COV_STATUS_DTYPE.itemsize == 16


def test_defaults_and_argument_errors_that_need_no_device():
    L = la.load()
    o = api.make_graph_cov_options()
    assert (o.max_pcg_iterations, o.batch_columns, o.pcg_tolerance) == (0, 0, 1e-8)
    assert api.make_graph_cov_options(batch_columns=7, pcg_tolerance=1e-6).batch_columns == 7
    with pytest.raises(KeyError):
        api.make_graph_cov_options(gradient_tolerance=1.0)
    L.liodom_graph_cov_options_default(None)
    one = np.ones(1, np.int32)
    buf = np.zeros(36)
    st = np.zeros(6, api.GRAPH_COV_STATUS_DTYPE)
    a, b = C.c_int64(7), C.c_int64(7)
    assert L.liodom_graph_solve_columns(None, api._ip(one), 1, C.byref(o), api._dp(buf), st.ctypes.data_as(C.c_void_p)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_solve_columns" in L.liodom_last_error()
    assert L.liodom_graph_covariance(None, api._ip(one), api._ip(one), 1, C.byref(o), api._dp(buf), api._ip(one)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_covariance" in L.liodom_last_error()
    assert L.liodom_graph_gate_edges(None, None, 0, C.byref(o), api._dp(buf), api._ip(one)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_gate_edges" in L.liodom_last_error()
    assert L.liodom_graph_cov_counters(None, C.byref(a), C.byref(b)) == api.ERR_INVALID_ARG and (a.value, b.value) == (7, 7)
    assert not buf.any() and one[0] == 1 and not st["status"].any()


class GateGraph:
    """A graph that records what is added and gates by a table: d2 of a candidate = 100 x the length of its Z's translation."""

    def __init__(self, status=0):
        self.n, self.edge_list, self.asked, self.status = 0, [], [], status

    def add_nodes(self, poses, fixed=None):
        first = self.n
        self.n += len(np.asarray(poses).reshape(-1, 7))
        return first

    def add_edges(self, edges):
        self.edge_list += [e.copy() for e in edges]

    def gate_edges(self, edges, **opt):
        self.asked.append((edges.copy(), opt))
        return np.array([100.0 * np.linalg.norm(e["z"][4:]) for e in edges]), np.full(len(edges), self.status, np.int32)


def _closer(graph, **kw):
    lc = loop.LoopCloser(None, None, [], graph=graph, min_dist=0.5, min_gap=100, **kw)
    for x in range(6):
        lc.feed(gm.from_axis_angle((0, 0, 1), 0.0, (float(x), 0.0, 0.0)), np.zeros((0, 4), np.float32))
    return lc


def test_loop_closer_adds_what_passes_the_gate_and_lists_what_does_not():
    near = gm.from_axis_angle((0, 0, 1), 0.1, (0.1, 0.0, 0.0))           # d2 = 10
    far = gm.from_axis_angle((0, 0, 1), 0.1, (0.3, 0.0, 0.0))            # d2 = 30
    gr = GateGraph()
    lc = _closer(gr, gate=16.81, gate_options=dict(pcg_tolerance=1e-6))
    assert len(gr.edge_list) == 5 and not gr.asked                        # odometry edges are never gated
    assert lc.add_loop(0, 5, near) is True and lc.add_loop(1, 4, far) is False
    assert len(gr.edge_list) == 6 and int(gr.edge_list[-1]["kind"]) == 1 and lc.loops == [(0, 5)]
    assert lc.gated == [(1, 4, pytest.approx(30.0), "ok")]
    assert len(gr.asked) == 2 and gr.asked[0][1] == dict(pcg_tolerance=1e-6) and int(gr.asked[1][0]["i"][0]) == 1
    # a status other than ok refuses whatever d2 is; a d2 that is NaN refuses
    gr = GateGraph(status=api.GRAPH_COV_NOT_CONVERGED)
    lc = _closer(gr, gate=16.81)
    assert lc.add_loop(0, 5, near) is False and lc.gated == [(0, 5, pytest.approx(10.0), "not_converged")] and len(gr.edge_list) == 5
    # without a gate nothing is asked and everything is added
    gr = GateGraph()
    lc = _closer(gr)
    assert lc.add_loop(0, 5, near) is True and lc.add_loop(1, 4, far) is True
    assert not gr.asked and len(gr.edge_list) == 7 and lc.loops == [(0, 5), (1, 4)] and lc.gated == []
