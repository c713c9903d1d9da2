"""The entry points of the pose graph (liodom_graph_*): exported by libliodom_hip.so and listed, the header still a C11 header with
the signatures given, liodom_graph_edge_t 360 bytes as its ctypes and NumPy mirrors are, and the argument errors that need no device.
CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_graph_create", "liodom_graph_destroy", "liodom_graph_reset", "liodom_graph_count", "liodom_graph_add_nodes",
       "liodom_graph_add_edges", "liodom_graph_set_fixed", "liodom_graph_get_poses", "liodom_graph_set_poses", "liodom_graph_get_edges",
       "liodom_graph_linearize", "liodom_graph_multiply", "liodom_graph_options_default", "liodom_graph_optimize")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("add_nodes", "add_edges", "set_fixed", "poses", "set_poses", "edges", "linearize", "multiply", "optimize", "reset", "count"):
        assert callable(getattr(api.PoseGraph, name))
    for src in ("kernels_graph.h", "liodom_graph_host.h", "graph_csr.h"):      # a change to any of them rebuilds the library
        assert any(p.endswith(os.sep + src) for p in api._SRC), src


def test_header_is_c11_and_the_structs_have_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  int (*cr)(int, int, liodom_graph_t**) = liodom_graph_create;\n'
                   '  void (*de)(liodom_graph_t*) = liodom_graph_destroy;\n'
                   '  int (*rs)(liodom_graph_t*) = liodom_graph_reset;\n'
                   '  int (*cn)(liodom_graph_t*, int32_t*, int32_t*) = liodom_graph_count;\n'
                   '  int (*an)(liodom_graph_t*, const double*, const int32_t*, int, int32_t*) = liodom_graph_add_nodes;\n'
                   '  int (*ae)(liodom_graph_t*, const liodom_graph_edge_t*, int) = liodom_graph_add_edges;\n'
                   '  int (*sf)(liodom_graph_t*, int, int, const int32_t*) = liodom_graph_set_fixed;\n'
                   '  int (*gp)(liodom_graph_t*, int, int, double*) = liodom_graph_get_poses;\n'
                   '  int (*sp)(liodom_graph_t*, int, int, const double*) = liodom_graph_set_poses;\n'
                   '  int (*ge)(liodom_graph_t*, int, int, liodom_graph_edge_t*) = liodom_graph_get_edges;\n'
                   '  int (*li)(liodom_graph_t*, double*, double*, double*) = liodom_graph_linearize;\n'
                   '  int (*mu)(liodom_graph_t*, double, const double*, double*) = liodom_graph_multiply;\n'
                   '  void (*od)(liodom_graph_options_t*) = liodom_graph_options_default;\n'
                   '  int (*op)(liodom_graph_t*, const liodom_graph_options_t*, liodom_graph_report_t*) = liodom_graph_optimize;\n'
                   '  liodom_graph_edge_t e;\n'
                   '  e.i = e.j = e.kind = e.reserved = 0; e.z[6] = e.info[35] = 0.0;\n'
                   '  return cr && de && rs && cn && an && ae && sf && gp && sp && ge && li && mu && od && op && e.i == 0 &&\n'
                   '         LIODOM_GRAPH_TERM_GRADIENT == 0 && LIODOM_GRAPH_TERM_BREAKDOWN == 4; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                     'sizeof(liodom_graph_edge_t), offsetof(liodom_graph_edge_t, z), offsetof(liodom_graph_edge_t, info), '
                     'sizeof(liodom_graph_options_t), offsetof(liodom_graph_options_t, pcg_tolerance), sizeof(liodom_graph_report_t), '
                     'offsetof(liodom_graph_report_t, iterations)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [360, 16, 72, 32, 8, 48, 32]
    assert C.sizeof(api.GraphEdge) == 360 and api.GraphEdge.z.offset == 16 and api.GraphEdge.info.offset == 72
    d = api.GRAPH_EDGE_DTYPE
    assert d.itemsize == 360 and d.fields["z"][1] == 16 and d.fields["info"][1] == 72 and d.fields["kind"][1] == 8
    assert C.sizeof(api.GraphOptions) == 32 and api.GraphOptions.pcg_tolerance.offset == 8
    assert C.sizeof(api.GraphReport) == 48 and api.GraphReport.iterations.offset == 32


def test_the_default_options():
    o = api.make_graph_options()
    assert (o.max_iterations, o.max_pcg_iterations, o.pcg_tolerance, o.gradient_tolerance, o.cost_tolerance) == (20, 0, 1e-8, 1e-9, 1e-10)
    la.load().liodom_graph_options_default(None)
    e = api.graph_edges([0, 1], [1, 2], np.tile([0, 0, 0, 1, 1, 0, 0], (2, 1)), np.eye(6), kind=1)
    assert e.shape == (2,) and e["kind"].tolist() == [1, 1] and np.array_equal(e["info"][1], np.eye(6)) and e["reserved"].tolist() == [0, 0]


def test_argument_errors_that_need_no_device():
    L = la.load()
    g = C.c_void_p(0x1234)
    assert L.liodom_graph_create(8, 8, None) == api.ERR_INVALID_ARG
    for max_nodes, max_edges in ((0, 8), (8, 0), (-1, 8), (8, -1), (65537, 8), (8, 262145)):
        g = C.c_void_p(0x1234)
        assert L.liodom_graph_create(max_nodes, max_edges, C.byref(g)) == api.ERR_INVALID_ARG, (max_nodes, max_edges)
        assert not g.value and b"liodom_graph_create" in L.liodom_last_error()
    poses = np.array([[0, 0, 0, 1, 0, 0, 0]], np.float64)
    one = np.ones(1, np.int32)
    e = api.graph_edges([0], [1], poses, np.eye(6))
    n = C.c_int32()
    buf = np.zeros(64)
    assert L.liodom_graph_reset(None) == api.ERR_INVALID_ARG
    assert L.liodom_graph_count(None, C.byref(n), C.byref(n)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_add_nodes(None, api._dp(poses), None, 1, None) == api.ERR_INVALID_ARG
    assert b"liodom_graph_add_nodes" in L.liodom_last_error()
    assert L.liodom_graph_add_edges(None, e.ctypes.data_as(C.c_void_p), 1) == api.ERR_INVALID_ARG
    assert L.liodom_graph_set_fixed(None, 0, 1, api._ip(one)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_get_poses(None, 0, 1, api._dp(buf)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_set_poses(None, 0, 1, api._dp(poses)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_get_edges(None, 0, 1, e.ctypes.data_as(C.c_void_p)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_linearize(None, None, None, None) == api.ERR_INVALID_ARG
    assert L.liodom_graph_multiply(None, 0.0, api._dp(buf), api._dp(buf)) == api.ERR_INVALID_ARG
    assert L.liodom_graph_optimize(None, None, None) == api.ERR_INVALID_ARG
    assert b"liodom_graph_optimize" in L.liodom_last_error()
    L.liodom_graph_destroy(None)                    # a null graph is nothing to destroy
