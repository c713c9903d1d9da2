"""The robust-loss entry points of the pose graph (liodom_graph_set_loss, _get_loss, _set_edge_active, _get_edge_active,
_edge_weights): exported by libliodom_hip.so and listed, the header still a C11 header with the signatures given and the loss
numbers, the struct sizes unchanged, and the argument errors that need no device.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_graph_set_loss", "liodom_graph_get_loss", "liodom_graph_set_edge_active", "liodom_graph_get_edge_active",
       "liodom_graph_edge_weights")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("set_loss", "loss", "set_edge_active", "edge_active", "edge_weights"):
        assert callable(getattr(api.PoseGraph, name))
    assert api.GRAPH_LOSSES == ("none", "huber", "cauchy", "geman_mcclure")


def test_header_is_c11_and_the_structs_keep_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  int (*sl)(liodom_graph_t*, int, int, double) = liodom_graph_set_loss;\n'
                   '  int (*gl)(liodom_graph_t*, int, int32_t*, double*) = liodom_graph_get_loss;\n'
                   '  int (*sa)(liodom_graph_t*, int, int, const int32_t*) = liodom_graph_set_edge_active;\n'
                   '  int (*ga)(liodom_graph_t*, int, int, int32_t*) = liodom_graph_get_edge_active;\n'
                   '  int (*ew)(liodom_graph_t*, double*, double*) = liodom_graph_edge_weights;\n'
                   '  return sl && gl && sa && ga && ew && LIODOM_GRAPH_LOSS_NONE == 0 && LIODOM_GRAPH_LOSS_HUBER == 1 &&\n'
                   '         LIODOM_GRAPH_LOSS_CAUCHY == 2 && LIODOM_GRAPH_LOSS_GEMAN_MCCLURE == 3; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                     'sizeof(liodom_graph_options_t), sizeof(liodom_graph_report_t), sizeof(liodom_graph_edge_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [32, 48, 360]
    assert (C.sizeof(api.GraphOptions), C.sizeof(api.GraphReport), C.sizeof(api.GraphEdge)) == (32, 48, 360)


def test_argument_errors_that_need_no_device():
    L = la.load()
    one = np.ones(1, np.int32)
    buf = np.zeros(8)
    l, c = C.c_int32(7), C.c_double(7.0)
    assert L.liodom_graph_set_loss(None, 1, 3, 5.0) == api.ERR_INVALID_ARG
    assert b"liodom_graph_set_loss" in L.liodom_last_error()
    assert L.liodom_graph_get_loss(None, 1, C.byref(l), C.byref(c)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_get_loss" in L.liodom_last_error() and (l.value, c.value) == (7, 7.0)
    assert L.liodom_graph_set_edge_active(None, 0, 1, api._ip(one)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_set_edge_active" in L.liodom_last_error()
    assert L.liodom_graph_get_edge_active(None, 0, 1, api._ip(one)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_get_edge_active" in L.liodom_last_error()
    assert L.liodom_graph_edge_weights(None, api._dp(buf), api._dp(buf)) == api.ERR_INVALID_ARG
    assert b"liodom_graph_edge_weights" in L.liodom_last_error()
    assert np.all(buf == 0.0) and one[0] == 1


def test_a_loss_name_is_checked_before_the_library_is_asked():
    class Fake(api.PoseGraph):
        def __init__(self):
            self.h = None
    g = Fake()
    try:
        g.set_loss(1, "tukey", 1.0)
    except ValueError as e:
        assert "tukey" in str(e)
    else:
        raise AssertionError("an unknown loss name was taken")
