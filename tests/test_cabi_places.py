"""The entry points of the place database (liodom_places_*): exported by libliodom_hip.so and listed, the header still a C11 header
with the signatures given, liodom_place_geometry_t 40 bytes and liodom_place_match_t 136 bytes as their ctypes and NumPy mirrors
are, and the argument errors that need no device.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_place_geometry_default", "liodom_places_create", "liodom_places_destroy", "liodom_places_count", "liodom_places_reset",
       "liodom_places_describe", "liodom_places_add", "liodom_places_query", "liodom_places_query_desc", "liodom_places_state_size",
       "liodom_places_export_state", "liodom_places_import_state")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("describe", "add", "query", "query_desc", "export_state", "import_state", "reset", "count"):
        assert callable(getattr(api.Places, name))
    for name in ("add_place", "relocalize_global"):
        assert callable(getattr(la.Liodom, name))
    assert callable(api.parse_place_state) and callable(api.build_place_state) and callable(api.PlacePolicy(1.0).feed)
    for src in ("kernels_places.h", "liodom_places_host.h", "place_state_format.h"):      # a change to any of them rebuilds the library
        assert any(p.endswith(os.sep + src) for p in api._SRC), src


def test_header_is_c11_and_the_structs_have_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  void (*gd)(liodom_place_geometry_t*) = liodom_place_geometry_default;\n'
                   '  int (*cr)(const liodom_place_geometry_t*, int, int, liodom_places_t**) = liodom_places_create;\n'
                   '  void (*de)(liodom_places_t*) = liodom_places_destroy;\n'
                   '  int (*cn)(liodom_places_t*, int32_t*) = liodom_places_count;\n'
                   '  int (*rs)(liodom_places_t*) = liodom_places_reset;\n'
                   '  int (*ds)(liodom_places_t*, const float*, int64_t, const int32_t*, int, uint64_t*, int32_t*) = liodom_places_describe;\n'
                   '  int (*ad)(liodom_places_t*, const float*, int, const double*, int64_t, int32_t*) = liodom_places_add;\n'
                   '  int (*qu)(liodom_places_t*, const float*, int64_t, const int32_t*, int, int, liodom_place_match_t*, int32_t*) = liodom_places_query;\n'
                   '  int (*qd)(liodom_places_t*, const uint64_t*, int, int, liodom_place_match_t*) = liodom_places_query_desc;\n'
                   '  int (*sz)(liodom_places_t*, int64_t*) = liodom_places_state_size;\n'
                   '  int (*ex)(liodom_places_t*, void*, int64_t, int64_t*) = liodom_places_export_state;\n'
                   '  int (*im)(liodom_places_t*, const void*, int64_t) = liodom_places_import_state;\n'
                   '  liodom_place_match_t m;\n'
                   '  m.index = m.distance = m.shift = m.bits_place = 0; m.id = 0; m.pose[6] = m.place_pose[6] = 0.0;\n'
                   '  return gd && cr && de && cn && rs && ds && ad && qu && qd && sz && ex && im && m.index == 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                     'sizeof(liodom_place_geometry_t), offsetof(liodom_place_geometry_t, r_max), sizeof(liodom_place_match_t), '
                     'offsetof(liodom_place_match_t, id), offsetof(liodom_place_match_t, pose), offsetof(liodom_place_match_t, place_pose)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [40, 8, 136, 16, 24, 80]
    assert C.sizeof(api.PlaceGeometry) == 40 and api.PlaceGeometry.r_max.offset == 8
    assert C.sizeof(api.PlaceMatch) == 136 and api.PlaceMatch.id.offset == 16 and api.PlaceMatch.pose.offset == 24 and api.PlaceMatch.place_pose.offset == 80
    d = api.PLACE_MATCH_DTYPE
    assert d.itemsize == 136 and d.fields["id"][1] == 16 and d.fields["pose"][1] == 24 and d.fields["place_pose"][1] == 80
    assert api.PLACE_RECORD_DTYPE.itemsize == api.PLACE_RECORD_BYTES == 72


def test_the_default_geometry():
    g = api.PlaceGeometry()
    la.load().liodom_place_geometry_default(C.byref(g))
    assert (g.n_rings, g.n_layers, g.r_max, g.z_min, g.z_max, g.reserved) == (16, 4, 80.0, -4.0, 12.0, 0)
    assert api.place_geometry() == (16, 4, 80.0, -4.0, 12.0)


def test_argument_errors_that_need_no_device():
    L = la.load()
    u64p = C.POINTER(C.c_uint64)
    g = api.PlaceGeometry()
    L.liodom_place_geometry_default(C.byref(g))
    db = C.c_void_p(0x1234)
    assert L.liodom_places_create(None, 8, 8, C.byref(db)) == api.ERR_INVALID_ARG
    assert L.liodom_places_create(C.byref(g), 8, 8, None) == api.ERR_INVALID_ARG
    for field, value in (("n_rings", 0), ("n_rings", 17), ("n_layers", -1), ("r_max", 0.0), ("r_max", float("nan")), ("z_min", 12.0), ("z_max", float("inf"))):
        h = api.PlaceGeometry()
        L.liodom_place_geometry_default(C.byref(h))
        setattr(h, field, value)
        db = C.c_void_p(0x1234)
        assert L.liodom_places_create(C.byref(h), 8, 8, C.byref(db)) == api.ERR_INVALID_ARG, (field, value)
        assert not db.value and b"liodom_places_create" in L.liodom_last_error()
    for max_places, max_edges in ((0, 8), ((1 << 20) + 1, 8), (8, 0), (-1, 8), (8, -1)):
        assert L.liodom_places_create(C.byref(g), max_places, max_edges, C.byref(db)) == api.ERR_INVALID_ARG
    e = np.zeros((4, 4), np.float32)
    n = np.array([2, 2], np.int32)
    desc = np.zeros((2, 64), np.uint64)
    out = np.zeros((2, 3), api.PLACE_MATCH_DTYPE)
    pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    cnt, size = C.c_int32(), C.c_int64()
    assert L.liodom_places_count(None, C.byref(cnt)) == api.ERR_INVALID_ARG
    assert L.liodom_places_reset(None) == api.ERR_INVALID_ARG
    assert L.liodom_places_describe(None, api._fp(e), 2, api._ip(n), 2, desc.ctypes.data_as(u64p), None) == api.ERR_INVALID_ARG
    assert b"liodom_places_describe" in L.liodom_last_error()
    assert L.liodom_places_add(None, api._fp(e), 4, api._dp(pose), 0, None) == api.ERR_INVALID_ARG
    assert L.liodom_places_query(None, api._fp(e), 2, api._ip(n), 2, 3, out.ctypes.data_as(C.c_void_p), None) == api.ERR_INVALID_ARG
    assert b"liodom_places_query" in L.liodom_last_error()
    assert L.liodom_places_query_desc(None, desc.ctypes.data_as(u64p), 2, 3, out.ctypes.data_as(C.c_void_p)) == api.ERR_INVALID_ARG
    assert L.liodom_places_state_size(None, C.byref(size)) == api.ERR_INVALID_ARG
    assert L.liodom_places_export_state(None, None, 0, C.byref(size)) == api.ERR_INVALID_ARG
    assert L.liodom_places_import_state(None, b"x", 1) == api.ERR_INVALID_ARG
    L.liodom_places_destroy(None)                   # a null database is nothing to destroy
