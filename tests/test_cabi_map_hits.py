"""The entry points of the per-scan map-hit records (liodom_set_map_hits, liodom_get_map_hit_log, liodom_map_hit_rows): exported by
libliodom_hip.so and listed, the header still a C11 header with the signatures given, liodom_map_hit_t 128 bytes as its ctypes and
NumPy mirrors are, and the argument errors that need no device.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import numpy as np

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_set_map_hits", "liodom_get_map_hit_log", "liodom_map_hit_rows")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("set_map_hits", "map_hits", "localize_scan"):
        assert callable(getattr(la.Liodom, name))
    assert callable(api.Map.hit_rows)


def test_header_is_c11_and_the_record_is_128_bytes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  int (*set)(liodom_handle_t*, int, int) = liodom_set_map_hits;\n'
                   '  int (*get)(liodom_handle_t*, int, int, int, liodom_map_hit_t*) = liodom_get_map_hit_log;\n'
                   '  int (*rows)(liodom_map_t*, const float*, int64_t, const int32_t*, const double*, int, int, int32_t*) = liodom_map_hit_rows;\n'
                   '  liodom_map_hit_t r;\n'
                   '  r.scan_index = r.n_edges = r.hits_r = r.hits_0 = r.radius = 0; r.reserved[1] = 0; r.T[11] = 0.0;\n'
                   '  r.flags = LIODOM_HIT_VALID | LIODOM_HIT_NO_READER | LIODOM_HIT_NO_SOLVE;\n'
                   '  return set != NULL && get != NULL && rows != NULL && r.flags == 7u; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(liodom_map_hit_t), '
                     'offsetof(liodom_map_hit_t, hits_0), offsetof(liodom_map_hit_t, radius), offsetof(liodom_map_hit_t, T)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [128, 16, 20, 32]
    assert C.sizeof(api.MapHit) == 128 and api.MapHit.hits_0.offset == 16 and api.MapHit.radius.offset == 20 and api.MapHit.T.offset == 32
    d = api.MAP_HIT_DTYPE
    assert d.itemsize == 128 and d.fields["hits_0"][1] == 16 and d.fields["radius"][1] == 20 and d.fields["T"][1] == 32
    assert (api.HIT_VALID, api.HIT_NO_READER, api.HIT_NO_SOLVE) == (1, 2, 4)


def test_argument_errors_that_need_no_device():
    L = la.load()
    rec = (api.MapHit * 2)()
    assert L.liodom_set_map_hits(None, 0, 1) == api.ERR_INVALID_ARG
    assert L.liodom_get_map_hit_log(None, 0, 0, 1, C.cast(rec, C.c_void_p)) == api.ERR_INVALID_ARG
    e = np.zeros((4, 4), np.float32)
    n = np.array([2, 2], np.int32)
    T = np.tile(np.eye(4)[:3].reshape(12), (2, 1))
    hits = np.zeros((2, 2), np.int32)
    assert L.liodom_map_hit_rows(None, api._fp(e), 2, api._ip(n), api._dp(T), 2, 1, api._ip(hits)) == api.ERR_INVALID_ARG
    assert b"liodom_map_hit_rows" in L.liodom_last_error()
