"""liodom_mapper_options_t and the entry points that came with it (liodom_attach_mapper_ex, liodom_map_prune): exported by
libliodom_hip.so, the documented defaults, the struct's size in C and in the ctypes mirror.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_mapper_options_default", "liodom_attach_mapper_ex", "liodom_map_prune", "liodom_attach_mapper")


def test_new_symbols_are_exported():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS


def test_defaults_and_size():
    assert C.sizeof(api.MapperOptions) == 32
    o = api.MapperOptions(7, 7, 7, 7, 7, 7, (C.c_int32 * 2)(7, 7))
    la.load().liodom_mapper_options_default(C.byref(o))
    assert (o.cells_xy, o.cells_z, o.lag, o.prune_period, o.keep_cells_xy, o.keep_cells_z) == (2, 1, 0, 0, 0, 0)
    assert list(o.reserved) == [0, 0]
    la.load().liodom_mapper_options_default(None)      # a null pointer is ignored
    p = api.make_mapper_options(lag=1, prune_period=10, keep_cells_xy=3, keep_cells_z=2)
    assert (p.cells_xy, p.cells_z, p.lag, p.prune_period, p.keep_cells_xy, p.keep_cells_z) == (2, 1, 1, 10, 3, 2)


def test_struct_size_in_c(tmp_path):
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "liodom_hip.h"\n'
                     'int main(void) { printf("%zu %zu %zu\\n", sizeof(liodom_mapper_options_t), offsetof(liodom_mapper_options_t, lag),\n'
                     '  offsetof(liodom_mapper_options_t, keep_cells_xy)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "8", "16"]
    assert api.MapperOptions.lag.offset == 8 and api.MapperOptions.keep_cells_xy.offset == 16
