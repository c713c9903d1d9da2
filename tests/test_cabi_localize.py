"""The entry points of localisation in a saved map (liodom_seed_stream, liodom_attach_map_reader, liodom_map_get_local_batch):
exported by libliodom_hip.so and listed, the header still a C11 header, and liodom_mapper_options_t untouched (the reader is an
entry point of its own, not a field of that struct).  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_seed_stream", "liodom_attach_map_reader", "liodom_map_get_local_batch")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("seed_stream", "attach_map_reader"):
        assert callable(getattr(la.Liodom, name))
    assert callable(api.Map.get_local_batch)


def test_header_is_c11_and_the_options_struct_keeps_its_size(tmp_path):
    inc = os.path.join(ROOT, "include")
    # the declarations, with the signatures the issue gives, as strict C11
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  int (*seed)(liodom_handle_t*, int, const double*) = liodom_seed_stream;\n'
                   '  int (*reader)(liodom_handle_t*, int, liodom_map_t*, int, int) = liodom_attach_map_reader;\n'
                   '  int (*batch)(liodom_map_t*, const double*, int, int, int, float*, int64_t, int64_t*) = liodom_map_get_local_batch;\n'
                   '  return seed != NULL && reader != NULL && batch != NULL; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu\\n", sizeof(liodom_mapper_options_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32"]
    assert C.sizeof(api.MapperOptions) == 32
