"""The entry points of map registration (liodom_map_register_default, liodom_map_register_poses): exported by libliodom_hip.so and
listed, the header still a C11 and a C++17 header with the signatures given, the two new structs as large as their ctypes mirrors
and laid out as documented, the defaults, and the argument errors that need no device.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import pytest

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_map_register_default", "liodom_map_register_poses")
USE = ('#include <stddef.h>\n#include "liodom_hip.h"\n'
       'int f(void) {\n'
       '  void (*dflt)(liodom_map_register_t*) = liodom_map_register_default;\n'
       '  int (*reg)(liodom_map_t*, const float*, int, const double*, int, const liodom_map_register_t*, liodom_map_registration_t*, int32_t*) =\n'
       '      liodom_map_register_poses;\n'
       '  liodom_map_register_t o; liodom_map_registration_t r;\n'
       '  o.cells_xy = o.cells_z = o.max_passes = o.min_matches = o.local_capacity = o.reserved = 0;\n'
       '  o.stop_translation = o.stop_rotation = o.min_range = o.max_range = 0.0;\n'
       '  r.pose[6] = r.information[35] = r.final_cost = r.sigma2 = r.last_move_t = r.last_move_r = 0.0;\n'
       '  r.termination = LIODOM_REG_CONVERGED + LIODOM_REG_MAX_PASSES + LIODOM_REG_FEW_MATCHES + LIODOM_REG_NO_MAP + LIODOM_REG_EVAL_FAILURE;\n'
       '  r.passes = r.matches = r.n_residuals = r.local_points = 0; r.cov_flags = LIODOM_COV_VALID; r.last_lm.termination = 0;\n'
       '  return dflt != NULL && reg != NULL && o.reserved == r.passes && r.termination == 10; }\n')


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    assert callable(api.Map.register_poses) and la.RegisterOptions is api.RegisterOptions and la.Registration is api.Registration


def test_header_is_c11_and_cxx17_and_the_structs_have_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    for name, cc, std in (("use.c", "gcc", "-std=c11"), ("use.cc", "g++", "-std=c++17")):
        f = tmp_path / name
        f.write_text(USE)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(f), "-o", str(tmp_path / (name + ".o"))])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                     'sizeof(liodom_map_register_t), offsetof(liodom_map_register_t, stop_translation), sizeof(liodom_map_registration_t), '
                     'offsetof(liodom_map_registration_t, information), offsetof(liodom_map_registration_t, termination), '
                     'offsetof(liodom_map_registration_t, cov_flags), offsetof(liodom_map_registration_t, last_lm), sizeof(liodom_lm_trace_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [56, 24, 432, 56, 376, 396, 400, 32]
    assert C.sizeof(api.RegisterOptions) == 56 and api.RegisterOptions.stop_translation.offset == 24
    assert C.sizeof(api.Registration) == 432 and api.Registration.information.offset == 56 and api.Registration.termination.offset == 376
    assert api.Registration.cov_flags.offset == 396 and api.Registration.last_lm.offset == 400 and C.sizeof(api.LmTrace) == 32


def test_the_defaults():
    o = api.RegisterOptions()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    api.load().liodom_map_register_default(C.byref(o))
    assert (o.cells_xy, o.cells_z, o.max_passes, o.min_matches, o.local_capacity, o.reserved) == (2, 1, 10, 6, 0, 0)
    assert (o.stop_translation, o.stop_rotation, o.min_range, o.max_range) == (1e-4, 1e-5, 3.0, 75.0)
    api.load().liodom_map_register_default(None)      # a null is ignored
    o = api.make_register_options(max_passes=3, stop_rotation=1e-7, local_capacity=2048)
    assert (o.max_passes, o.stop_rotation, o.local_capacity, o.cells_xy) == (3, 1e-7, 2048, 2)
    with pytest.raises(KeyError):
        api.make_register_options(passes=3)
    assert (api.REG_CONVERGED, api.REG_MAX_PASSES, api.REG_FEW_MATCHES, api.REG_NO_MAP, api.REG_EVAL_FAILURE) == (0, 1, 2, 3, 4)


def test_a_null_map_is_refused_before_any_device_call():
    L = api.load()
    out = (api.Registration * 1)()
    before = bytes(out)
    poses = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    assert L.liodom_map_register_poses(None, None, 0, poses, 1, None, out, None) == -1
    assert b"liodom_map_register_poses" in L.liodom_last_error() and bytes(out) == before
