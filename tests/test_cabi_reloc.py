"""The entry points of relocalisation (liodom_map_score_poses, liodom_pose_search_default, liodom_map_search_pose): exported by
libliodom_hip.so and listed, the header still a C11 header with the signatures given, the two new structs as large as their ctypes
mirrors, and liodom_mapper_options_t untouched.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_map_score_poses", "liodom_pose_search_default", "liodom_map_search_pose")


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("score_poses", "search_pose"):
        assert callable(getattr(api.Map, name))
    assert callable(la.Liodom.relocalize)


def test_header_is_c11_and_the_structs_keep_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text('#include <stddef.h>\n#include "liodom_hip.h"\n'
                   'int f(void) {\n'
                   '  int (*score)(liodom_map_t*, const float*, int, const double*, int, int, int32_t*) = liodom_map_score_poses;\n'
                   '  void (*dflt)(liodom_pose_search_t*) = liodom_pose_search_default;\n'
                   '  int (*search)(liodom_map_t*, const float*, int, const liodom_pose_search_t*, liodom_pose_search_result_t*, double*, int32_t*) = liodom_map_search_pose;\n'
                   '  liodom_pose_search_t s; liodom_pose_search_result_t r;\n'
                   '  s.centre[6] = 0.0; s.step_xy = s.step_z = s.step_yaw = 0.0; s.nx = s.ny = s.nz = s.nyaw = s.radius = 0; s.reserved[2] = 0;\n'
                   '  r.best_index = r.hits_r = r.hits_0 = r.n_candidates = 0; r.pose[6] = 0.0; r.T[11] = 0.0;\n'
                   '  return score != NULL && dflt != NULL && search != NULL && s.nx == r.hits_0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(liodom_pose_search_t), '
                     'sizeof(liodom_pose_search_result_t), sizeof(liodom_mapper_options_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(api.PoseSearch), C.sizeof(api.PoseSearchResult), 32]
    assert sizes[:2] == [112, 168] and C.sizeof(api.MapperOptions) == 32
