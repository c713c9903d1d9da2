"""The entry points of branch-and-bound relocalisation (liodom_pose_search_bnb_default, liodom_map_bound_nodes,
liodom_map_search_pose_bnb): exported by libliodom_hip.so and listed, the header still a C11 and a C++17 header with the signatures
given, the two new structs as large as their ctypes mirrors and the older ones untouched.  CPU only; no compute calls."""
import ctypes as C
import os
import subprocess

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("liodom_pose_search_bnb_default", "liodom_map_bound_nodes", "liodom_map_search_pose_bnb")
USE = ('#include <stddef.h>\n#include "liodom_hip.h"\n'
       'int f(void) {\n'
       '  void (*dflt)(liodom_pose_search_bnb_t*) = liodom_pose_search_bnb_default;\n'
       '  int (*bound)(liodom_map_t*, const float*, int, const double*, const double*, int, int, int, int32_t*) = liodom_map_bound_nodes;\n'
       '  int (*search)(liodom_map_t*, const float*, int, const liodom_pose_search_t*, const liodom_pose_search_bnb_t*, liodom_pose_search_result_t*,\n'
       '                liodom_pose_search_stats_t*) = liodom_map_search_pose_bnb;\n'
       '  liodom_pose_search_bnb_t o; liodom_pose_search_stats_t s;\n'
       '  o.batch = 0; o.reserved[6] = 0;\n'
       '  s.n_candidates = s.nodes_bounded = s.candidates_scored = 0; s.rounds = s.levels_built = 0; s.reserved[1] = 0;\n'
       '  return dflt != NULL && bound != NULL && search != NULL && o.batch == s.rounds; }\n')


def test_new_symbols_are_exported_and_listed():
    la.build()
    L = C.CDLL(la.lib_path())
    for name in NEW:
        assert hasattr(L, name), "missing export: " + name
        assert name in api.EXPORTED_SYMBOLS
    for name in ("bound_nodes", "search_pose_bnb", "search_pose", "score_poses"):
        assert callable(getattr(api.Map, name))
    opt = api.PoseSearchBnb()
    opt.batch = -5
    api.load().liodom_pose_search_bnb_default(C.byref(opt))
    assert opt.batch == 1024 and not any(opt.reserved)
    api.load().liodom_pose_search_bnb_default(None)      # a null is ignored


def test_header_is_c11_and_cxx17_and_the_structs_keep_their_sizes(tmp_path):
    inc = os.path.join(ROOT, "include")
    use = tmp_path / "use.c"
    use.write_text(USE)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(use), "-o", str(tmp_path / "use.o")])
    usepp = tmp_path / "use.cc"
    usepp.write_text(USE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-I", inc, "-c", str(usepp), "-o", str(tmp_path / "usepp.o")])
    probe = tmp_path / "sz.c"
    probe.write_text('#include <stdio.h>\n#include "liodom_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(liodom_pose_search_bnb_t), '
                     'sizeof(liodom_pose_search_stats_t), sizeof(liodom_pose_search_t), sizeof(liodom_pose_search_result_t)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", inc, str(probe), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(api.PoseSearchBnb), C.sizeof(api.PoseSearchStats), C.sizeof(api.PoseSearch), C.sizeof(api.PoseSearchResult)]
    assert sizes == [32, 40, 112, 168]
