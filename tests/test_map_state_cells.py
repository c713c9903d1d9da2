"""map_state_split / map_state_join (liodom_amd/csrc/map_state_cells.h: the plain-C++ blob handling of liodom::MapPager) in a
program of their own under host sanitizers; no GPU, nothing sanitized is loaded into Python."""
import os
import re
import shutil
import subprocess

import numpy as np

from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_and_join_stand_alone_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    exe = str(tmp_path / "map_state_cells")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-Wall", "-Wextra", "-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "map_state_cells_main.cc")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    xy, z, res = 40.0, 50.0, 0.4
    rng = np.random.default_rng(1)
    cells = []
    for i, n in enumerate((3, 7, 1, 5)):
        p = rng.uniform(0.5, 9.5, (n, 4)).astype(np.float32)
        p[:, 0] += i * xy
        cells.append(p)
    good = tmp_path / "good.mapstate"
    good.write_bytes(api.build_map_state(xy, z, res, cells, status=8))
    r = subprocess.run([exe, str(good)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"map_state_cells: \d{3,} cases, 0 failures", r.stdout), r.stdout
