"""What an export and an import of a device map cost (the line in DESIGN.md §3): the maps left by the three cases of
tests/test_gpu_map.py::test_random_updates_bit_exact, HIP-event time around the kernels (the library reports it on stderr under
LIODOM_MAP_STATE_TIMING=1) and wall time of the C call.  Needs a GPU.

    python tools/map_state_cost.py [repeats]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["LIODOM_MAP_STATE_TIMING"] = "1"

import liodom_amd as la  # noqa: E402


def pose(yaw, t):
    T = np.eye(4)[:3].copy()
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:, 3] = t
    return T


def build(sizes):
    rng = np.random.default_rng(7)
    xy, z, res = sizes
    mg = la.Map(xy, z, res, max_cells=512, cell_capacity=32768, max_update_points=4096, max_modified_cells=128)
    for k in range(25):
        n = int(rng.integers(1, 3000))
        centres = rng.uniform(-30, 30, size=(40, 3)) * [1, 1, 0.2]
        pts = centres[rng.integers(0, 40, n)] + rng.normal(0, 0.35, size=(n, 3))
        pts[: n // 20] = np.round(pts[: n // 20] / res) * res
        x = np.zeros((n, 4), np.float32)
        x[:, :3] = pts
        x[:, 3] = rng.uniform(0, 100, n)
        mg.update(x, pose(0.02 * k, [0.8 * k, 0.1 * k, 0.01 * k]))
    return mg


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = la.load()
    for sizes in ((40.0, 50.0, 0.4), (10.0, 10.0, 0.25), (25.0, 30.0, 0.3)):
        mg = build(sizes)
        need = mg.state_size()
        buf = (C.c_ubyte * need)()
        n = C.c_int64(0)
        print("sizes %s: %d cells, %d points, blob %d bytes" % (sizes, mg.num_cells(), mg.all().shape[0], need), flush=True)
        mi = la.Map(*sizes, max_cells=512, cell_capacity=32768, max_update_points=4096, max_modified_cells=128)
        for r in range(repeats):
            sys.stderr.flush()
            t0 = time.perf_counter()
            rc = L.liodom_map_export_state(mg.h, buf, need, C.byref(n))
            t1 = time.perf_counter()
            assert rc == 0 and n.value == need
            blob = bytes(buf)
            t2 = time.perf_counter()
            rc = L.liodom_map_import_state(mi.h, blob, len(blob))
            t3 = time.perf_counter()
            assert rc == 0
            print("  repeat %d: export wall %.3f ms, import wall %.3f ms" % (r, 1e3 * (t1 - t0), 1e3 * (t3 - t2)), flush=True)
        assert mi.export_state() == blob
        mg.close(); mi.close()


if __name__ == "__main__":
    main()
