#!/usr/bin/env python3
"""What paging the mapper's map costs.  Needs a GPU.

1. One evict and one merge on designed maps: `--cells` cells of `--points` points each, every other cell outside the keep box.
   HIP-event time around the kernels (the library reports it on stderr under LIODOM_MAP_STATE_TIMING=1, as the blob calls do) and
   wall time of the C call, median of `--repeats` rounds; every round re-imports the map.
2. The per-scan cost of a pager step on the mapper shape of tools/mapper_step_cost.py (mapping handle, one stream, 64 x 1800,
   R = 8, epr = 10, prev_frames = 15, lag 1): P + 10 scans untimed, then `--scans` timed scans with the pose read back after every
   scan (the pager needs it), one child process per leg and round.  Legs:
     p  prune_period = 1, keep box (2, 1): the on-device prune of every scan (what the parent commit offers)
     q  no auto-prune, MapPager(keep 3, 1; load 3, 1).step(pose) after every scan
   With --parent-tree DIR (a checkout of the parent commit, built) leg p also runs from that tree in every round.
Writes everything as JSON to --out and prints the table.
usage: tools/map_paging_cost.py [--parent-tree DIR] [--repeats 7] [--scans 200] [--out profiles/map_paging_cost.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, R, EPR, P = 64, 1800, 8, 10, 15
N = H * W
SIZES = (40.0, 50.0, 0.4)


def calls_worker(n_cells, n_points, repeats):
    """Part 1; the library's timer lines go to stderr, this prints the wall times and the sizes as one JSON line."""
    os.environ["LIODOM_MAP_STATE_TIMING"] = "1"
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api
    xy, z, res = SIZES
    side = int(np.ceil(n_points ** (1.0 / 3.0)))
    i = np.arange(n_points)
    base = np.zeros((n_points, 4), np.float32)
    base[:, 0], base[:, 1], base[:, 2] = res * (1.5 + i % side), res * (1.5 + (i // side) % side), res * (1.5 + i // (side * side))
    cells = []
    for c in range(n_cells):               # even cells far away along x (outside), odd ones in a column along y (inside)
        p = base.copy()
        p[:, 0] += (1000 + c) * xy if c % 2 == 0 else 0.0
        p[:, 1] += 0.0 if c % 2 == 0 else (c // 2 - n_cells // 4) * xy
        p[:, 3] = c
        cells.append(p)
    blob = api.build_map_state(xy, z, res, cells)
    m = la.Map(xy, z, res, max_cells=n_cells, cell_capacity=n_points, max_update_points=64, max_modified_cells=8)
    L = la.load()
    T = np.ascontiguousarray(np.eye(4)[:3], np.float64).reshape(12)
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    keep = n_cells
    wall = dict(evict=[], merge=[])
    tile_bytes = 0
    for r in range(repeats + 1):           # round 0 warms up (allocations of the first call)
        m.import_state(blob)
        need, n = C.c_int64(0), C.c_int32(0)
        assert L.liodom_map_evict(m.h, Tp, keep, 0, None, 0, C.byref(need), C.byref(n)) == api.ERR_CAPACITY
        buf = (C.c_ubyte * need.value)()
        sys.stderr.write("ROUND %d\n" % r); sys.stderr.flush()
        t0 = time.perf_counter()
        rc = L.liodom_map_evict(m.h, Tp, keep, 0, buf, need.value, C.byref(need), C.byref(n))
        t1 = time.perf_counter()
        assert rc == 0 and n.value == (n_cells + 1) // 2, (rc, n.value, L.liodom_last_error())
        tile = bytes(buf)
        tile_bytes = len(tile)
        t2 = time.perf_counter()
        rc = L.liodom_map_merge_state(m.h, tile, len(tile), None, C.byref(n))
        t3 = time.perf_counter()
        assert rc == 0 and n.value == (n_cells + 1) // 2 and m.num_cells() == n_cells, (rc, n.value, L.liodom_last_error())
        if r:
            wall["evict"].append(1e3 * (t1 - t0)); wall["merge"].append(1e3 * (t3 - t2))
    m.close()
    print("RESULT " + json.dumps(dict(wall_ms=wall, tile_bytes=tile_bytes, cells=n_cells, points_per_cell=n_points)), flush=True)


def step_worker(tree, leg, scans_file, n_timed):
    """Part 2, one leg with the package of `tree`."""
    sys.path.insert(0, tree)
    import numpy as np
    import liodom_amd as la
    scans = np.load(scans_file, mmap_mode="r")
    K = scans.shape[0]
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                  la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8))
    m = la.Map(max_cells=1024, cell_capacity=16384)
    pager = None
    if leg == "p":
        g.attach_mapper(m, 2, 1, lag=1, prune_period=1, keep_cells_xy=2, keep_cells_z=1)
    else:
        from liodom_amd.pager import MapPager
        g.attach_mapper(m, 2, 1, lag=1)
        pager = MapPager(m, 3, 1, 3, 1)
    g.alloc_resident(K)
    for k in range(K):
        g.upload_scan(0, k, scans[k])
    g.sync()

    def T34(pq):
        qx, qy, qz, qw = pq[:4]
        return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw), pq[4]],
                         [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw), pq[5]],
                         [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy), pq[6]]])

    def run(lo, hi):
        for k in range(lo, hi):
            poses, _ = g.process_resident(k, N, H, W, readback=True, next_slot=(k + 1 if k + 1 < K else -1))
            if pager is not None:
                pager.step(T34(np.asarray(poses).reshape(-1, 7)[0]))
    pre = K - n_timed
    run(0, pre)
    g.sync()
    t0 = time.perf_counter()
    run(pre, K)
    g.sync()
    dt = (time.perf_counter() - t0) / n_timed
    out = dict(s_per_scan=dt, cells=m.num_cells(), map_status=m.status(), modes=g.modes())
    if pager is not None:
        out.update(evicted=pager.evicted, loaded=pager.loaded, conflicts=pager.conflicts, stored=len(pager.store))
    g.attach_mapper(None)
    m.close(); g.close()
    print("RESULT " + json.dumps(out), flush=True)


def child(args, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError("worker failed: %s\n%s" % (args, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--leg", default="")
    ap.add_argument("--scans-file", default="")
    a = ap.parse_args()
    if a.worker == "calls":
        return calls_worker(a.cells, a.points, a.repeats)
    if a.worker == "step":
        return step_worker(a.tree, a.leg, a.scans_file, a.scans)
    med = statistics.median
    # 1. the two calls
    shapes = [(64, 256), (a.cells, a.points)]
    calls = []
    for n_cells, n_points in shapes:
        res, err = child(["--worker", "calls", "--cells", str(n_cells), "--points", str(n_points), "--repeats", str(a.repeats)])
        kern = dict(evict=[], merge=[])
        rnd = 0
        for ln in err.splitlines():
            if ln.startswith("ROUND "):
                rnd = int(ln[6:])
            f = re.match(r"liodom_map_(evict|merge_state): kernels ([0-9.]+) ms", ln)
            if f and rnd > 0:
                kern["evict" if f.group(1) == "evict" else "merge"].append(float(f.group(2)))
        # (the size query of an evict returns before its timer is stopped and prints nothing)
        res["kernel_ms"] = kern
        calls.append(res)
        print("evict + merge of %d of %d cells x %d points (tile %.2f MB): evict kernels %.3f ms, wall %.3f ms; merge kernels %.3f ms, wall %.3f ms  (median of %d)" % (
            (n_cells + 1) // 2, n_cells, n_points, res["tile_bytes"] / 1e6, med(kern["evict"]), med(res["wall_ms"]["evict"]), med(kern["merge"]),
            med(res["wall_ms"]["merge"]), a.repeats), flush=True)
    # 2. the pager step on the mapper shape
    sys.path.insert(0, ROOT)
    import numpy as np
    from liodom_amd import synth
    cfg = synth.make_cfg(H, W, 0)
    K = P + 10 + a.scans
    samples, last = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        scans_file = os.path.join(tmp, "scans.npy")
        np.save(scans_file, np.stack([synth.scan(cfg, 0, k)[0].astype(np.float32).reshape(-1, 4) for k in range(K)]))
        legs = [("this:p", ROOT, "p"), ("this:q", ROOT, "q")] + ([("parent:p", os.path.abspath(a.parent_tree), "p")] if a.parent_tree else [])
        for r in range(a.repeats):
            for name, tree, leg in (legs if r % 2 == 0 else legs[::-1]):
                res, _ = child(["--worker", "step", "--tree", tree, "--leg", leg, "--scans-file", scans_file, "--scans", str(a.scans)])
                samples.setdefault(name, []).append(res["s_per_scan"] * 1e6)
                last[name] = res
    rows = {}
    print("# mapping handle, 64x1800 R=8 epr=10 P=%d lag 1, pose read back every scan, %d timed scans, %d repeats: us/scan median (min .. max)" % (P, a.scans, a.repeats))
    for key, xs in samples.items():
        rows[key] = dict(median_us=med(xs), min_us=min(xs), max_us=max(xs), samples_us=xs, **{k: v for k, v in last[key].items() if k != "s_per_scan"})
        print("%-9s %9.2f (%9.2f .. %9.2f)  cells %4d  %s" % (key, rows[key]["median_us"], min(xs), max(xs), last[key]["cells"],
                                                              " ".join("%s=%s" % (k, last[key][k]) for k in ("evicted", "loaded", "conflicts", "stored") if k in last[key])))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(calls=calls, step=dict(shape=dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, prev_frames=P, timed_scans=a.scans, repeats=a.repeats),
                                                  legs=dict(p="lag 1, prune_period 1, keep (2, 1)", q="lag 1, MapPager(keep 3, 1; load 3, 1) after every scan"),
                                                  results=rows)), f, indent=1)


if __name__ == "__main__":
    main()
