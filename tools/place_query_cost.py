#!/usr/bin/env python3
"""What the place database costs per call, and what finding a scan without a prior costs with and without it.  Needs a GPU.
One job, one child process per row (each under its own time limit), wall time of the whole call, median over `--repeats` calls.

  rows      liodom_places_describe, _add, _query and _query_desc at 1 024 / 32 768 / 262 144 places (4 096 synthetic descriptors of
            the circle's bit density — about 3 % of the bits — repeated), 1 and 64 queries of 480 edges, k = 3, the default
            geometry (W = 64) and a 8 x 2 one (W = 16).  The kernels' share of a call comes from a kernel trace of one row's child,
            in a run of its own: rocprofv3 --kernel-trace --stats -- python3 tools/place_query_cost.py --row 16x4 262144 64
            (profiles/place_kernel_trace.txt; tools/rocprof_summary.py reads the trace).
  circle    the same scan (scan 205 of the circle of tests/place_model.py, turned by 2.5 rad) found two ways in the site map of its
            first lap: (a) liodom_map_search_pose_bnb over +-40 m and every heading at 0.4 m / 0.02 rad from the circle's centre —
            the only means without a prior before the database; (b) liodom_places_query with k = 3 plus the two small levels of
            tests/test_gpu_places.py around each match.  Both times and both results are recorded.
usage: tools/place_query_cost.py [--repeats 20] [--out profiles/place_query_cost.json]"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLACES = (1024, 32768, 262144)
QUERIES = (1, 64)
GEOMS = {"16x4": dict(), "8x2": dict(n_rings=8, n_layers=2)}
N_EDGES, K = 480, 3
LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=8, ny=8, nyaw=7), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]
WIDE = dict(step_xy=0.4, step_yaw=0.02, nx=100, ny=100, nyaw=157)      # 201 x 201 x 315 candidates


def _timed(call, repeats):
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e6)
    return r, wall


def row_worker(geom, places, queries, repeats):
    sys.path.insert(0, ROOT)
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api
    rng = np.random.default_rng(1)
    db = la.Places(max_places=places + repeats + 8, max_edges=1024, **GEOMS[geom])
    W = db.words
    base = rng.integers(0, 1 << 63, (5, 4096, W), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (5, 4096, W), dtype=np.uint64)
    desc = np.tile(base[0] & base[1] & base[2] & base[3] & base[4], (places // 4096 + 1, 1))[:places]      # (1 / 2)^5: 3 % of the bits
    poses = np.zeros((places, 7))
    poses[:, 3] = 1.0
    db.import_state(api.build_place_state(db.geometry, desc, np.arange(places), poses))
    g = db.geometry
    clouds = []
    for _ in range(queries):
        p = np.zeros((N_EDGES, 4), np.float32)
        p[:, :2] = rng.uniform(-0.6 * g[2], 0.6 * g[2], (N_EDGES, 2))
        p[:, 2] = rng.uniform(g[3], g[4], N_EDGES)
        clouds.append(p)
    qdesc, _ = db.describe(clouds)                  # (the first calls allocate the staging)
    db.query(clouds, K); db.query_desc(qdesc, K)
    out = dict(geometry=geom, words=W, places=places, queries=queries, bits_per_place=float(np.bitwise_count(desc[:4096]).sum(axis=1).mean()))
    _, out["describe_us"] = _timed(lambda: db.describe(clouds), repeats)
    a, out["query_us"] = _timed(lambda: db.query(clouds, K), repeats)
    b, out["query_desc_us"] = _timed(lambda: db.query_desc(qdesc, K), repeats)
    out["query_equals_query_desc"] = bool(a.tobytes() == b.tobytes())
    _, out["add_us"] = _timed(lambda: db.add(clouds[0], poses[0], 7), repeats)
    db.close()
    print("RESULT " + json.dumps(out), flush=True)


def circle_worker(repeats):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import liodom_amd as la
    from liodom_amd import synth
    from oracle import oracle as orc
    import place_model as pm
    from mapper_lag_common import T_of
    orc.build(); synth.build()
    run = pm.circle(orc, synth)
    m = la.Map(12.0, 50.0, 0.4, max_cells=512, cell_capacity=4096, max_modified_cells=256)
    for k in range(pm.N_SITE_SCANS):
        m.update(run["edges"][k], T_of(run["gt"][k]))
    db = la.Places(max_places=64, max_edges=2048)
    for k, e, gt in run["keys"]:
        db.add(e, gt, k)
    scan_no, yaw = 205, 2.5
    edges, true = next((e, t) for k, a, e, t in run["queries"] if (k, a) == (scan_no, yaw))
    centre = np.array([0.0, 0.0, 0.0, 1.0] + list(np.mean([gt[4:] for gt in run["gt"][:pm.N_SITE_SCANS]], axis=0)))

    def off(pose):
        return float(np.linalg.norm(pose[4:] - true[4:])), float(2.0 * math.acos(min(1.0, abs(float(np.dot(pose[:4], true[:4]))))))

    def with_places():
        best = None
        for mt in db.query([edges], K)[0]:
            pose = mt["pose"]
            for grid in LEVELS:
                lv = m.search_pose(edges, pose, **grid)
                pose = lv["pose"]
            if best is None or lv["hits_r"] + lv["hits_0"] > best["hits_r"] + best["hits_0"]:
                best = lv
        return best

    m.search_pose_bnb(edges, centre, nx=1, ny=1); with_places()          # (first calls allocate)
    a, wall_a = _timed(lambda: m.search_pose_bnb(edges, centre, **WIDE), max(3, repeats // 4))
    b, wall_b = _timed(with_places, repeats)
    out = dict(scan=scan_no, turned=yaw, n_edges=int(edges.shape[0]), map_points=int(m.all().shape[0]), map_cells=m.num_cells(), places=db.count(),
               wide=dict(n_candidates=a["n_candidates"], hits_r=a["hits_r"], hits_0=a["hits_0"], off_truth=off(a["pose"]), stats=a["stats"], wall_us=wall_a),
               places_then_levels=dict(hits_r=b["hits_r"], hits_0=b["hits_0"], off_truth=off(b["pose"]), wall_us=wall_b))
    m.close(); db.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError("child %r failed (%d): %s" % (args, r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--row", nargs=3, default=None)
    ap.add_argument("--circle", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.row:
        return row_worker(a.row[0], int(a.row[1]), int(a.row[2]), a.repeats)
    if a.circle:
        return circle_worker(a.repeats)
    med = statistics.median
    rows = []
    print("# us per call: median over %d calls; %d edges per query, k = %d" % (a.repeats, N_EDGES, K))
    for geom in GEOMS:
        for places in PLACES:
            for queries in QUERIES:
                r = run_child(["--repeats", str(a.repeats), "--row", geom, str(places), str(queries)], 240)      # a failed child ends the job
                rows.append(r)
                print("%-5s W %2d  %7d places %3d queries: describe %8.1f  add %8.1f  query %9.1f  query_desc %9.1f%s" % (
                    geom, r["words"], places, queries, med(r["describe_us"]), med(r["add_us"]), med(r["query_us"]), med(r["query_desc_us"]),
                    "" if r["query_equals_query_desc"] else "  QUERY DIFFERS FROM QUERY_DESC"), flush=True)
    c = run_child(["--repeats", str(a.repeats), "--circle"], 420)
    wa, wb = med(c["wide"]["wall_us"]), med(c["places_then_levels"]["wall_us"])
    print("circle, scan %d turned %.1f rad, %d edges, %d map points:" % (c["scan"], c["turned"], c["n_edges"], c["map_points"]))
    print("  (a) bnb over %d candidates: %.1f us, score %d + %d, %.3f m / %.4f rad off the truth" % (
        c["wide"]["n_candidates"], wa, c["wide"]["hits_r"], c["wide"]["hits_0"], *c["wide"]["off_truth"]))
    print("  (b) query k = %d + levels:   %.1f us, score %d + %d, %.3f m / %.4f rad off the truth   (a) / (b) = %.1f" % (
        K, wb, c["places_then_levels"]["hits_r"], c["places_then_levels"]["hits_0"], *c["places_then_levels"]["off_truth"], wa / wb))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(repeats=a.repeats, n_edges=N_EDGES, k=K, rows=rows, circle=c), f, indent=1)


if __name__ == "__main__":
    main()
