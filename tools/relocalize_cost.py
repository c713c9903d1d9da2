#!/usr/bin/env python3
"""What relocalising in a saved map costs per call.  Needs a GPU.  The site map and scan of tests/localize_model.py (16 x 900; the
edges of synth stream 0 at ground truth; scan 0 of stream 1), the centre 3.1 / -2.3 m and 0.37 rad off, and the two levels of
DESIGN.md §5.10: 21 x 21 x 51 = 22 491 candidates at 0.4 m / 0.02 rad, then 9 x 9 x 9 = 729 at 0.1 m / 0.005 rad around the
first level's best.  Per level, over `--repeats` calls of liodom_map_search_pose in a child process:
  kernels   HIP-event time of the occupancy build (k_map_occ_clear + k_map_occ_build), of k_map_score_poses and of
            k_map_score_best, as the library reports them under LIODOM_MAP_STATE_TIMING=1
  call      wall time of the whole call (matrices made on the host, uploads, kernels, read-back) in a child without that switch
and the bytes of the occupancy.  The NumPy model (tests/reloc_model.py) scores the same candidates once, for scale only.
usage: tools/relocalize_cost.py [--repeats 20] [--no-model] [--out profiles/relocalize.json]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, R, EPR, P, SITE_SCANS = 16, 900, 6, 10, 4, 14
LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=10, ny=10, nyaw=25), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]
OFFSET = (3.1, -2.3, 0.37)


def worker(repeats, model):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api, synth
    from relocalize_accuracy import T34, moved
    cfg = synth.make_cfg(H, W, 0)
    x = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P), la.make_config(max_points=H * W, max_width=W))
    m = la.Map(max_cells=128, cell_capacity=16384)
    for k in range(SITE_SCANS):
        scan, pose = synth.scan(cfg, 0, k)
        m.update(x.extract_edges(scan, H, W)["edges"], T34(pose))
    scan, gt = synth.scan(cfg, 1, 0)
    edges = x.extract_edges(scan, H, W)["edges"]
    x.close()
    centre = moved(np.array(gt, dtype=np.float64), OFFSET)
    out = dict(n_edges=int(edges.shape[0]), cells=m.num_cells(), points=int(m.all().shape[0]), levels=[])
    state = api.parse_map_state(m.export_state())
    if model:
        import reloc_model as rm
        occ = rm.Occupancy(state)
        out["occupancy_bytes"] = occ.bytes
    m.search_pose(edges, centre, nx=1)          # the first call allocates the occupancy
    for grid in LEVELS:
        wall = []
        for _ in range(repeats):
            sys.stderr.write("CALL\n"); sys.stderr.flush()
            t0 = time.perf_counter()
            r = m.search_pose(edges, centre, **grid)
            wall.append((time.perf_counter() - t0) * 1e6)
        rec = dict(grid=grid, n_candidates=r["n_candidates"], best_index=r["best_index"], hits_r=r["hits_r"], hits_0=r["hits_0"], wall_us=wall)
        if model:
            full = m.search_pose(edges, centre, want_T=True, want_hits=True, **grid)
            t0 = time.perf_counter()
            want = occ.hits(edges, full["T_all"], radius=1)
            rec["model_s"] = time.perf_counter() - t0
            rec["model_equal"] = bool(np.array_equal(want, full["hits"]) and rm.best_of(want) == full["best_index"])
        out["levels"].append(rec)
        centre = r["pose"]
    m.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(repeats, model, timing):
    env = dict(os.environ)
    env.pop("LIODOM_MAP_STATE_TIMING", None)
    if timing:
        env["LIODOM_MAP_STATE_TIMING"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(repeats)] + ([] if model else ["--no-model"]),
                       capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    calls = []
    for ln in r.stderr.splitlines():
        if ln == "CALL":
            calls.append({})
        found = re.match(r"liodom_map_score_poses (\w+): kernels ([0-9.]+) ms", ln)
        if found and calls and found.group(1) not in calls[-1]:
            calls[-1][found.group(1)] = float(found.group(2)) * 1e3
    return res, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.repeats, not a.no_model)
    plain, _ = run_child(a.repeats, not a.no_model, False)
    _, calls = run_child(a.repeats, False, True)
    print("# %d edges against %d points in %d cells; occupancy %s bytes; us per call: median (min .. max) over %d calls"
          % (plain["n_edges"], plain["points"], plain["cells"], plain.get("occupancy_bytes", "?"), a.repeats))
    med = lambda xs: (statistics.median(xs), min(xs), max(xs))
    for i, lv in enumerate(plain["levels"]):
        mine = calls[i * a.repeats:(i + 1) * a.repeats]
        lv["kernels_us"] = {k: [c[k] for c in mine if k in c] for k in ("occupancy", "score", "best")}
        print("%6d candidates: best %5d (%d + %d)  occupancy %8.1f (%.1f .. %.1f)  score %9.1f (%.1f .. %.1f)  best %6.1f (%.1f .. %.1f)  whole call %9.1f (%.1f .. %.1f)%s"
              % ((lv["n_candidates"], lv["best_index"], lv["hits_r"], lv["hits_0"]) + med(lv["kernels_us"]["occupancy"]) + med(lv["kernels_us"]["score"]) +
                 med(lv["kernels_us"]["best"]) + med(lv["wall_us"]) +
                 ((("  NumPy model %.2f s, counts %s" % (lv["model_s"], "equal" if lv["model_equal"] else "DIFFER")) if "model_s" in lv else ""),)))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["cost"] = dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, offset=OFFSET, repeats=a.repeats, **plain)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
