#!/usr/bin/env python3
"""What relocalising over a wide window costs per call: liodom_map_search_pose_bnb beside liodom_map_search_pose.  Needs a GPU.
The site map and scan of tools/relocalize_cost.py (16 x 900; the edges of synth stream 0 at ground truth; scan 0 of stream 1).
In one job, over `--repeats` calls each, in a child process:
  the exhaustive call and the new call (batch 256 / 1024 / 4096) on the window of DESIGN.md §5.10: 21 x 21 x 51 = 22 491 candidates
      at 0.4 m / 0.02 rad around a centre 3.1 / -2.3 m and 0.37 rad off;
  the new call (the same batches) on 201 x 201 x 157 = 6 342 957 and 201 x 201 x 315 = 12 726 315 candidates (+-40 m; +-1.56 and
      +-3.14 rad) around a centre 31.1 / -22.3 m and 0.37 rad off.
  call      wall time of the whole call, in a child without LIODOM_MAP_STATE_TIMING
  split     where the new call's time goes, as the library reports it under LIODOM_MAP_STATE_TIMING=1 in a second child: build
            (occupancy + block tables), bound (k_map_bound_nodes rounds: node matrices, upload, launch, read-back), exact
            (k_map_score_poses rounds likewise), host (the rest: the rounds' sorting and splitting) — a host clock around work that
            ends in a synchronise
and the search's own counters.  Every new call's result is compared with the exhaustive one where that exists.
usage: tools/relocalize_bnb_cost.py [--repeats 20] [--out profiles/relocalize_bnb.json]"""
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
BATCHES = (256, 1024, 4096)
WINDOWS = [
    dict(name="21x21x51", offset=(3.1, -2.3, 0.37), exhaustive=True, grid=dict(step_xy=0.4, step_yaw=0.02, nx=10, ny=10, nyaw=25)),
    dict(name="201x201x157", offset=(31.1, -22.3, 0.37), exhaustive=False, grid=dict(step_xy=0.4, step_yaw=0.02, nx=100, ny=100, nyaw=78)),
    dict(name="201x201x315", offset=(31.1, -22.3, 0.37), exhaustive=False, grid=dict(step_xy=0.4, step_yaw=0.02, nx=100, ny=100, nyaw=157)),
]


def worker(repeats):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import liodom_amd as la
    from liodom_amd import synth
    from relocalize_accuracy import T34, moved, pose_diff
    cfg = synth.make_cfg(H, W, 0)
    x = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P), la.make_config(max_points=H * W, max_width=W))
    m = la.Map(max_cells=128, cell_capacity=16384)
    for k in range(SITE_SCANS):
        scan, pose = synth.scan(cfg, 0, k)
        m.update(x.extract_edges(scan, H, W)["edges"], T34(pose))
    scan, gt = synth.scan(cfg, 1, 0)
    edges = x.extract_edges(scan, H, W)["edges"]
    modes = x.modes()
    x.close()
    gt = np.array(gt, dtype=np.float64)
    out = dict(n_edges=int(edges.shape[0]), cells=m.num_cells(), points=int(m.all().shape[0]), modes=modes, cases=[])
    m.search_pose(edges, gt, nx=1)              # the first calls allocate the occupancy and the block tables
    m.search_pose_bnb(edges, gt, nx=1, ny=1)

    def timed(call):
        wall = []
        for _ in range(repeats):
            sys.stderr.write("CALL\n"); sys.stderr.flush()
            t0 = time.perf_counter()
            r = call()
            wall.append((time.perf_counter() - t0) * 1e6)
        return r, wall

    for w in WINDOWS:
        centre, want = moved(gt, w["offset"]), None
        if w["exhaustive"]:
            want, wall = timed(lambda: m.search_pose(edges, centre, **w["grid"]))
            out["cases"].append(dict(window=w["name"], call="exhaustive", batch=None, n_candidates=want["n_candidates"], best_index=want["best_index"],
                                     hits_r=want["hits_r"], hits_0=want["hits_0"], wall_us=wall))
        for batch in BATCHES:
            m.search_pose_bnb(edges, centre, batch=batch, **w["grid"])      # (a larger batch regrows the staging once)
            r, wall = timed(lambda: m.search_pose_bnb(edges, centre, batch=batch, **w["grid"]))
            dt, dr = pose_diff(r["pose"], gt)
            rec = dict(window=w["name"], call="bnb", batch=batch, n_candidates=r["n_candidates"], best_index=r["best_index"], hits_r=r["hits_r"],
                       hits_0=r["hits_0"], stats=r["stats"], off_truth_m=dt, off_truth_rad=dr, wall_us=wall)
            if want is not None:
                rec["equals_exhaustive"] = bool(all(np.array_equal(r[k], want[k]) for k in want))
            out["cases"].append(rec)
    m.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(repeats, timing):
    env = dict(os.environ)
    env.pop("LIODOM_MAP_STATE_TIMING", None)
    if timing:
        env["LIODOM_MAP_STATE_TIMING"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--repeats", str(repeats)], capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    calls = []
    for ln in r.stderr.splitlines():
        if ln == "CALL":
            calls.append({})
        found = re.match(r"liodom_map_search_pose_bnb: build ([0-9.]+) ms, bound ([0-9.]+) ms, exact ([0-9.]+) ms, host ([0-9.]+) ms, total ([0-9.]+) ms", ln)
        if found and calls and not calls[-1]:
            calls[-1].update({k: float(v) * 1e3 for k, v in zip(("build", "bound", "exact", "host", "total"), found.groups())})
    return res, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.repeats)
    plain, _ = run_child(a.repeats, False)
    _, calls = run_child(a.repeats, True)
    print("# %d edges against %d points in %d cells; us per call: median (min .. max) over %d calls" % (plain["n_edges"], plain["points"], plain["cells"], a.repeats))
    print("# modes of the extracting handle: %s" % json.dumps(plain["modes"], sort_keys=True))
    med = lambda xs: (statistics.median(xs), min(xs), max(xs)) if xs else (float("nan"),) * 3
    for i, c in enumerate(plain["cases"]):
        mine = calls[i * a.repeats:(i + 1) * a.repeats]
        c["split_us"] = {k: [s[k] for s in mine if k in s] for k in ("build", "bound", "exact", "host", "total")} if c["call"] == "bnb" else {}
        line = "%-12s %-10s batch %5s: best %8d (%d + %d)  whole call %9.1f (%.1f .. %.1f)" % ((c["window"], c["call"], c["batch"], c["best_index"], c["hits_r"], c["hits_0"]) + med(c["wall_us"]))
        if c["call"] == "bnb":
            st = c["stats"]
            line += "  build %.1f bound %.1f exact %.1f host %.1f  rounds %d levels %d bounded %d scored %d  off truth %.3f m %.4f rad%s" % (
                med(c["split_us"]["build"])[0], med(c["split_us"]["bound"])[0], med(c["split_us"]["exact"])[0], med(c["split_us"]["host"])[0],
                st["rounds"], st["levels_built"], st["nodes_bounded"], st["candidates_scored"], c["off_truth_m"], c["off_truth_rad"],
                "" if "equals_exhaustive" not in c else ("  == exhaustive" if c["equals_exhaustive"] else "  DIFFERS from the exhaustive call"))
        print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, repeats=a.repeats, batches=BATCHES, **plain), f, indent=1)


if __name__ == "__main__":
    main()
