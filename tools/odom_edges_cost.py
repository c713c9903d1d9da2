#!/usr/bin/env python3
"""What does an odometry edge's information cost?  A 16 x 900 handle with pose_covariance = 1 runs 200 synthetic scans; then, for
n = 1, 64 and 1 024 intervals of 8 scans each (overlapping, spread over the log), the wall time of
  device   one Liodom.odometry_edges call (liodom_get_odometry_edges: k_odom_edges on the logs where they lie, n records back)
  host     the alternative on the same handle: both logs copied out (liodom_get_pose_log, liodom_get_pose_covariance_log, the
           whole log of 200 scans, as a caller who keeps no copy would) and chained in NumPy (matrix form, tests/odom_edge_model.py
           chain_dense), split into its copy and its arithmetic
Median of --repeat calls after 3 warm-up calls, host clock (time.perf_counter) around calls that synchronise before they return.
Written as JSON to --out and printed as the rows of DESIGN.md §5.22's table.  No GPU: the script fails.
usage: tools/odom_edges_cost.py [--repeat 20] [--out profiles/odom_edges_cost.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H, W, SCANS, SPAN = 16, 900, 200, 8


def median_ms(fn, repeat):
    for _ in range(3):
        fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t.sort()
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odom_edges_cost.json"))
    a = ap.parse_args()
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api, synth
    import odom_edge_model as om
    if la.device_count() < 1:
        sys.exit("odom_edges_cost: no GPU")
    synth.build()
    cfg = synth.make_cfg(H, W, 0)
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=6, edges_per_region=10, prev_frames=5),
                  la.make_config(max_points=H * W, max_width=W, pose_covariance=1, pose_log_capacity=SCANS + 8))
    for k in range(SCANS):
        g.process_scan(synth.scan(cfg, 7, k)[0], H, W)
    g.sync()
    result = dict(scans=SCANS, span=SPAN, repeat=a.repeat, rows=[])
    for n in (1, 64, 1024):
        f = (np.arange(n, dtype=np.int64) * 7) % (SCANS - SPAN - 1) + 1
        t = f + SPAN
        logs = {}

        def copy():
            logs["poses"] = g.pose_log(0, 0, SCANS)[0]
            recs = (api.PoseCov * SCANS)()
            g._check(g.L.liodom_get_pose_covariance_log(g.h, 0, 0, SCANS, recs))
            logs["covs"] = np.frombuffer(recs, dtype=api.POSE_COV_DTYPE)["covariance"]

        def chain():
            return [om.chain_dense(logs["poses"], logs["covs"], int(i), int(j))[2] for i, j in zip(f, t)]

        device = median_ms(lambda: g.odometry_edges(0, f, t), a.repeat)
        copy_ms = median_ms(copy, a.repeat)
        chain_ms = median_ms(chain, max(3, a.repeat // 4) if n > 64 else a.repeat)
        rec = g.odometry_edges(0, f, t)
        ok = rec["flags"] == api.ODOM_EDGE_VALID
        worst = max(float(np.linalg.norm(o - r["information"]) / np.linalg.norm(o)) for o, r, u in zip(chain(), rec, ok) if u)
        row = dict(n=n, device_ms=device, host_copy_ms=copy_ms, host_chain_ms=chain_ms, host_ms=copy_ms + chain_ms, valid=int(ok.sum()),
                   host_vs_device_omega=worst)
        result["rows"].append(row)
        print("| %d | %.3f | %.3f | %.3f + %.3f |" % (n, device, copy_ms + chain_ms, copy_ms, chain_ms))
    g.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
