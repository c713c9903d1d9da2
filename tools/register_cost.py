#!/usr/bin/env python3
"""What one liodom_map_register_poses call costs, beside what existed before it for one pose.

Two sites, each a map of the edges of synth stream 0 inserted at their ground truth and the edge cloud of a scan of stream 1:
  localize   16 x 900, R = 6, epr = 10, 14 scans (tests/localize_model.py's site: rows of ~1.6 k points, ~690 edges)
  hdl64      64 x 1800, R = 8, epr = 16, `--site-scans` (30) scans (rows of tens of thousands of points, thousands of edges)
Legs, per site: register n = 1, 3, 8 start poses (the truth displaced by up to 0.2 m / 0.005 half-angle per axis) at max_passes =
2 and 10 with stops 0 (so every pass runs) — a host clock around the call, which ends in a device synchronise; and `seeded`: what
a caller had before, liodom_seed_stream plus the same scan's odometry step on a reader handle of the same shapes (two passes, one
pose; the scan's edges already extracted: liodom_odometry_step).  LIODOM_MAP_STATE_TIMING=1 would add the kernels' event time on
stderr; it is left off here.

Every leg: `--warmup` (5) untimed calls, then `--calls` (50) timed ones; `--repeats` (5) rounds of all legs in turn; the JSON holds
every sample, the medians and the spread.  No GPU: the script fails.
usage: tools/register_cost.py [--calls 50] [--warmup 5] [--repeats 5] [--site-scans 30] [--out profiles/register_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SITES = dict(localize=(16, 900, 6, 10, 4, 14), hdl64=(64, 1800, 8, 16, 15, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--site-scans", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_cost.json"))
    a = ap.parse_args()
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api, synth
    import register_model as rm
    if la.device_count() < 1:
        sys.exit("register_cost: no GPU")
    result = dict(calls=a.calls, warmup=a.warmup, repeats=a.repeats, sites={})
    for name, (h, w, r, epr, p, count) in SITES.items():
        count = count or a.site_scans
        cfg = synth.make_cfg(h, w, 0)
        g = la.Liodom(la.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=p, mapping=1),
                      la.make_config(max_points=h * w, max_width=w, recv_capacity=1 << 18))
        m = la.Map(max_cells=1024, cell_capacity=32768, max_update_points=32768)
        for k in range(count):
            x, gt = synth.scan(cfg, 0, k)
            m.update(g.extract_edges(x, h, w)["edges"], api.pose_T34(gt))
        assert m.status() == 0
        scan, gt = synth.scan(cfg, 1, count // 2)
        edges = g.extract_edges(scan, h, w)["edges"]
        rng = np.random.default_rng(11)
        poses = np.array([rm.displaced(gt, (rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.005, 0.005, 3))) for _ in range(8)])
        local = int(m.get_local(api.pose_T34(gt), 2, 1).shape[0])
        cap = 1 << max(11, int(np.ceil(np.log2(local + 1))))
        legs = {}
        for n in (1, 3, 8):
            for passes in (2, 10):
                legs["register n=%d passes=%d" % (n, passes)] = (
                    lambda n=n, passes=passes: m.register_poses(edges, poses[:n], max_passes=passes, stop_translation=0.0, stop_rotation=0.0, local_capacity=cap))
        g.attach_map_reader(m, 2, 1)

        def seeded():
            g.seed_stream(poses[0])
            g.odometry_step(edges)
        legs["seeded (seed_stream + odometry_step, 2 passes, 1 pose)"] = seeded
        samples = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, f in legs.items():
                for _ in range(a.warmup):
                    f()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()
                samples[k].append((time.perf_counter() - t0) / a.calls * 1e6)
        rows = m.register_poses(edges, poses, max_passes=10, local_capacity=cap)
        result["sites"][name] = dict(shape=[h, w, r, epr], site_scans=count, n_edges=int(edges.shape[0]), local_points=local, local_capacity=cap,
                                     terminations=[r_["termination"] for r_ in rows], passes=[r_["passes"] for r_ in rows],
                                     matches=[r_["matches"] for r_ in rows],
                                     legs={k: dict(us=v, median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in samples.items()})
        for k, v in samples.items():
            print("%-9s %-58s median %9.1f us  (min %9.1f, max %9.1f)" % (name, k, statistics.median(v), min(v), max(v)))
        g.attach_mapper(None)
        g.close(); m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
