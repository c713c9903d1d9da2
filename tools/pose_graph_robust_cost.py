#!/usr/bin/env python3
"""What a robust loss costs on the pose graph: the robust kernel instances against the quadratic ones on the same graph, in the same
job.  Needs a GPU.  One child process per row (each under its own time limit), as tools/pose_graph_cost.py; within a row every
timed call is warmed up once and repeated --repeats times from the same poses, and the median, the smallest and the largest are kept.

  times   a host clock around a call that ends in a device synchronise:
          optimize_ms    liodom_graph_optimize with the options of tests/test_gpu_pose_graph.py (pcg_tolerance 1e-10, 50 steps)
          linearize_ms   set_poses + liodom_graph_linearize: the upload, ONE launch of k_graph_linearize (or its robust twin),
                         k_graph_sum, k_graph_gather and the download — an upper bound of the launch; the difference between two
                         rows on the same graph is the difference of the two kernel instances
  rows    ring257            drifted_ring(257, 1, 257), no loss: the quadratic kernels
          ring257_w1         the same with Huber of scale 1e300 on both kinds: the robust kernels, every weight exactly 1, so
                             the same steps, the same iterations, the same bytes — what the instances themselves cost
          ring257_false      ring257 plus one false loop edge 192 -> 64 (identity), no loss
          ring257_false_gm5  the same with Geman-McClure 5 on the loop edges
          ring48_plain / ring48_two_stage   ring_with_false_loop(48, 2, 48): one quadratic solve against the two-stage close on
                             the graph alone (robust solve, edge_weights, the rejected edge switched off, quadratic solve)
  circle  (--circle, a row of its own) the project's circle (tests/place_model.py) driven as
          test_the_loop_of_the_circle_is_found_and_closed drives it, one false loop planted through add_loop between the key
          frames a quarter and three quarters of the way round, closed the plain way and the two-stage way: key-frame rms.
usage: tools/pose_graph_robust_cost.py [--repeats 7] [--circle] [--out profiles/pose_graph_robust_cost.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("ring257", "ring257_w1", "ring257_false", "ring257_false_gm5", "ring48_plain", "ring48_two_stage")
OPT = dict(pcg_tolerance=1e-10, max_iterations=50)


def _paths():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def row_worker(name, repeats):
    _paths()
    import numpy as np
    import graph_model as gm
    import graph_robust_model as rm
    from liodom_amd import api
    table = {}
    if name.startswith("ring257"):
        poses, fixed, edges = gm.drifted_ring(257, 1, seed=257)[1:]
        if "false" in name:
            edges = np.concatenate([edges, api.graph_edges([192], [64], [[0, 0, 0, 1, 0, 0, 0]], gm.OMEGA, kind=1)])
        if name.endswith("_w1"):
            table = {0: ("huber", 1e300), 1: ("huber", 1e300)}
        if name.endswith("_gm5"):
            table = {1: ("geman_mcclure", 5.0)}
    else:
        _, poses, fixed, edges, fi = rm.ring_with_false_loop(48, 2, 48)
    g = api.PoseGraph(max_nodes=len(poses), max_edges=len(edges))
    g.add_nodes(poses, fixed)
    g.add_edges(edges)
    for kind, (loss, scale) in table.items():
        g.set_loss(kind, loss, scale)
    row = dict(row=name, nodes=int(len(poses)), edges=int(len(edges)), losses={str(k): list(v) for k, v in table.items()}, options=OPT)

    def solve():
        if name != "ring48_two_stage":
            return dict(report=g.optimize(**OPT))
        g.set_edge_active(0, np.ones(len(edges)))
        g.set_loss(1, "geman_mcclure", 5.0)
        first = g.optimize(**OPT)
        w = g.edge_weights()[1]
        g.set_loss(1, "none")
        for e in np.nonzero((edges["kind"] == 1) & (w < 0.5))[0]:
            g.set_edge_active(int(e), [0])
        return dict(robust_report=first, report=g.optimize(**OPT), rejected=[int(e) for e in np.nonzero((edges["kind"] == 1) & (w < 0.5))[0]])

    opt_ms, lin_ms, last = [], [], None
    for k in range(repeats + 1):                   # the first round loads the code objects and is not kept
        g.set_poses(0, poses)
        t0 = time.perf_counter()
        g.linearize()
        t1 = time.perf_counter()
        last = solve()
        t2 = time.perf_counter()
        if k:
            lin_ms.append((t1 - t0) * 1e3)
            opt_ms.append((t2 - t1) * 1e3)
    row.update(last)
    row["optimize_ms"], row["linearize_ms"] = _stats(opt_ms), _stats(lin_ms)
    if "false" in name or name.startswith("ring48"):
        clean, _ = gm.lm(poses, fixed, edges[:-1], max_iterations=50)
        row["worst_distance_to_clean"] = list(rm.max_distance(g.poses(), clean))
    g.close()
    print("ROW " + json.dumps(row))


def circle_worker():
    _paths()
    import numpy as np
    import graph_model as gm
    import place_model as pm
    import liodom_amd as la
    from liodom_amd import api, loop, synth
    from oracle import oracle as orc
    orc.build()
    synth.build()
    run = pm.circle(orc, synth)
    H, W = pm.H, pm.W_SCAN
    gt = np.stack([gm.pose(p[:4], p[4:]) for p in run["gt"]])
    levels = [dict(step_xy=0.4, step_yaw=0.02, nx=8, ny=8, nyaw=7), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]
    row = dict(row="circle")
    for mode in ("plain", "two_stage"):
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, mapping=1, max_range=pm.MAX_RANGE),
                      la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))
        m = la.Map(12.0, 50.0, 0.4, max_cells=512, cell_capacity=4096, max_modified_cells=256)
        db = la.Places(max_places=64, max_edges=2048)
        lc = loop.LoopCloser(m, db, levels, min_dist=4.0, min_gap=10, k=2, min_fraction=0.3, max_nodes=128, max_edges=512)
        key_scans, found = [], []
        for k in range(len(run["scans"]) - 1):
            pose, info = g.process_scan(run["scans"][k], H, W)
            pose = gm.compose(gt[0], gm.pose(pose[:4], pose[4:]))
            edges = g.get_edges()["edges"]
            if k < pm.N_SITE_SCANS:
                m.update(edges, api.pose_T34(pose))
            r = lc.feed(pose, edges)
            if r["key_frame"]:
                key_scans.append(k)
            found += r["loops"]
        n = len(key_scans)
        lc.add_loop(n // 4, 3 * n // 4, [0, 0, 0, 1, 0, 0, 0])           # "a quarter and three quarters of the way round are one place"
        gt_keys = gt[key_scans]

        def rms(poses):
            d = np.linalg.norm(np.asarray(poses)[:, 4:] - gt_keys[:, 4:], axis=1)
            return float(np.sqrt(np.mean(d * d)))

        t0 = time.perf_counter()
        if mode == "plain":
            out = lc.close(handle=g, reader_cells=(3, 1), **OPT)
        else:
            out = lc.close(handle=g, reader_cells=(3, 1), loss=("geman_mcclure", 5.0), reject_below=0.5, **OPT)
        row[mode] = dict(key_frames=n, true_loops=[(l["place"], l["node"]) for l in found], false_loop=(n // 4, 3 * n // 4), close_ms=(time.perf_counter() - t0) * 1e3,
                         rms_before=rms(out["before"]), rms_after=rms(out["after"]), report=out["report"],
                         rejected=out.get("rejected"), kept=out.get("kept"), applied=out.get("applied", True))
        g.attach_mapper(None)
        g.close(); m.close(); db.close(); lc.graph.close()
    print("ROW " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--circle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_robust_cost.json"))
    ap.add_argument("--row", default="")
    a = ap.parse_args()
    if a.row == "circle":
        circle_worker()
        return 0
    if a.row:
        row_worker(a.row, a.repeats)
        return 0
    rows = []
    for name in ROWS + (("circle",) if a.circle else ()):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", name, "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            return 1                               # nothing more is started on the GPU after a row that failed
        line = [l for l in r.stdout.split("\n") if l.startswith("ROW ")][-1]
        rows.append(json.loads(line[4:]))
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/pose_graph_robust_cost.py", rows=rows), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
