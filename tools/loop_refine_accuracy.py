#!/usr/bin/env python3
"""Does registering the loop measurement help?  The circle of tests/place_model.py (the run of
tests/test_gpu_pose_graph.py::test_the_loop_of_the_circle_is_found_and_closed) closed three ways:
  plain    LoopCloser as it was: Z from the pose the search levels found, the constant LOOP_INFO
  refine   LoopCloser(refine=dict(min_fraction=0.25)): Z from the pose registered to the map (Map.register_poses), LOOP_INFO
  solve    the same with loop_info="solve": the edge's information from the registration's solve
Per way: loop edges, key-frame position rms / z rms / last key frame before and after close(), each registration's termination,
passes and matches.  Written as JSON to --out and printed as the rows of DESIGN.md §5.16's table.  The run takes too long for a
test.  No GPU: the script fails.
usage: tools/loop_refine_accuracy.py [--out profiles/loop_refine_accuracy.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SITE_SZ, SITE_CELLS = (12.0, 50.0, 0.4), (3, 1)
LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=8, ny=8, nyaw=7), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]
WAYS = dict(plain={}, refine=dict(refine=dict(min_fraction=0.25, cells_xy=SITE_CELLS[0], cells_z=SITE_CELLS[1])),
            solve=dict(refine=dict(min_fraction=0.25, cells_xy=SITE_CELLS[0], cells_z=SITE_CELLS[1]), loop_info="solve"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_refine_accuracy.json"))
    a = ap.parse_args()
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api, loop, synth
    from oracle import oracle as orc
    import graph_model as gm
    import place_model as pm
    if la.device_count() < 1:
        sys.exit("loop_refine_accuracy: no GPU")
    run = pm.circle(orc, synth)
    H, W = pm.H, pm.W_SCAN
    gt = np.stack([gm.pose(p[:4], p[4:]) for p in run["gt"]])
    result = {}
    for way, kw in WAYS.items():
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, mapping=1, max_range=pm.MAX_RANGE),
                      la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))
        m = la.Map(*SITE_SZ, max_cells=512, cell_capacity=4096, max_modified_cells=256)
        db = la.Places(max_places=64, max_edges=2048)
        lc = loop.LoopCloser(m, db, LEVELS, min_dist=4.0, min_gap=10, k=2, min_fraction=0.3, max_nodes=128, max_edges=512, **kw)
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
        gt_keys = gt[key_scans]

        def errors(poses):
            d = np.asarray(poses)[:, 4:] - gt_keys[:, 4:]
            n = np.linalg.norm(d, axis=1)
            return dict(rms=float(np.sqrt(np.mean(n * n))), z_rms=float(np.sqrt(np.mean(d[:, 2] ** 2))), last=float(n[-1]))

        row = dict(key_frames=len(key_scans), loop_edges=len(found),
                   registrations=[dict(termination=l["registration"]["termination"], passes=l["registration"]["passes"],
                                       matches=l["registration"]["matches"], moved=float(np.linalg.norm(l["pose"][4:] - l["searched_pose"][4:])))
                                  for l in found if "registration" in l])
        if found:
            out = lc.close(handle=g, reader_cells=SITE_CELLS, pcg_tolerance=1e-10, max_iterations=50)
            row.update(before=errors(out["before"]), after=errors(out["after"]), termination=out["report"]["termination"])
            print("| %s | %d | %.3f → %.3f | %.3f → %.3f | %.3f → %.3f |" % (way, len(found), row["before"]["rms"], row["after"]["rms"],
                  row["before"]["z_rms"], row["after"]["z_rms"], row["before"]["last"], row["after"]["last"]))
        else:
            print("| %s | 0 | no loop edge: nothing closed |" % way)
        result[way] = row
        g.attach_mapper(None)
        g.close(); m.close(); db.close(); lc.graph.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
