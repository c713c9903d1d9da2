#!/usr/bin/env python3
"""Does relocalising in a saved map find the pose?  Needs a GPU.  The site map holds the edges of synth stream 0 (every
`--site-step`-th scan) at the generator's ground-truth poses; the scans come from synth stream 1 — the same world and path under
other noise.  For each scan of `--scans` and each offset of OFFSETS (metres in x and y, radians of yaw about the world z axis; six
are multiples of the fine level's steps, so that the truth is a candidate, two lie between its points) the
centre is the ground truth moved by the offset; Liodom.relocalize searches a coarse and a fine level and seeds the stream, and the
same scan is processed.  A case counts as found when that pose lies within the project's pose tolerance (1e-4 m, 1e-4 rad) of the
same scan processed after liodom_seed_stream(ground truth).  One row per coarse yaw step of `--coarse-yaw` (the window stays
+-0.5 rad): the step must be of the order of leaf / range.  Reported, not asserted.
usage: tools/relocalize_accuracy.py [--scans 0,5,11,40,80] [--coarse-yaw 0.02,0.05,0.1] [--out profiles/relocalize.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import liodom_amd as la  # noqa: E402
from liodom_amd import synth  # noqa: E402

H, W, R, EPR, P = 16, 900, 6, 10, 5
TOL_T, TOL_R = 1e-4, 1e-4
OFFSETS = [(0.3, -0.2, 0.02), (1.2, -0.8, 0.1), (3.1, -2.3, 0.37), (-3.7, 3.3, -0.45), (3.9, 3.9, 0.49), (-2.0, 0.1, -0.25),      # on the fine grid
           (2.47, -1.33, 0.213), (-0.85, 3.06, -0.337)]                                                                          # between its points
FINE = dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)


def T34(pq):
    qx, qy, qz, qw = pq[:4]
    Rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                   [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                   [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return np.concatenate([Rm, np.array(pq[4:]).reshape(3, 1)], axis=1)


def moved(gt, off):
    """The ground truth moved by (dx, dy, yaw about the world z axis)."""
    h = 0.5 * off[2]
    ax, ay, az, aw = 0.0, 0.0, np.sin(h), np.cos(h)
    bx, by, bz, bw = gt[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz])
    return np.concatenate([q / np.linalg.norm(q), gt[4:] + np.array([off[0], off[1], 0.0])])


def pose_diff(a, b):
    d = abs(float(np.dot(a[:4], b[:4])))
    return float(np.linalg.norm(a[4:] - b[4:])), 2.0 * float(np.arccos(min(1.0, d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", default="0,5,11,40,80")
    ap.add_argument("--coarse-yaw", default="0.02,0.05,0.1")
    ap.add_argument("--site-scans", type=int, default=120)
    ap.add_argument("--site-step", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    scans = [int(v) for v in a.scans.split(",")]
    synth.build()
    cfg = synth.make_cfg(H, W, 0)
    params = dict(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P)
    conf = dict(max_points=H * W, max_width=W)
    x = la.Liodom(la.make_params(**params), la.make_config(**conf))
    site = la.Map(max_cells=1024, cell_capacity=32768)
    for k in range(0, a.site_scans, a.site_step):
        scan, pose = synth.scan(cfg, 0, k)
        site.update(x.extract_edges(scan, H, W)["edges"], T34(pose))
    x.close()
    blob = site.export_state()
    print("# %d x %d, R = %d, epr = %d; site map: %d points in %d cells; fine level %s" % (H, W, R, EPR, site.all().shape[0], site.num_cells(), FINE))
    g = la.Liodom(la.make_params(mapping=1, **params), la.make_config(recv_capacity=1 << 16, **conf))
    g.attach_map_reader(site, 2, 1)
    rows = []
    for yaw_step in (float(v) for v in a.coarse_yaw.split(",")):
        coarse = dict(step_xy=0.4, step_yaw=yaw_step, nx=10, ny=10, nyaw=int(round(0.5 / yaw_step)))
        found, cases = 0, []
        for k in scans:
            scan, gt = synth.scan(cfg, 1, k)
            gt = np.array(gt, dtype=np.float64)
            g.seed_stream(gt)
            want, _ = g.process_scan(scan, H, W)
            for off in OFFSETS:
                g.reset_stream(0)
                r = g.relocalize(site, scan, H, W, moved(gt, off), [coarse, FINE], min_fraction=0.0)
                got, _ = g.process_scan(scan, H, W)
                dt, dr = pose_diff(got, want)
                ok = dt <= TOL_T and dr <= TOL_R
                found += ok
                cases.append(dict(scan=k, offset=off, coarse_error=pose_diff(r["levels"][0]["pose"], gt), fine_error=pose_diff(r["levels"][1]["pose"], gt),
                                  fraction=r["fraction"], seeded_scan_error=(dt, dr), found=bool(ok)))
        n = len(cases)
        worst = max(c["fine_error"][0] for c in cases)
        off_grid = [c for c in cases if c["offset"] in OFFSETS[6:]]
        print("coarse yaw step %.3f rad (%5d candidates): found %2d of %2d; fine level's worst distance from the truth %.3f m; lowest fraction %.3f; "
              "offsets between grid points: fine level within %.3f m / %.4f rad, seeded scan within %.4f m / %.5f rad of the truth-seeded one"
              % (yaw_step, 21 * 21 * (2 * coarse["nyaw"] + 1), found, n, worst, min(c["fraction"] for c in cases),
                 max(c["fine_error"][0] for c in off_grid), max(c["fine_error"][1] for c in off_grid),
                 max(c["seeded_scan_error"][0] for c in off_grid), max(c["seeded_scan_error"][1] for c in off_grid)))
        rows.append(dict(coarse=coarse, fine=FINE, found=int(found), cases=n, detail=cases))
    g.attach_mapper(None)
    g.close()
    assert site.export_state() == blob, "relocalising wrote to the site map"
    site.close()
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["accuracy"] = dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, prev_frames=P, scans=scans, offsets=OFFSETS, tol_t=TOL_T, tol_r=TOL_R, rows=rows)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
