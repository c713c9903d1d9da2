#!/usr/bin/env python3
"""Does localising in a saved map help?  Needs a GPU.  The site map holds the edges of synth stream 0 (every `--site-step`-th
scan) at the generator's ground-truth poses; the traversal is synth stream 1 — the same world and path under other noise —
over `--scans` (120) scans.  Rows:
  odometry    a handle without a map, started at the identity; its poses are moved by the ground truth of scan 0 for the comparison
  reader      liodom_attach_map_reader on the site map, seeded (liodom_seed_stream) at the ground truth of scan 0
  reader+off  the same, seeded 0.2 / -0.1 / 0.05 m and 0.01 rad off
Reports the absolute pose error against the ground truth (translation and rotation: mean, max, last scan) and how the finalising
solves ended.  Reported, not asserted.
usage: tools/localize_accuracy.py [--scans 120] [--height 16 --width 900] [--prev-frames 5] [--site-step 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import liodom_amd as la  # noqa: E402
from liodom_amd import synth  # noqa: E402


def T44(pq):
    qx, qy, qz, qw = pq[:4]
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                 [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                 [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
    T[:3, 3] = pq[4:]
    return T


def err(E):
    return float(np.linalg.norm(E[:3, 3])), float(np.arccos(max(-1.0, min(1.0, (np.trace(E[:3, :3]) - 1.0) / 2.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--height", type=int, default=16)
    ap.add_argument("--width", type=int, default=900)
    ap.add_argument("--prev-frames", type=int, default=5)
    ap.add_argument("--site-step", type=int, default=2)
    a = ap.parse_args()
    H, W, R, epr, P = a.height, a.width, 6, 10, a.prev_frames
    synth.build()
    cfg = synth.make_cfg(H, W, 0)
    trav = [synth.scan(cfg, 1, k) for k in range(a.scans)]
    gt = [T44(t[1]) for t in trav]
    params = dict(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P)
    conf = dict(max_points=H * W, max_width=W)
    x = la.Liodom(la.make_params(**params), la.make_config(**conf))
    site = la.Map(max_cells=1024, cell_capacity=32768)
    for k in range(0, a.scans, a.site_step):
        scan, pose = synth.scan(cfg, 0, k)
        site.update(x.extract_edges(scan, H, W)["edges"], T44(pose)[:3])
    x.close()
    blob = site.export_state()
    print("# %d x %d, R = %d, epr = %d, prev_frames = %d, %d scans; site map: %d points in %d cells; absolute pose error against the generator's ground truth"
          % (H, W, R, epr, P, a.scans, site.all().shape[0], site.num_cells()))
    print("%-11s %10s %10s %10s %11s %11s %11s  %s" % ("mode", "t mean", "t max", "t last", "r mean", "r max", "r last", "terminations of the finalising solve"))
    off = np.array(trav[0][1], dtype=np.float64)
    off[4:] += (0.2, -0.1, 0.05)
    dq = np.array([0.0, 0.0, np.sin(0.005), np.cos(0.005)])
    q = off[:4]
    off[:4] = [q[3] * dq[0] + q[0] * dq[3] + q[1] * dq[2] - q[2] * dq[1], q[3] * dq[1] - q[0] * dq[2] + q[1] * dq[3] + q[2] * dq[0],
               q[3] * dq[2] + q[0] * dq[1] - q[1] * dq[0] + q[2] * dq[3], q[3] * dq[3] - q[0] * dq[0] - q[1] * dq[1] - q[2] * dq[2]]
    off[:4] /= np.linalg.norm(off[:4])
    for mode, seed in (("odometry", None), ("reader", trav[0][1]), ("reader+off", off)):
        g = la.Liodom(la.make_params(mapping=0 if seed is None else 1, **params), la.make_config(recv_capacity=1 << 16, **conf))
        if seed is not None:
            g.attach_map_reader(site, 2, 1)
            g.seed_stream(seed)
        est, term = [], []
        for scan, _ in trav:
            pose, info = g.process_scan(scan, H, W)
            est.append(T44(pose) if seed is not None else gt[0] @ T44(pose))
            term.append(info.lm[1].termination)
        if seed is not None:
            g.attach_mapper(None)
        g.close()
        e = [err(np.linalg.inv(gt[k]) @ est[k]) for k in range(a.scans)]
        counts = {t: term[1:].count(t) for t in sorted(set(term[1:]))}
        print("%-11s %10.4f %10.4f %10.4f %11.5f %11.5f %11.5f  %s" % (
            mode, np.mean([v[0] for v in e]), max(v[0] for v in e), e[-1][0], np.mean([v[1] for v in e]), max(v[1] for v in e), e[-1][1], counts))
    assert site.export_state() == blob, "a reader wrote to the site map"
    site.close()


if __name__ == "__main__":
    main()
