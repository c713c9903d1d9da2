#!/usr/bin/env python3
"""Does the lagged map help?  CPU only: the oracle's odometer over `--scans` (120) synthetic scans with the generator's ground
truth, once odometry-only (mapping off) and once with the lagged mapper's loop (mapping on; after step j >= P the oracle's Map
takes the frame that left the window, update(e_{j-P}, T_{j-P}), and the odometer receives local(T_j, 2, 1)).  Reports the
relative pose error per scan (translation and rotation of gt_delta^-1 * est_delta, mean / max), the drift of the final pose,
and how the solves ended.  The synchronous replay (lag 0) is listed for the record: its poses are the constant-velocity
prediction.  usage: tools/mapper_lag_accuracy.py [--scans 120] [--height 16 --width 900] [--prev-frames 5]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from liodom_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402


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


def run(mode, scans, H, W, R, epr, P):
    """mode: 'odometry', 'lag1' or 'lag0'.  -> estimated 4 x 4 poses, terminations of the finalising solves."""
    po = orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1,
                         mapping={"odometry": 0, "lag1": 2, "lag0": 1}[mode])
    od, mo = orc.Odometer(po), orc.Map()
    est, term, hist = [], [], []
    for j, x in enumerate(scans):
        e = orc.extract(po, x, H, W)["edges"]
        pose, info = od.step(e)
        est.append(T44(pose))
        term.append(info.lm[1].termination)
        hist.append((e, est[-1][:3]))
        if mode == "lag1" and j >= P:
            mo.update(*hist[j - P])
            od.set_received_map(mo.local(hist[j][1], 2, 1))
    od.close()
    return est, term


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=120)
    ap.add_argument("--height", type=int, default=16)
    ap.add_argument("--width", type=int, default=900)
    ap.add_argument("--prev-frames", type=int, default=5)
    a = ap.parse_args()
    H, W, R, epr, P = a.height, a.width, 6, 10, a.prev_frames
    synth.build(); orc.build()
    cfg = synth.make_cfg(H, W, 0)
    data = [synth.scan(cfg, 0, k) for k in range(a.scans)]
    scans = [d[0] for d in data]
    gt = [T44(d[1]) for d in data]
    gt = [np.linalg.inv(gt[0]) @ g for g in gt]          # the odometer starts at the identity
    print("# oracle, %d x %d, R = %d, epr = %d, prev_frames = %d, %d scans; relative pose error per scan against the generator's ground truth" % (H, W, R, epr, P, a.scans))
    print("%-10s %12s %12s %12s %12s %14s %14s  %s" % ("mode", "rpe_t mean", "rpe_t max", "rpe_r mean", "rpe_r max", "final drift t", "final drift r", "terminations of the finalising solve"))
    for mode in ("odometry", "lag1", "lag0"):
        est, term = run(mode, scans, H, W, R, epr, P)
        rpe = [err(np.linalg.inv(np.linalg.inv(gt[k - 1]) @ gt[k]) @ (np.linalg.inv(est[k - 1]) @ est[k])) for k in range(1, a.scans)]
        dt, dr = err(np.linalg.inv(gt[-1]) @ est[-1])
        counts = {t: term[1:].count(t) for t in sorted(set(term[1:]))}
        print("%-10s %12.5f %12.5f %12.6f %12.6f %14.4f %14.5f  %s" % (
            mode, np.mean([r[0] for r in rpe]), max(r[0] for r in rpe), np.mean([r[1] for r in rpe]), max(r[1] for r in rpe), dt, dr, counts))


if __name__ == "__main__":
    main()
