"""Does deskewing the edge clouds by the predicted scan motion make the odometry more accurate?  CPU only (oracle).

Input: the synthetic generator's rolling sweep (synth make_cfg(sweep=1): column c fired at c / W of the sweep from the pose the
sensor has then).  Three runs of the oracle odometer over the same stream:
  raw    edges as extracted (what LiODOM does)
  pred   edges deskewed with the motion the constant-velocity prediction applies, D = T_{k-2}^-1 T_{k-1}, read from
         Odometer.state() before each step (the model of tests/deskewref.py)
  true   edges deskewed with the generator's own motion of that scan, T_{k-1}^-1 T_k (an upper bound of what the model can give)
Prints the relative pose error against the generator's ground truth: mean translation error of consecutive relative motions
over all scans and from scan 10 on (after the start-up), and the drift relative to scan 10 at the end.

    python tools/deskew_accuracy.py [--shape vlp16|hdl64] [--scans 60] [--speed 1.0] [--yaw 3.0]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deskewref as dr  # noqa: E402
from liodom_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

SHAPES = {"vlp16": (16, 1800, 6), "hdl64": (64, 1800, 8)}


def run(shape, scans, speed, yaw, mode, stream=0):
    H, W, R = SHAPES[shape]
    cfg = synth.make_cfg(H, W, 0, speed=speed, yaw_rate_deg=yaw, sweep=1)
    po = orc.make_params(scan_lines=H, scan_regions=R, edges_per_region=10, prev_frames=5, knn_mode=1)
    od = orc.Odometer(po)
    est, gt = [], []
    for k in range(scans):
        x, g = synth.scan(cfg, stream, k)
        e = orc.extract(po, x, H, W)["edges"]
        if mode == "pred":
            odom, prev = od.state()
            e = dr.deskew_edges(e, dr.delta_of(prev, odom), 1, 0.0)
        elif mode == "true":
            _, g_prev = synth.scan(cfg, stream, k - 1)
            e = dr.deskew_edges(e, dr.delta_of(dr.pose34(g_prev), dr.pose34(g)), 1, 0.0)
        p, _ = od.step(e)
        est.append(dr.pose34(p))
        gt.append(dr.pose34(g))
    od.close()
    rpe = np.array([np.linalg.norm(dr.delta_of(dr.delta_of(gt[k - 1], gt[k]), dr.delta_of(est[k - 1], est[k]))[:, 3])
                    for k in range(1, scans)])
    drift = np.linalg.norm(dr.delta_of(dr.delta_of(gt[10], gt[-1]), dr.delta_of(est[10], est[-1]))[:, 3])
    return dict(shape=shape, mode=mode, speed=speed, yaw_deg=yaw, scans=scans, rpe_mean=float(rpe.mean()),
                rpe_mean_from10=float(rpe[9:].mean()), drift_from10=float(drift))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--scans", type=int, default=60)
    ap.add_argument("--speed", type=float, default=1.0)
    ap.add_argument("--yaw", type=float, default=3.0)
    a = ap.parse_args()
    synth.build()
    orc.build()
    for shape in a.shape or ["vlp16", "hdl64"]:
        for mode in ("raw", "pred", "true"):
            print(json.dumps(run(shape, a.scans, a.speed, a.yaw, mode)), flush=True)


if __name__ == "__main__":
    main()
