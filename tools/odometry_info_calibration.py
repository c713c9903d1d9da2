#!/usr/bin/env python3
"""How honest is the information of an odometry edge?  The circle of tests/place_model.py (225 scans, two laps begun, ground truth
from the generator) run through a pose_covariance = 1 handle; key frames by the policy LoopCloser uses (4 m).  For every
key-frame interval (a, b): Z = between(odometry pose a, odometry pose b), e = the edge's error of Z against the true relative
pose (graph_edge_error at the ground-truth poses), s = e^T Omega e.  If Omega is honest s is chi-square with 6 degrees of freedom:
mean 6.  Reported for the constant loop.ODOMETRY_INFO and for the chained Omega of Liodom.odometry_edges (inflation 1, no floors):
mean and quantiles of s, the inflation that brings the chained mean to 6 (s scales with 1 / inflation), and — the gate of
LoopCloser at 16.81 — the share of the run's true loop candidates that PoseGraph.gate_edges refuses under each Omega.  A true
loop candidate here is a pair (first-lap key frame i, second-lap key frame j) whose ground-truth positions are within 3 m, with
the true relative pose as its measurement and loop.LOOP_INFO: what a perfect search would hand the gate.
Written as JSON to --out and printed as the rows of DESIGN.md §5.22's tables.  No GPU: the script fails.
usage: tools/odometry_info_calibration.py [--out profiles/odometry_info_calibration.json]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GATE = 16.81
QUANTILES = (0.1, 0.5, 0.9, 0.99)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_info_calibration.json"))
    a = ap.parse_args()
    import numpy as np
    import liodom_amd as la
    from liodom_amd import api, loop, synth
    import graph_model as gm
    import place_model as pm
    if la.device_count() < 1:
        sys.exit("odometry_info_calibration: no GPU")
    synth.build()
    H, W = pm.H, pm.W_SCAN
    n_scans = pm.QUERY_SCANS[-1] + 1
    cfg = synth.make_cfg(H, W, 0, yaw_rate_deg=pm.YAW_RATE, speed=pm.SPEED)
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, max_range=pm.MAX_RANGE),
                  la.make_config(max_points=H * W, max_width=W, pose_covariance=1, pose_log_capacity=n_scans + 8))
    gt, odo = [], []
    for k in range(n_scans):
        x, t = synth.scan(cfg, 0, k)
        pose, info = g.process_scan(x, H, W)
        assert info.scan_index == k
        gt.append(gm.pose(t[:4], t[4:]))
        odo.append(gm.compose(gt[0], gm.pose(pose[:4], pose[4:])))
    gt, odo = np.stack(gt), np.stack(odo)
    policy = api.PlacePolicy(4.0)
    keys = [k for k in range(n_scans) if policy.feed(odo[k])]
    f, t = keys[:-1], keys[1:]
    rec = g.odometry_edges(0, f, t)
    cov_flags = [int(r["flags"]) for r in g.pose_covariance_log(0, 0, n_scans)]
    g.close()
    usable = rec["flags"] == api.ODOM_EDGE_VALID
    err = np.stack([gm.edge_error(gt[i], gt[j], gm.between(odo[i], odo[j])) for i, j in zip(f, t)])
    s_const = np.array([e @ loop.ODOMETRY_INFO @ e for e in err])
    s_chain = np.array([e @ r["information"] @ e for e, r in zip(err[usable], rec[usable])])

    def stats(s):
        return dict(n=int(s.shape[0]), mean=float(np.mean(s)), quantiles={str(q): float(np.quantile(s, q)) for q in QUANTILES},
                    above_gate=float(np.mean(s > GATE)))

    inflation = float(np.mean(s_chain) / 6.0)
    digits = 10.0 ** math.floor(math.log10(inflation))
    recommended = float(math.ceil(inflation / digits) * digits)           # rounded up to one significant digit

    # the gate on the run's true loop candidates
    first_lap = [n for n, k in enumerate(keys) if k < pm.N_SITE_SCANS]
    cands = [(i, j) for j in range(len(keys)) if keys[j] >= pm.N_SITE_SCANS for i in first_lap
             if j - i >= 10 and np.linalg.norm(gt[keys[i]][4:] - gt[keys[j]][4:]) <= 3.0]

    def refused(infos):
        if not cands:
            return dict(candidates=0, not_ok=0, refused_share=None, d2_median=None, d2_max=None)
        graph = api.PoseGraph(len(keys) + 1, len(keys) + len(cands) + 1)
        graph.add_nodes(odo[keys], [1] + [0] * (len(keys) - 1))
        graph.add_edges(api.graph_edges(range(len(keys) - 1), range(1, len(keys)), [gm.between(odo[i], odo[j]) for i, j in zip(f, t)], infos, kind=0))
        edges = api.graph_edges([c[0] for c in cands], [c[1] for c in cands], [gm.between(gt[keys[i]], gt[keys[j]]) for i, j in cands], loop.LOOP_INFO, kind=1)
        d2, status = graph.gate_edges(edges)
        graph.close()
        ok = status == api.GRAPH_COV_OK
        return dict(candidates=len(cands), not_ok=int(np.sum(~ok)), refused_share=float(np.mean(~ok | ~(d2 <= GATE))),
                    d2_median=float(np.median(d2[ok])) if ok.any() else None, d2_max=float(np.max(d2[ok])) if ok.any() else None)

    def chained_infos(scale):
        return np.stack([r["information"] / scale if u else loop.ODOMETRY_INFO for r, u in zip(rec, usable)])

    result = dict(scans=n_scans, key_frames=len(keys), intervals=len(f), intervals_valid=int(usable.sum()),
                  interval_scans=dict(min=int(min(b - a for a, b in zip(f, t))), max=int(max(b - a for a, b in zip(f, t)))),
                  records_not_valid=int(sum(1 for k, fl in enumerate(cov_flags) if k > 0 and fl != api.COV_VALID)),
                  error_rms=dict(rotation_half_angle=float(np.sqrt(np.mean(err[:, :3] ** 2))), translation=float(np.sqrt(np.mean(err[:, 3:] ** 2)))),
                  constant=stats(s_const), chained=stats(s_chain), inflation_to_mean_6=inflation, recommended_inflation=recommended,
                  chained_at_recommended=stats(s_chain / recommended), gate=GATE,
                  gate_constant=refused(np.repeat(loop.ODOMETRY_INFO[None], len(f), axis=0)), gate_chained=refused(chained_infos(1.0)),
                  gate_chained_at_recommended=refused(chained_infos(recommended)))
    for name in ("constant", "chained", "chained_at_recommended"):
        r = result[name]
        print("| %s | %d | %.3g | %s | %.2f |" % (name, r["n"], r["mean"], " / ".join("%.3g" % r["quantiles"][str(q)] for q in QUANTILES), r["above_gate"]))
    print("inflation that brings the chained mean to 6: %.4g (recommended: %g)" % (inflation, recommended))
    for name in ("gate_constant", "gate_chained", "gate_chained_at_recommended"):
        r = result[name]
        print("| %s | %d | %.2f | %s | %s |" % (name, r["candidates"], r["refused_share"], r["d2_median"], r["d2_max"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(result, fo, indent=1)


if __name__ == "__main__":
    main()
