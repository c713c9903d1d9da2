#!/usr/bin/env python3
"""Cost of the per-scan pose covariance (config.pose_covariance = 1: the finalising solve's store + k_pose_cov per scan), measured
as interleaved repeats of the same replay with the switch 0 and 1 on one GPU:
  headline  chain-mode replay (liodom_replay_resident, depth 1) of the HDL-64-shape stream 64 x 1800, R = 8, epr = 10, P = 20:
            prefill P + 10 scans untimed, then `--scans` timed; one handle per repeat (chain mode needs the GPU to one handle)
  batch     256 lock-step streams of the same shape (liodom_process_resident over resident slots, no read-back, the next slot's
            extraction issued ahead), 8 distinct data streams; both handles live, liodom_reset before every repeat
Prints one table and writes it (and the raw samples as JSON) to --out.  usage: tools/pose_cov_cost.py [--repeats 5] [--out file]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import liodom_amd as la  # noqa: E402
from liodom_amd import synth  # noqa: E402

H, W, R, EPR, P = 64, 1800, 8, 10, 20
N = H * W


def headline_once(scans, cov, n_timed):
    K = len(scans)
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P),
                  la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8, pose_covariance=cov))
    g.alloc_resident(K)
    for k in range(K):
        g.upload_scan(0, k, scans[k])
    g.sync()
    pre = K - n_timed
    g.replay_resident(0, pre, N, H, W, ahead=True, depth=1)
    t0 = time.perf_counter()
    g.replay_resident(pre, n_timed, N, H, W, depth=1)
    dt = time.perf_counter() - t0
    modes = g.modes()
    g.close()
    return dt / n_timed, modes


def batch_handles(S, K, D):
    cfg = synth.make_cfg(H, W, 0)
    data = [[synth.scan(cfg, 50 + d, k)[0] for k in range(K)] for d in range(D)]
    hs = {}
    for cov in (0, 1):
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P),
                      la.make_config(n_streams=S, max_points=N, max_width=W, pose_log_capacity=K + 8, pose_covariance=cov))
        g.alloc_resident(K)
        for s in range(S):
            for k in range(K):
                g.upload_scan(s, k, data[s % D][k])
        g.sync()
        hs[cov] = g
    return hs


def batch_once(g, K, warm):
    g.reset()
    for k in range(warm):
        g.process_resident(k, N, H, W, readback=False, next_slot=k + 1)
    g.sync()
    t0 = time.perf_counter()
    for k in range(warm, K):
        g.process_resident(k, N, H, W, readback=False, next_slot=(k + 1 if k + 1 < K else -1))
    g.sync()
    return (time.perf_counter() - t0) / (K - warm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scans", type=int, default=150)
    ap.add_argument("--batch-streams", type=int, default=256)
    ap.add_argument("--batch-scans", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cfg = synth.make_cfg(H, W, 0)
    scans = [synth.scan(cfg, 0, k)[0] for k in range(P + 10 + a.scans)]
    res = {"headline": {0: [], 1: []}, "batch": {0: [], 1: []}}
    modes = {}
    for r in range(a.repeats):
        for cov in ((0, 1) if r % 2 == 0 else (1, 0)):
            dt, m = headline_once(scans, cov, a.scans)
            res["headline"][cov].append(dt)
            modes[cov] = m
    S, K = a.batch_streams, a.batch_scans
    hs = batch_handles(S, K, 8)
    for r in range(a.repeats):
        for cov in ((0, 1) if r % 2 == 0 else (1, 0)):
            res["batch"][cov].append(batch_once(hs[cov], K, 4))
    for g in hs.values():
        g.close()
    lines = ["# pose covariance cost: interleaved repeats, pose_covariance 0 vs 1 (median, min .. max of %d repeats)" % a.repeats,
             "# headline: chain-mode replay_resident depth 1, 64x1800 R=8 epr=10 P=20, %d timed scans after %d untimed" % (a.scans, P + 10),
             "# batch: %d lock-step streams, same shape, process_resident without read-back, scans 4..%d of %d resident" % (S, K - 1, K),
             "# modes (switch on): chain=%s lm_groups=%s pose_cov=%s" % (modes[1].get("chain"), modes[1].get("lm_groups"), modes[1].get("pose_cov")),
             "%-10s %-4s %12s %22s %12s" % ("workload", "cov", "us/scan", "min .. max", "scans/s")]
    for wl, unit in (("headline", 1), ("batch", S)):
        med = {}
        for cov in (0, 1):
            xs = [x * 1e6 for x in res[wl][cov]]
            med[cov] = statistics.median(xs)
            lines.append("%-10s %-4d %12.2f %10.2f .. %-9.2f %12.0f" % (wl, cov, med[cov], min(xs), max(xs), unit * 1e6 / med[cov]))
        lines.append("%-10s cost of the switch: %+.2f us per step (%+.2f %%)" % (wl, med[1] - med[0], 100.0 * (med[1] - med[0]) / med[0]))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
        with open(os.path.splitext(a.out)[0] + ".json", "w") as f:
            json.dump({"samples_s": res, "modes": modes}, f, indent=1)


if __name__ == "__main__":
    main()
