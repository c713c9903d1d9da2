#!/usr/bin/env python3
"""What a subset step costs: steady-state time per step of a lock-step handle that advances m of its S streams
(liodom_process_resident_subset, every S/m-th stream), beside the full step of an m-stream handle — the yardstick: a subset of m
streams should cost about what an m-stream handle's full step costs.

    tools/subset_step_bench.py --mode subset [--streams 256] [--active 256,128,64,16] [--workload hdl64]
    tools/subset_step_bench.py --mode full   [--active 256,128,64,16] [--tree DIR]

--mode subset: one S-stream handle; per m: reset, window pre-fill by full steps, then `--steps` timed steps over the list
0, S/m, 2 S/m, ... (per-step synchronous, the next step's extraction issued ahead for the same list — bench.py's batched mode).
--mode full: per m an m-stream handle whose stream i replays what stream i * S/m of the S-stream handle replays, the same steps
through process_resident.  --tree: another built checkout of the project whose package and library run instead (the parent
commit's, for the yardstick).
Per m the median over `--repeats` repeats (each from a reset) and the spread; one JSON line per m."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL = {"hdl64": (64, 1800, 0, 8, 10, 20), "vlp16": (16, 1800, 0, 8, 20, 10), "small": (16, 900, 0, 6, 10, 5)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=["subset", "full"], required=True)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--active", default="256,128,64,16")
    ap.add_argument("--workload", default="hdl64", choices=sorted(WL))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--data-streams", type=int, default=8)
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import numpy as np
    import liodom_amd as la
    from liodom_amd import synth
    synth.build()
    H, W, lt, R, epr, P = WL[a.workload]
    N, S = H * W, a.streams
    F = P + 4                                   # full window + a few warm steps
    tb = F + a.steps
    cfg = synth.make_cfg(H, W, lt)
    data = [[synth.scan(cfg, 1000 + d, k)[0] for k in range(tb)] for d in range(max(1, min(a.data_streams, S)))]
    params = la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P)

    def handle(n, source):
        g = la.Liodom(params, la.make_config(n_streams=n, max_points=N, max_width=W, pose_log_capacity=tb + 8))
        g.alloc_resident(tb)
        for s in range(n):
            for k in range(tb):
                g.upload_scan(s, k, data[source(s) % len(data)][k])
        g.sync()
        return g

    def timed(g, step):
        """One repeat: reset, pre-fill by full steps, `steps` timed steps; milliseconds per step."""
        g.reset()
        for k in range(F):
            g.process_resident(k, N, H, W, readback=True, next_slot=(k + 1 if k + 1 < F else -1))
        g.sync()
        t0 = time.perf_counter()
        for k in range(F, tb):
            step(g, k)
        g.sync()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def report(m, ms, g, extra):
        ms = sorted(ms[1:])                      # (the first repeat runs every launch shape for the first time)
        st = 0
        for s in range(int(g.config.n_streams)):
            st |= int(g.pose_log(s, tb - 1, 1)[1][0].status)
        print(json.dumps(dict(mode=a.mode, workload=a.workload, active=m, ms_per_step=round(float(np.median(ms)), 4), min=round(ms[0], 4),
                              max=round(ms[-1], 4), scans_per_s=round(m / float(np.median(ms)) * 1e3, 1), status_bits=st, **extra)), flush=True)

    actives = [int(x) for x in a.active.split(",")]
    if a.mode == "subset":
        g = handle(S, lambda s: s)
        for m in actives:
            L = list(range(0, S, S // m))[:m]

            def step(g, k, L=L):
                g.process_resident_subset(k, L, N, H, W, readback=True, next_slot=(k + 1 if k + 1 < tb else -1), next_streams=L)
            ms = [timed(g, step) for _ in range(a.repeats + 1)]
            report(m, ms, g, dict(streams=S, subset_steps=int(g.modes()["subset_steps"])))
        g.close()
    else:
        for m in actives:
            g = handle(m, lambda s, m=m: s * (S // m))

            def step(g, k):
                g.process_resident(k, N, H, W, readback=True, next_slot=(k + 1 if k + 1 < tb else -1))
            ms = [timed(g, step) for _ in range(a.repeats + 1)]
            report(m, ms, g, dict(streams=m, tree=a.tree or "this"))
            g.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
