#!/usr/bin/env python3
"""Wall time of liodom_reset_stream / liodom_export_stream_state / liodom_import_stream_state (the calls synchronise by design):
on a one-stream handle and on one stream of a 256-stream lock-step handle, 64 x 1800, P = 20, full window.  On the batch handle the
other 255 streams stall for as long as the call lasts (it holds both sides and waits for the handle's HIP streams), so the call's
wall time IS their stall; the step time of the batch is printed beside it.
usage: tools/stream_state_cost.py [--streams 1,256] [--reps 9] > profiles/stream_state_cost.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import liodom_amd as la
from liodom_amd import synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,256")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    synth.build()
    H, W, P, D = 64, 1800, 20, 4
    K = P + 4
    cfg = synth.make_cfg(H, W, 0)
    data = [[synth.scan(cfg, d, k)[0] for k in range(K)] for d in range(D)]
    print("# tools/stream_state_cost.py: wall time of the per-stream calls, microseconds, median [min - max] of %d; 64 x 1800, P = %d, "
          "window full (%d scans)" % (a.reps, P, K))
    for S in (int(x) for x in a.streams.split(",")):
        g = la.Liodom(la.make_params(scan_lines=H, prev_frames=P), la.make_config(n_streams=S, max_points=H * W, max_width=W))
        g.alloc_resident(K)
        for s in range(S):
            for k in range(K):
                g.upload_scan(s, k, data[s % D][k])
        step = []
        for k in range(K):
            t0 = time.perf_counter()
            g.process_resident(k, H * W, H, W, readback=True)
            step.append((time.perf_counter() - t0) * 1e6)
        g.sync()
        s = S // 2
        t = {"export": [], "import": [], "reset_stream": []}
        blob = g.export_stream_state(s)          # (first call: allocates the staging buffers)
        for _ in range(a.reps):
            t0 = time.perf_counter(); blob = g.export_stream_state(s); t["export"].append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter(); g.import_stream_state(s, blob); t["import"].append((time.perf_counter() - t0) * 1e6)
        for _ in range(a.reps):
            t0 = time.perf_counter(); g.reset_stream(s); t["reset_stream"].append((time.perf_counter() - t0) * 1e6)
            g.import_stream_state(s, blob)
        m = g.modes()
        print("n_streams=%d (hash_build=%s early_rebuild=%s): blob %d bytes; lock-step step %.0f us (median of the last %d)"
              % (S, m["hash_build"], m["early_rebuild"], len(blob), statistics.median(step[-8:]), 8))
        for name in ("reset_stream", "export", "import"):
            v = t[name]
            print("  %-13s %8.0f [%.0f - %.0f]%s" % (name, statistics.median(v), min(v), max(v),
                                                    "   = stall of the other %d streams" % (S - 1) if S > 1 else ""))
        g.close()


if __name__ == "__main__":
    main()
