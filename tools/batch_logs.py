#!/usr/bin/env python3
"""Continuous batching: N logs of unequal length through an S-stream lock-step handle with S < N.  Every slot (stream) replays one
log; when its log ends the slot is reset (liodom_reset_stream) and takes the next log in line, while the other slots go on.  A slot with no
log left is fed its last scan again and its result is dropped (the default), or — with --sit-out — left out of the step
(liodom_process_resident_subset): the step then runs over the busy slots only and the GPU processes no scan that does not count.

    tools/batch_logs.py [--streams 16] [--logs 24] [--min-len 6] [--max-len 40] [--shape 16x900] [--sit-out] [--out DIR]

replays synthetic logs, prints aggregate scans/s and writes DIR/log_NNN.txt (one pose per line: qx qy qz qw tx ty tz).
run(g, logs, H, W, sit_out=False) is the loop itself, for callers with their own handle and clouds."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(g, logs, H, W, sit_out=False):
    """logs[i][k]: scan k of log i (float32 [H * W, 4]).  sit_out: idle slots are left out of the step instead of being fed their
    last scan.  Returns dict(poses = per log its [len, 7] poses, slot_of_log, steps, scans, gpu_scans = scans the GPU processed
    (counted or dropped), seconds, status_bits = OR of the status bits of every scan that counted)."""
    S = int(g.config.n_streams)
    n = H * W
    queue = list(range(len(logs)))
    cur = [None] * S               # log a slot replays
    pos = [0] * S                  # next scan of that log
    last = [None] * S              # what an idle slot is fed
    poses = {i: [] for i in range(len(logs))}
    slot_of_log = {}
    status = 0
    steps = scans = gpu_scans = 0
    g.alloc_resident(1)
    t0 = time.perf_counter()
    while True:
        for s in range(S):
            if cur[s] is not None and pos[s] == len(logs[cur[s]]):
                cur[s] = None
            if cur[s] is None and queue:
                cur[s], pos[s] = queue.pop(0), 0
                slot_of_log[cur[s]] = s
                if steps:
                    g.reset_stream(s)          # the slot's next scan is the first of its new log
        if all(c is None for c in cur):
            break
        active = [s for s in range(S) if cur[s] is not None] if sit_out else list(range(S))
        for s in active:
            if cur[s] is not None:
                last[s] = logs[cur[s]][pos[s]]
            elif last[s] is None:
                last[s] = next(logs[c][0] for c in cur if c is not None)
            g.upload_scan(s, 0, last[s])
        if sit_out:
            out, infos = g.process_resident_subset(0, active, n, H, W, readback=True)
        else:
            out, infos = g.process_resident(0, n, H, W, readback=True)
        steps += 1
        gpu_scans += len(active)
        for i, s in enumerate(active):
            if cur[s] is None:
                continue
            poses[cur[s]].append(out[i].copy())
            status |= int(infos[i].status)
            pos[s] += 1
            scans += 1
    secs = time.perf_counter() - t0
    return dict(poses={i: np.array(p).reshape(-1, 7) for i, p in poses.items()}, slot_of_log=slot_of_log, steps=steps, scans=scans, gpu_scans=gpu_scans,
                seconds=secs, status_bits=status)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--logs", type=int, default=24)
    ap.add_argument("--min-len", type=int, default=6)
    ap.add_argument("--max-len", type=int, default=40)
    ap.add_argument("--shape", default="16x900")
    ap.add_argument("--prev-frames", type=int, default=5)
    ap.add_argument("--sit-out", action="store_true", help="leave idle slots out of the step instead of feeding them their last scan")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import liodom_amd as la
    from liodom_amd import synth
    synth.build()
    H, W = (int(x) for x in a.shape.split("x"))
    cfg = synth.make_cfg(H, W, 0)
    rng = np.random.default_rng(0)
    lengths = rng.integers(a.min_len, a.max_len + 1, a.logs)
    logs = [[synth.scan(cfg, i, k)[0] for k in range(int(lengths[i]))] for i in range(a.logs)]
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=6 if H <= 16 else 8, prev_frames=a.prev_frames),
                  la.make_config(n_streams=a.streams, max_points=H * W, max_width=W))
    r = run(g, logs, H, W, sit_out=a.sit_out)
    g.close()
    print("%d logs (%d scans) through %d streams in %d lock-step steps%s, %d scans processed by the GPU: %.0f scans/s aggregate (uploads included), status bits 0x%x"
          % (a.logs, r["scans"], a.streams, r["steps"], " (idle slots sit out)" if a.sit_out else "", r["gpu_scans"], r["scans"] / r["seconds"], r["status_bits"]))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        for i, p in r["poses"].items():
            np.savetxt(os.path.join(a.out, "log_%03d.txt" % i), p, fmt="%.17g")
    return 0 if r["status_bits"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
