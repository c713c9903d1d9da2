#!/usr/bin/env python3
"""What the per-scan map-hit records (liodom_set_map_hits) cost a reader step.

Lock-step handles of 1 and 256 streams on the cheap oracle shape (16 x 900, R = 6, epr = 10, prev_frames = 5), every stream reading
ONE site map (synth stream 0 inserted at its ground truth) and seeded at its traversal's first pose, as part 2 of
tools/localize_cost.py.  Legs, every one in a fresh child process, alternating in one job:
  off   the reader step as it was        r0   hits on, radius 0        r1   hits on, radius 1
Timed: BATCH_STEPS steps through liodom_process_resident without read-back, one device synchronise at the end.  Then, in the same
child, the same steps again with liodom_set_profiling: the HIP-event time of the "other" bucket per step (the map block's scopes —
k_map_local_rows in one, the hit launches in another — and nothing else on a handle without pose covariance); the difference of
that figure between a hits leg and the off leg is the kernels' share: k_map_hit_rows, plus the occupancy's two kernels in the one
step that builds it.
usage: tools/map_hits_cost.py [--repeats 5] [--streams 1,256] [--out profiles/map_hits_cost.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SH, SW, SR, SEPR, SP = 16, 900, 6, 10, 5
BATCH_STEPS, BATCH_PREFILL, BATCH_BASES = 40, 10, 8
LEGS = {"off": -1, "r0": 0, "r1": 1}


def worker(leg, data_file, S):
    sys.path.insert(0, ROOT)
    import numpy as np
    import liodom_amd as la
    from localize_cost import site_map
    data = np.load(data_file)
    base, gt = data["scans"], data["gt"]           # [bases, K, n, 4], [bases, K, 7]
    K, N = base.shape[1], SH * SW
    g = la.Liodom(la.make_params(scan_lines=SH, scan_regions=SR, edges_per_region=SEPR, prev_frames=SP, mapping=1),
                  la.make_config(n_streams=S, max_points=N, max_width=SW, recv_capacity=1 << 14, pose_log_capacity=2 * K + 8))
    m = site_map(la, data, (SH, SW, SR, SEPR, SP))
    for s in range(S):
        g.attach_map_reader(m, 2, 1, stream=s)
        if LEGS[leg] >= 0:
            g.set_map_hits(LEGS[leg], stream=s)
    g.alloc_resident(K)
    for s in range(S):
        for k in range(K):
            g.upload_scan(s, k, base[s % BATCH_BASES][k])

    def run(profiled):
        for s in range(S):
            g.seed_stream(gt[s % BATCH_BASES][0], stream=s)
        g.sync()
        for k in range(BATCH_PREFILL):
            g.process_resident(k, N, SH, SW, readback=False, next_slot=k + 1)
        g.sync()
        if profiled:
            g.set_profiling(True)
            g.reset_kernel_stats()
        t0 = time.perf_counter()
        for k in range(BATCH_PREFILL, K):
            g.process_resident(k, N, SH, SW, readback=False, next_slot=(k + 1 if k + 1 < K else -1))
        g.sync()
        dt = (time.perf_counter() - t0) / (K - BATCH_PREFILL)
        other = None
        if profiled:
            launches, ms = g.kernel_stats()["other"]
            other = dict(scopes_per_step=launches / (K - BATCH_PREFILL), us_per_step=1e3 * ms / (K - BATCH_PREFILL))
            g.set_profiling(False)
        return dt * 1e6, other

    us, _ = run(False)
    _, other = run(True)
    hit = g.map_hits(K - 1, 1, stream=S - 1)[0] if LEGS[leg] >= 0 else None
    rec = dict(us=us, other=other, modes=g.modes(), map_status=m.status(), cells=m.num_cells(),
               last_hit=(None if hit is None else [int(hit["hits_r"]), int(hit["hits_0"]), int(hit["n_edges"]), int(hit["flags"])]))
    for s in range(S):
        g.attach_mapper(None, stream=s)
    m.close()
    g.close()
    print("RESULT " + json.dumps({"%d:%s" % (S, leg): rec}), flush=True)


def run_child(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", default="1,256")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--data", default="")
    ap.add_argument("--n-streams", type=int, default=1)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.data, a.n_streams)
    sys.path.insert(0, ROOT)
    import numpy as np
    from liodom_amd import synth
    samples, other, last = {}, {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        cfg = synth.make_cfg(SH, SW, 0)
        K = BATCH_PREFILL + BATCH_STEPS
        bases = [[synth.scan(cfg, 1 + b, k) for k in range(K)] for b in range(BATCH_BASES)]
        site = [synth.scan(cfg, 0, k) for k in range(0, K, 2)]
        f = os.path.join(tmp, "batch.npz")
        np.savez(f, scans=np.stack([np.stack([t[0] for t in b]) for b in bases]), gt=np.stack([np.stack([t[1] for t in b]) for b in bases]),
                 site=np.stack([t[0] for t in site]), site_gt=np.stack([t[1] for t in site]))
        for r in range(a.repeats):
            for S in (int(x) for x in a.streams.split(",")):
                legs = list(LEGS)
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    for key, rec in run_child(["--worker", leg, "--data", f, "--n-streams", str(S)]).items():
                        samples.setdefault(key, []).append(rec["us"])
                        other.setdefault(key, []).append(rec["other"]["us_per_step"])
                        last[key] = rec
    rows = {}
    print("# us per lock-step step (S streams, 16x900): median (min .. max) over %d repeats; 'other': HIP-event time of the map block's scopes per step, profiled run" % a.repeats)
    for key, xs in samples.items():
        rows[key] = dict(median_us=statistics.median(xs), min_us=min(xs), max_us=max(xs), samples_us=xs, other_median_us=statistics.median(other[key]),
                         other_samples_us=other[key], **{k: v for k, v in last[key].items() if k != "us"})
        print("%-8s %10.2f (%10.2f .. %10.2f)  other %8.2f us in %.1f scopes  last hit %s  map_hits=%s" % (
            key, rows[key]["median_us"], min(xs), max(xs), rows[key]["other_median_us"], last[key]["other"]["scopes_per_step"], last[key]["last_hit"],
            last[key]["modes"].get("map_hits", "-")))
    if a.out:
        with open(a.out, "w") as fo:
            json.dump(dict(H=SH, W=SW, scan_regions=SR, edges_per_region=SEPR, prev_frames=SP, timed_steps=BATCH_STEPS, bases=BATCH_BASES,
                           repeats=a.repeats, results=rows), fo, indent=1)


if __name__ == "__main__":
    main()
