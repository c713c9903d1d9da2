#!/usr/bin/env python3
"""Per-scan cost of the mapper modes of a mapping handle (mapping = 1, one stream) on the HDL-64 shape 64 x 1800, R = 8, epr = 10,
prev_frames = 15: prefill P + 10 scans untimed, then `--scans` (200) timed scans through liodom_process_resident without
read-back (the next slot's extraction issued ahead), one device synchronise at the end.  Legs:
  a  no mapper                      b  liodom_attach_mapper (lag 0: the reference's loop)
  c  lag 1                          d  lag 1 with prune_period 10, keep box = the getLocalMap extent (2, 1)
`--repeats` (9) rounds; every round runs each leg once, in a fresh child process per tree so that no leg inherits a warm handle.
With --parent-tree DIR (a checkout of the parent commit, built) legs a and b also run from that tree in every round, alternating
with this tree's: the claim to check is that a and b do not change, against the spread of the parent's own repeats.
Writes the samples, the medians and liodom_get_modes of every leg as JSON to --out.
usage: tools/mapper_step_cost.py [--parent-tree DIR] [--repeats 9] [--scans 200] [--out profiles/mapper_lag_cost.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, R, EPR, P = 64, 1800, 8, 10, 15
N = H * W
LEGS = {"a": None, "b": dict(), "c": dict(lag=1), "d": dict(lag=1, prune_period=10, keep_cells_xy=2, keep_cells_z=1)}


def worker(tree, legs, scans_file, n_timed):
    """One repeat of `legs` with the package of `tree`; prints one JSON line."""
    sys.path.insert(0, tree)
    import numpy as np
    import liodom_amd as la
    scans = np.load(scans_file, mmap_mode="r")
    K = scans.shape[0]
    out = {}
    for leg in legs:
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                      la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8))
        m = None
        if LEGS[leg] is not None:
            m = la.Map(max_cells=1024, cell_capacity=16384)
            g.attach_mapper(m, 2, 1, **LEGS[leg])
        g.alloc_resident(K)
        for k in range(K):
            g.upload_scan(0, k, scans[k])
        g.sync()
        pre = K - n_timed
        for k in range(pre):
            g.process_resident(k, N, H, W, readback=False, next_slot=k + 1)
        g.sync()
        t0 = time.perf_counter()
        for k in range(pre, K):
            g.process_resident(k, N, H, W, readback=False, next_slot=(k + 1 if k + 1 < K else -1))
        g.sync()
        dt = (time.perf_counter() - t0) / n_timed
        log, infos = g.pose_log(0, K - 1, 1)
        out[leg] = dict(s_per_scan=dt, modes=g.modes(), cells=(m.num_cells() if m else 0), map_status=(m.status() if m else 0),
                        last_termination=[infos[0].lm[i].termination for i in (0, 1)], last_translation=[float(x) for x in log[0][4:]])
        if m is not None:
            g.attach_mapper(None)
            m.close()
        g.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(tree, legs, scans_file, n_timed):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--legs", legs, "--scans-file", scans_file, "--scans", str(n_timed)]
    txt = subprocess.run(cmd, capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--scans-file", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.legs, a.scans_file, a.scans)
    sys.path.insert(0, ROOT)
    import numpy as np
    from liodom_amd import synth
    cfg = synth.make_cfg(H, W, 0)
    K = P + 10 + a.scans
    with tempfile.TemporaryDirectory() as tmp:
        scans_file = os.path.join(tmp, "scans.npy")
        np.save(scans_file, np.stack([synth.scan(cfg, 0, k)[0].astype(np.float32).reshape(-1, 4) for k in range(K)]))
        trees = [("this", ROOT, a.legs)] + ([("parent", os.path.abspath(a.parent_tree), "ab")] if a.parent_tree else [])
        samples, last = {}, {}
        for r in range(a.repeats):
            for name, tree, legs in (trees if r % 2 == 0 else trees[::-1]):
                for leg, rec in run_worker(tree, legs, scans_file, a.scans).items():
                    samples.setdefault(name + ":" + leg, []).append(rec["s_per_scan"] * 1e6)
                    last[name + ":" + leg] = rec
    rows = {}
    print("# mapping handle, 64x1800 R=8 epr=10 P=%d, %d timed scans after %d untimed, %d repeats: us/scan median (min .. max)" % (P, a.scans, P + 10, a.repeats))
    for key, xs in samples.items():
        rows[key] = dict(median_us=statistics.median(xs), min_us=min(xs), max_us=max(xs), samples_us=xs, cells=last[key]["cells"],
                         map_status=last[key]["map_status"], last_termination=last[key]["last_termination"],
                         last_translation=last[key]["last_translation"], modes=last[key]["modes"])
        print("%-10s %9.2f (%9.2f .. %9.2f)  cells %4d  terminations %s  mapper_lag=%s" % (
            key, rows[key]["median_us"], min(xs), max(xs), last[key]["cells"], last[key]["last_termination"], last[key]["modes"].get("mapper_lag", "-")))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, prev_frames=P, timed_scans=a.scans, repeats=a.repeats),
                           legs={k: (v if v is not None else "no mapper") for k, v in LEGS.items()}, results=rows), f, indent=1)


if __name__ == "__main__":
    main()
