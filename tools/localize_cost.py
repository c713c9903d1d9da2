#!/usr/bin/env python3
"""What localising in a saved map costs per scan.

Part 1, one stream, the HDL-64 shape of tools/mapper_step_cost.py (64 x 1800, R = 8, epr = 10, prev_frames = 15):
prefill P + 10 scans untimed, then `--scans` (200) timed scans through liodom_process_resident without read-back (the next
slot's extraction issued ahead), one device synchronise at the end.  Legs:
  a  no mapper      c  lag 1 mapper (it writes its own map: the parent commit's way to odometry that solves against a map)
  r  map reader on a site map (synth stream 0 inserted at its ground truth), the stream seeded at the traversal's first pose
With --parent-tree DIR (a checkout of the parent commit, built) legs a and c also run from that tree, alternating with this one's.

Part 2, lock-step handles of 16 and 256 streams on the cheap oracle shape (16 x 900, R = 6, epr = 10, prev_frames = 5), every
stream reading ONE map: the step through k_map_local_rows (one launch per step) against the per-stream launches of
k_map_local_plan + k_map_gather (LIODOM_MAP_ROWS=0: two launches per stream and step), and against the same handle without readers.

`--repeats` (9) rounds, every leg in a fresh child process.  Writes samples, medians and liodom_get_modes as JSON to --out.
usage: tools/localize_cost.py [--parent-tree DIR] [--repeats 9] [--scans 200] [--out profiles/localize_cost.json]"""
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
SH, SW, SR, SEPR, SP = 16, 900, 6, 10, 5
BATCH_STEPS, BATCH_PREFILL, BATCH_BASES = 40, 10, 8


def T_of(pq):
    import numpy as np
    qx, qy, qz, qw = pq[:4]
    Rm = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                   [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                   [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return np.concatenate([Rm, np.array(pq[4:]).reshape(3, 1)], axis=1)


def site_map(la, data, shape):
    """A map of the edges of data["site"] (scans) inserted at data["site_gt"] (ground-truth poses)."""
    h, w, r, epr, p = shape
    x = la.Liodom(la.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=p), la.make_config(max_points=h * w, max_width=w))
    m = la.Map(max_cells=1024, cell_capacity=32768)
    for scan, gt in zip(data["site"], data["site_gt"]):
        m.update(x.extract_edges(scan, h, w)["edges"], T_of(gt))
    x.close()
    assert m.status() == 0
    return m


def worker_single(tree, legs, data_file, n_timed):
    sys.path.insert(0, tree)
    import numpy as np
    import liodom_amd as la
    data = np.load(data_file)
    scans = data["scans"]
    K, N = scans.shape[0], H * W
    out = {}
    for leg in legs:
        g = la.Liodom(la.make_params(scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P, mapping=1),
                      la.make_config(max_points=N, max_width=W, pose_log_capacity=K + 8))
        m = None
        if leg == "c":
            m = la.Map(max_cells=1024, cell_capacity=16384)
            g.attach_mapper(m, 2, 1, lag=1)
        elif leg == "r":
            m = site_map(la, data, (H, W, R, EPR, P))
            g.attach_map_reader(m, 2, 1)
            g.seed_stream(data["gt"][0])
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
        out[leg] = dict(us=dt * 1e6, modes=g.modes(), cells=(m.num_cells() if m else 0), map_status=(m.status() if m else 0),
                        received=int(g.received_map().shape[0]), last_termination=[infos[0].lm[i].termination for i in (0, 1)],
                        last_error_t=float(np.linalg.norm(log[0][4:] - data["gt"][K - 1][4:])) if leg == "r" else None)
        if m is not None:
            g.attach_mapper(None)
            m.close()
        g.close()
    print("RESULT " + json.dumps(out), flush=True)


def worker_batch(tree, leg, data_file, S):
    """leg: 'none' (no readers), 'rows' (k_map_local_rows), 'loop' (per-stream launches; the parent process sets LIODOM_MAP_ROWS=0)."""
    sys.path.insert(0, tree)
    import numpy as np
    import liodom_amd as la
    data = np.load(data_file)
    base, gt = data["scans"], data["gt"]           # [bases, K, n, 4], [bases, K, 7]
    K, N = base.shape[1], SH * SW
    g = la.Liodom(la.make_params(scan_lines=SH, scan_regions=SR, edges_per_region=SEPR, prev_frames=SP, mapping=1),
                  la.make_config(n_streams=S, max_points=N, max_width=SW, recv_capacity=1 << 14, pose_log_capacity=K + 8))
    m = None
    if leg != "none":
        m = site_map(la, data, (SH, SW, SR, SEPR, SP))
        for s in range(S):
            g.attach_map_reader(m, 2, 1, stream=s)
            g.seed_stream(gt[s % BATCH_BASES][0], stream=s)
    g.alloc_resident(K)
    for s in range(S):
        for k in range(K):
            g.upload_scan(s, k, base[s % BATCH_BASES][k])
    g.sync()
    for k in range(BATCH_PREFILL):
        g.process_resident(k, N, SH, SW, readback=False, next_slot=k + 1)
    g.sync()
    t0 = time.perf_counter()
    for k in range(BATCH_PREFILL, K):
        g.process_resident(k, N, SH, SW, readback=False, next_slot=(k + 1 if k + 1 < K else -1))
    g.sync()
    dt = (time.perf_counter() - t0) / (K - BATCH_PREFILL)
    _, infos = g.pose_log(S - 1, K - 1, 1)
    rec = dict(us=dt * 1e6, modes=g.modes(), received=int(g.received_map(stream=S - 1).shape[0]), map_status=(m.status() if m else 0),
               last_termination=[infos[0].lm[i].termination for i in (0, 1)])
    if m is not None:
        for s in range(S):
            g.attach_mapper(None, stream=s)
        m.close()
    g.close()
    print("RESULT " + json.dumps({"%d:%s" % (S, leg): rec}), flush=True)


def run_child(args, env=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    if r.returncode != 0:
        raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--streams", default="16,256")
    ap.add_argument("--worker", default="")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--legs", default="acr")
    ap.add_argument("--data", default="")
    ap.add_argument("--n-streams", type=int, default=16)
    a = ap.parse_args()
    if a.worker == "single":
        return worker_single(a.tree, a.legs, a.data, a.scans)
    if a.worker == "batch":
        return worker_batch(a.tree, a.legs, a.data, a.n_streams)
    sys.path.insert(0, ROOT)
    import numpy as np
    from liodom_amd import synth
    samples, last = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        # part 1
        cfg = synth.make_cfg(H, W, 0)
        K = P + 10 + a.scans
        trav = [synth.scan(cfg, 1, k) for k in range(K)]
        site = [synth.scan(cfg, 0, k) for k in range(0, K, 4)]      # every fourth scan of stream 0: 0.4 m apart, the leaves are 0.4 m
        f1 = os.path.join(tmp, "single.npz")
        np.savez(f1, scans=np.stack([t[0] for t in trav]), gt=np.stack([t[1] for t in trav]), site=np.stack([t[0] for t in site]),
                 site_gt=np.stack([t[1] for t in site]))
        trees = [("this", ROOT, "acr")] + ([("parent", os.path.abspath(a.parent_tree), "ac")] if a.parent_tree else [])
        for r in range(a.repeats):
            for name, tree, legs in (trees if r % 2 == 0 else trees[::-1]):
                for leg, rec in run_child(["--worker", "single", "--tree", tree, "--legs", legs, "--data", f1, "--scans", str(a.scans)]).items():
                    samples.setdefault("1:" + name + ":" + leg, []).append(rec["us"])
                    last["1:" + name + ":" + leg] = rec
        # part 2
        cfg = synth.make_cfg(SH, SW, 0)
        K2 = BATCH_PREFILL + BATCH_STEPS
        bases = [[synth.scan(cfg, 1 + b, k) for k in range(K2)] for b in range(BATCH_BASES)]
        site = [synth.scan(cfg, 0, k) for k in range(0, K2, 2)]
        f2 = os.path.join(tmp, "batch.npz")
        np.savez(f2, scans=np.stack([np.stack([t[0] for t in b]) for b in bases]), gt=np.stack([np.stack([t[1] for t in b]) for b in bases]),
                 site=np.stack([t[0] for t in site]), site_gt=np.stack([t[1] for t in site]))
        for r in range(a.repeats):
            for S in (int(x) for x in a.streams.split(",")):
                legs = ["none", "rows", "loop"]
                for leg in (legs if r % 2 == 0 else legs[::-1]):
                    env = dict(os.environ, LIODOM_MAP_ROWS=("0" if leg == "loop" else "1"))
                    for key, rec in run_child(["--worker", "batch", "--legs", leg, "--data", f2, "--n-streams", str(S)], env=env).items():
                        samples.setdefault(key, []).append(rec["us"])
                        last[key] = rec
    rows = {}
    print("# us per scan (part 1: one stream, 64x1800) / per lock-step step (part 2: S streams, 16x900): median (min .. max) over %d repeats" % a.repeats)
    for key, xs in samples.items():
        rows[key] = dict(median_us=statistics.median(xs), min_us=min(xs), max_us=max(xs), samples_us=xs, **{k: v for k, v in last[key].items() if k != "us"})
        print("%-16s %10.2f (%10.2f .. %10.2f)  received %6d  terminations %s  map_rows=%s" % (
            key, rows[key]["median_us"], min(xs), max(xs), last[key]["received"], last[key]["last_termination"], last[key]["modes"].get("map_rows", "-")))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(part1=dict(H=H, W=W, scan_regions=R, edges_per_region=EPR, prev_frames=P, timed_scans=a.scans),
                           part2=dict(H=SH, W=SW, scan_regions=SR, edges_per_region=SEPR, prev_frames=SP, timed_steps=BATCH_STEPS, bases=BATCH_BASES),
                           repeats=a.repeats, results=rows), f, indent=1)


if __name__ == "__main__":
    main()
