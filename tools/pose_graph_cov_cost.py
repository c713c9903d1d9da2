#!/usr/bin/env python3
"""What the covariances of a pose graph and the loop gate cost.  Needs a GPU.  One job, one child process per row (each under its own
time limit); within a row every timed call is warmed up once and repeated --repeats times, and the median, the smallest and the
largest are kept.  A time is a host clock around a call that ends in a device synchronise.

  rows    drifted_ring(n, 1, n) (tests/graph_model.py) at n = 64, 257, 1 024, 4 096, 16 384 key frames — the node counts of
          DESIGN.md 5.16 —, node 0 fixed, Omega = diag(400, 400, 400, 100, 100, 100).  Per row:
          covariance_ms[q]   liodom_graph_covariance of the marginals of q = 1, 8, 42, 256 nodes spread evenly over the ring (as
                             many as the ring has free nodes): 6 q columns, one workgroup each, in as many launches as the
                             automatic plan makes (recorded), with the statuses met
          columns            liodom_graph_solve_columns of the node opposite the fixed one: iterations and |r| per column
          gate_ms            liodom_graph_gate_edges of 1 candidate and of 64 candidates (the same two nodes: 12 columns either
                             way — what is left is k_graph_gate and the copies), and the time per candidate of the 64
          The conjugate gradients stop at --max-pcg-iterations (default 200) where they have not converged to 1e-8: a long ring
          walked in steps of a metre is badly conditioned, and this tool measures time, not accuracy.
  kernels registers, LDS and occupancy of k_graph_pcg_columns, k_graph_cov_gather and k_graph_gate, read from
          profiles/pose_graph_cov_kernel_resources.txt (the compiler's resource remarks).
usage: tools/pose_graph_cov_cost.py [--repeats 5] [--max-pcg-iterations 200] [--out profiles/pose_graph_cov_cost.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = (64, 257, 1024, 4096, 16384)
QUERIES = (1, 8, 42, 256)


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), n=len(ms))


def row_worker(n, repeats, cap):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import graph_model as gm
    from liodom_amd import api
    _, poses, fixed, edges = gm.drifted_ring(n, 1, seed=n)
    g = api.PoseGraph(max_nodes=n, max_edges=len(edges))
    g.add_nodes(poses, fixed)
    g.add_edges(edges)
    opt = dict(max_pcg_iterations=cap, pcg_tolerance=1e-8)
    row = dict(nodes=n, edges=int(len(edges)), options=opt, covariance_ms={}, launches={}, statuses={})
    g.linearize()                                   # the upload and the linearisation are not what is timed

    def timed(call):
        ms = []
        for k in range(repeats + 1):               # the first round loads the code objects and is not kept
            t0 = time.perf_counter()
            out = call()
            if k:
                ms.append((time.perf_counter() - t0) * 1e3)
        return _stats(ms), out

    for q in QUERIES:
        if q > n - 1:
            continue
        nodes = (1 + (np.arange(q) * (n - 1)) // q).astype(np.int32)
        l0 = g.cov_counters()[0]
        row["covariance_ms"][str(q)], (blocks, st) = timed(lambda: g.covariance(nodes, **opt))
        row["launches"][str(q)] = (g.cov_counters()[0] - l0) // (repeats + 1)
        row["statuses"][str(q)] = {api.GRAPH_COV_STATUSES[int(s)]: int(np.sum(st == s)) for s in np.unique(st)}
    x, cst = g.solve_columns([n // 2], **opt)
    row["columns"] = dict(node=n // 2, iterations=[int(v) for v in cst["iterations"][0]], residual=[float(v) for v in cst["residual"][0]],
                          status=[api.GRAPH_COV_STATUSES[int(v)] for v in cst["status"][0]])
    one = api.graph_edges([0], [n - 1], [gm.between(poses[0], poses[n - 1])], gm.OMEGA, kind=1)
    many = np.concatenate([one] * 64)
    t1, (d2, st) = timed(lambda: g.gate_edges(one, **opt))
    t64, _ = timed(lambda: g.gate_edges(many, **opt))
    row["gate_ms"] = {"1": t1, "64": t64, "per_candidate_of_64": t64["median"] / 64.0}
    row["gate_d2"], row["gate_status"] = float(d2[0]), api.GRAPH_COV_STATUSES[int(st[0])]
    g.close()
    print("ROW " + json.dumps(row))


def kernel_resources():
    path = os.path.join(ROOT, "profiles", "pose_graph_cov_kernel_resources.txt")
    out, name = {}, None
    if not os.path.exists(path):
        return out
    with open(path) as f:
        for line in f:
            if line.startswith("Function Name:"):
                name = next((k for k in ("k_graph_pcg_columns", "k_graph_cov_gather", "k_graph_gate") if k in line), None)
                if name:
                    out[name] = {}
            elif name and ":" in line and not line.startswith("#"):
                key, value = line.strip().rsplit(":", 1)
                out[name][key.strip()] = int(value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-pcg-iterations", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_cov_cost.json"))
    ap.add_argument("--row", type=int, default=0)
    a = ap.parse_args()
    if a.row:
        row_worker(a.row, a.repeats, a.max_pcg_iterations)
        return 0
    rows = []
    for n in NODES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(n), "--repeats", str(a.repeats), "--max-pcg-iterations",
                            str(a.max_pcg_iterations)], capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            return 1                               # nothing more is started on the GPU after a row that failed
        line = [l for l in r.stdout.split("\n") if l.startswith("ROW ")][-1]
        rows.append(json.loads(line[4:]))
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/pose_graph_cov_cost.py", kernels=kernel_resources(), rows=rows), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
