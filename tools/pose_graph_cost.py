#!/usr/bin/env python3
"""What optimising a pose graph costs, and how the conjugate gradients in one workgroup scale on a long chain, with the
preconditioner working along the chain and as plain block-Jacobi.  Needs a GPU.
One job, one child process per row (each under its own time limit).

  rows    chains of 64 / 1 024 / 4 096 / 16 384 key frames 1 m apart with one loop edge from the last node to the first
          (tests/graph_model.py chain), node 0 fixed, Omega = diag(400, 400, 400, 100, 100, 100), the default options but
          --max-iterations Levenberg-Marquardt steps (the long chains would otherwise run every step to the PCG cap).  Recorded per
          row: wall time of liodom_graph_optimize (a host clock around the call, which ends in a device synchronise), the report
          (LM steps, accepted steps, PCG iterations, termination, chi2 before and after), and the call's time over its PCG
          iterations — an upper bound of one iteration's time: the call also linearises, gathers and retracts.
  ring    the ring of 257 key frames of tests/test_gpu_pose_graph.py (the oracle's drift, one loop edge) with that test's options
          (pcg_tolerance 1e-10, 50 steps) and its distance to the dense solve.
  block-Jacobi   every row a second time with each odometry edge (n - 1, n, Z) stored as (n, n - 1, Z^-1): the same measurement,
          its error written in the other node's frame, the same structure of the normal equations — but no node hangs on an
          edge (n - 1, n) any more, so the preconditioner finds no chain and is plain block-Jacobi (kernels_graph.h "the preconditioner").  This is how the figures of DESIGN.md 5.16 for
          block-Jacobi are made.
  dense   the model's dense Levenberg-Marquardt (tests/graph_model.py lm, NumPy on the CPU) on the same graph where its matrix
          fits (up to 1 024 nodes): the yardstick for the result and for the step count, not a GPU time.
usage: tools/pose_graph_cost.py [--max-iterations 3] [--out profiles/pose_graph_cost.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = (64, 1024, 4096, 16384)
DENSE_LIMIT = 1024


def row_worker(n, max_iterations, ring, reverse):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import graph_model as gm
    from liodom_amd import api
    options = dict(max_iterations=max_iterations)
    if ring:
        poses, fixed, edges = gm.drifted_ring(n, 1, seed=n)[1:]
        options = dict(max_iterations=50, pcg_tolerance=1e-10)
    else:
        poses, fixed, edges = gm.chain(n, seed=n, loop=True)
    if reverse:
        edges = edges.copy()
        for k in np.nonzero(edges["j"] == edges["i"] + 1)[0]:
            i, j = int(edges["i"][k]), int(edges["j"][k])
            edges["i"][k], edges["j"][k], edges["z"][k] = j, i, gm.inverse(gm.normalised(edges["z"][k])[0])
    row = dict(graph="ring" if ring else "chain", preconditioner="block-Jacobi" if reverse else "chain", nodes=n, edges=int(len(edges)), options=options)
    g = api.PoseGraph(max_nodes=n, max_edges=len(edges))
    g.add_nodes(poses, fixed)
    g.add_edges(edges)
    g.linearize()                                  # code objects loaded, the graph uploaded: not part of the timed call
    g.set_poses(0, poses)
    t0 = time.perf_counter()
    rep = g.optimize(**options)
    row["optimize_ms"] = (time.perf_counter() - t0) * 1e3
    row["report"] = rep
    row["us_per_pcg_iteration_upper_bound"] = row["optimize_ms"] * 1e3 / max(rep["pcg_iterations"], 1)
    out = g.poses()
    g.close()
    if n <= DENSE_LIMIT:
        t0 = time.perf_counter()
        want, want_rep = gm.lm(poses, fixed, edges, max_iterations=options["max_iterations"])
        row["dense_cpu_ms"] = (time.perf_counter() - t0) * 1e3
        want_rep.pop("costs")
        row["dense_report"] = want_rep
        d = [gm.pose_distance(a, b) for a, b in zip(out, want)]
        row["worst_distance_to_dense"] = [max(x[0] for x in d), max(x[1] for x in d)]
    print("ROW " + json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-iterations", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph_cost.json"))
    ap.add_argument("--row", type=int, default=0)
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--reverse", action="store_true")
    a = ap.parse_args()
    if a.row:
        row_worker(a.row, a.max_iterations, a.ring, a.reverse)
        return 0
    rows = []
    for n, flags in [(n, f) for f in ([], ["--reverse"]) for n in NODES] + [(257, ["--ring"]), (257, ["--ring", "--reverse"])]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(n), "--max-iterations", str(a.max_iterations)] + flags,
                           capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            print(r.stdout + r.stderr)
            return 1                               # nothing more is started on the GPU after a row that failed
        line = [l for l in r.stdout.split("\n") if l.startswith("ROW ")][-1]
        rows.append(json.loads(line[4:]))
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/pose_graph_cost.py", rows=rows), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
