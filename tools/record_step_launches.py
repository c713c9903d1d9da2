#!/usr/bin/env python3
"""Record what the library launches for every scenario of tests/step_scenarios.py on this device.

    python tools/record_step_launches.py [-o tests/step_launches_mi355x.json] [--only NAME ...] [--no-trace]

Per scenario, each part twice, kept only if both runs agree (the tool exits with status 2 otherwise):
  launches   under `rocprofv3 --kernel-trace` (a run of its own, no counters; the traced program is a fresh child of this tool
             after `--`): per kernel instance, in dispatch order, [grid x, grid y, block, dynamic LDS bytes, repeats] with
             grids in workgroups and consecutive identical rows folded into one with a repeat count.  Launches of different
             queues have no reliable order among themselves and this trace does not name the HIP stream's role, so rows are
             compared PER KERNEL INSTANCE (the file's "compare"), never as one sequence.
  confirmed  whether the speculative hand-over of every scan in front of a chain flush was confirmed: no stand-alone repair
             launch (k_chain_redo0 of ceil(edge_cap / 256) workgroups) in the trace.  A scenario where some flushes repair and
             others do not is refused: redesign it.
  counts     without the tracer, with set_profiling(1) from the start: liodom_get_kernel_stats launches per bucket."""
import argparse
import glob
import json
import os
import re
import shutil
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import handle_matrix as hm          # noqa: E402
import step_scenarios as ss         # noqa: E402

NAME = re.compile(r"(k_[a-z0-9_]+)\s*(<[^(]*>)?")


def instance_name(demangled):
    """'void liodom_dev::k_knn<256, false, true, false>(liodom_dev::DevView, ...)' -> 'k_knn<256, false, true, false>'."""
    m = NAME.search(demangled.replace("liodom_dev::", ""))
    if not m:
        return None
    args = m.group(2) or ""
    return m.group(1) + re.sub(r"\s*,\s*", ", ", args.replace("(bool)", "").replace("(int)", ""))


def child(name, profiling):
    import liodom_amd as la
    from liodom_amd import synth
    sc = ss.SCENARIOS[ss.NAMES.index(name)]
    for k in [k for k in os.environ if k.startswith("LIODOM_")]:
        del os.environ[k]
    os.environ.update(ss.entry_of(sc)[4])
    g = ss.run(la, synth, sc, profiling=profiling)
    if profiling:
        print("COUNTS " + json.dumps({k: v[0] for k, v in g.kernel_stats().items()}), flush=True)
    dev, cus = g.device_info()
    print("DEVICE " + json.dumps([dev, cus]), flush=True)
    g.close()
    return 0


def fold(rows):
    out = []
    for r in rows:
        if out and out[-1][:4] == r:
            out[-1][4] += 1
        else:
            out.append(list(r) + [1])
    return out


def read_trace(directory):
    dbs = glob.glob(os.path.join(directory, "**", "*.db"), recursive=True)
    assert dbs, "rocprofv3 wrote no .db under " + directory
    per = {}
    for path in dbs:
        db = sqlite3.connect(path)
        cols = [c[1] for c in db.execute("pragma table_info(kernels)").fetchall()]
        need = ("name", "dispatch_id", "grid_x", "grid_y", "workgroup_x", "workgroup_y", "lds_size", "static_lds_size")
        assert all(c in cols for c in need), (path, cols)
        for name, _, gx, gy, wx, wy, lds, slds in db.execute("select %s from kernels order by dispatch_id" % ", ".join(need)):
            inst = instance_name(name)
            if inst is None:
                continue
            assert gx % wx == 0 and gy % max(1, wy) == 0, (name, gx, wx, gy, wy)
            per.setdefault(inst, []).append([gx // wx, gy // max(1, wy), wx, max(0, lds - slds)])
    return {k: fold(v) for k, v in sorted(per.items())}


def run_child(name, profiling, trace_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name] + (["--profiling"] if profiling else [])
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "-d", trace_dir, "--"] + cmd
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    tagged = {ln.split(" ", 1)[0]: json.loads(ln.split(" ", 1)[1]) for ln in r.stdout.splitlines() if ln.startswith(("COUNTS ", "DEVICE "))}
    return tagged


def record(name, trace):
    sc = ss.SCENARIOS[ss.NAMES.index(name)]
    out, ok = {"handle": sc[1]}, True
    if trace:
        runs = []
        for _ in range(2):
            d = tempfile.mkdtemp(prefix="steptrace")
            try:
                tagged = run_child(name, False, d)
                runs.append(read_trace(d))
            finally:
                shutil.rmtree(d, ignore_errors=True)
        ok = ok and runs[0] == runs[1]
        out["launches"] = runs[0]
        out["device"], out["cus"] = tagged["DEVICE"]
        # stand-alone repairs: k_chain_redo0 launches smaller than the chain-mode ones of the same trace
        redo = [r for r in runs[0].get("k_chain_redo0<256>", [])]
        small = min((r[0] for r in redo), default=0)
        flushes = sum(1 for ln in ss.requests(sc) if ln == "f")
        repairs = sum(r[4] for r in redo if r[0] == small) if len({r[0] for r in redo}) > 1 else 0
        assert repairs == 0 or repairs == flushes, "%s: %d repairs at %d flushes: redesign the scenario" % (name, repairs, flushes)
        out["confirmed"] = repairs == 0
    counts = [run_child(name, True) for _ in range(2)]
    ok = ok and counts[0]["COUNTS"] == counts[1]["COUNTS"]
    out["counts"] = counts[0]["COUNTS"]
    out.setdefault("cus", counts[0]["DEVICE"][1])
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "tests", "step_launches_mi355x.json"))
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--profiling", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.profiling)
    assert all(s[1] in hm.NAMES for s in ss.SCENARIOS)
    result = {"compare": "per_instance", "row": ["grid_x", "grid_y", "block", "dynamic_lds_bytes", "repeats"], "scenarios": {}}
    differ = []
    for name in (a.only or ss.NAMES):
        try:
            rec, ok = record(name, not a.no_trace)
        except AssertionError as ex:
            # (a child that faulted, aborted or hung: nothing more is started on the GPU)
            print("%-32s FAILED %s" % (name, str(ex)[:3000]), flush=True)
            differ.append(name)
            break
        if not ok:
            differ.append(name)
        result["scenarios"][name] = rec
        print("%-32s %s %d instances, counts %s" % (name, "ok    " if ok else "DIFFER", len(rec.get("launches", {})), rec["counts"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, separators=(",", ":"))
        f.write("\n")
    if differ:
        print("two recordings differ for: %s (redesign these scenarios)" % ", ".join(differ))
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
