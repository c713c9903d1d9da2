"""The plain-C++ half of liodom_map_register_poses (liodom_amd/csrc/map_register.h: option defaults and validation, the workspace's
sizes and byte offsets; liodom_math.h: the convergence verdict) in a program of its own, tests/map_register_main.cc, built plain
and under host sanitizers, the way test_handle_plan.py treats handle_plan.h.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import register_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}
RECORD_BYTES = 432      # sizeof(liodom_map_registration_t), held to the compiler's by test_cabi_register.py


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("register") / ("map_register_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "map_register_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def run(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    return out


def test_defaults(exe):
    assert run(exe, ["default"]) == ["default 2 1 10 6 0 0 0.0001 1.0000000000000001e-05 3 75"]
    assert run(exe, ["check", "check local_capacity=0", "check local_capacity=1", "check local_capacity=2147483647"]) == \
        ["ok 65536", "ok 65536", "ok 1", "ok 2147483647"]


def test_refusals_and_their_edges(exe):
    good = ["max_passes=1", "max_passes=16", "min_matches=1", "cells_xy=0 cells_z=0", "stop_translation=0 stop_rotation=0",
            "min_range=0 max_range=1e-300", "stop_translation=1e300"]
    bad = {"reserved=1": "reserved", "reserved=-1": "reserved", "cells_xy=-1": "extents", "cells_z=-1": "extents",
           "max_passes=0": "max_passes", "max_passes=17": "max_passes", "max_passes=-2147483648": "max_passes",
           "min_matches=0": "min_matches", "local_capacity=-1": "local_capacity", "stop_translation=-1e-300": "stop",
           "stop_rotation=-1": "stop", "stop_translation=nan": "stop", "stop_rotation=inf": "stop", "min_range=-1": "range",
           "min_range=75 max_range=75": "range", "max_range=nan": "range", "max_range=inf": "range"}
    out = run(exe, ["check " + g for g in good] + ["check " + b for b in bad])
    assert out[:len(good)] == ["ok 65536"] * len(good)
    for ln, (case, word) in zip(out[len(good):], bad.items()):
        assert ln.startswith("refused ") and word in ln, (case, ln)


def test_table_sizes(exe):
    ns = [0, 1, 4, 5, 8, 9, 1609, 65536, 65537, 1 << 29]
    out = run(exe, ["table %d" % n for n in ns])
    for n, ln in zip(ns, out):
        t = int(ln.split()[1])
        assert t >= 8 and t >= 2 * n and t & (t - 1) == 0 and (t == 8 or t // 2 < 2 * n), (n, t)


SECTIONS = ("pose", "T", "count", "pts", "order", "slot", "key", "first", "fill", "corr", "out")


def _layout(ln):
    v = [int(x) for x in ln.split()[1:]]
    return dict(zip(("table",) + SECTIONS + ("bytes",), v))


def test_layouts_do_not_overlap_and_hold_what_the_kernels_index(exe):
    cases = [(1, 1, 0), (1, 8, 1), (1, 2048, 1024), (5, 2048, 16384), (64, 2048, 16384), (1, 65536, 16384), (64, 65536, 16384), (3, 1609, 777)]
    out = run(exe, ["layout %d %d %d" % c for c in cases])
    for (rows, cap, edge_cap), ln in zip(cases, out):
        L = _layout(ln)
        table = L["table"]
        assert table >= 2 * cap and table & (table - 1) == 0
        need = dict(pose=64, T=96, count=8, pts=16 * cap, order=4 * cap, slot=4 * cap, key=8 * table, first=4 * table, fill=4 * table,
                    corr=8 * max(edge_cap, 1), out=RECORD_BYTES)
        ends = [L[s] for s in SECTIONS[1:]] + [L["bytes"]]
        assert L["pose"] == 0
        for s, end in zip(SECTIONS, ends):
            assert L[s] % 16 == 0 and end - L[s] >= rows * need[s] and end - L[s] < rows * need[s] + 16, (rows, cap, edge_cap, s)


def test_sizes_that_do_not_fit_are_refused(exe):
    out = run(exe, ["layout 0 8 8", "layout 65 8 8", "layout 1 0 8", "layout 1 8 -1", "layout 64 33554432 8", "layout 2 2147483647 8",
                    "layout 1 536870913 8", "layout 64 33554431 2147483647", "layout 1 536870912 8"])
    assert out[:7] == ["nofit"] * 7
    for ln in out[7:]:      # 64 x 2^25 - 64 points fit 2^31 - 1 and a row of 2^29 is allowed; whether the bytes fit 2^40 decides
        assert ln == "nofit" or _layout(ln)["bytes"] <= 1 << 40


def test_the_verdict_is_the_models(exe, orc, synth):
    r = rm.site_case(orc, synth, 0, rm.START_A, stop_translation=1e-6, stop_rotation=1e-7)
    prev, lines, want = rm.normalised(r["start"]), [], []
    for pose, mv in zip(r["poses"], r["moves"]):
        lines.append("verdict " + " ".join(repr(float(x)) for x in list(prev) + list(pose)) + " 1e-6 1e-7")
        want.append(mv)
        prev = pose
    lines.append("verdict 0 0 0 1 0 0 0 0 0 0 1 0 0 nan 1 1")
    out = run(exe, lines)
    for ln, (mt, mr) in zip(out, want):
        _, ok, gt, gr = ln.split()
        assert abs(float(gt) - mt) <= 1e-15 and abs(float(gr) - mr) <= 1e-15 and int(ok) == int(mt <= 1e-6 and mr <= 1e-7)
    assert out[-1].split()[1] == "0"
