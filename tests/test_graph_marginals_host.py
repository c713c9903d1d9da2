"""The plain-C++ half of the graph's covariance calls (liodom_amd/csrc/graph_marginals.h) in a program of its own
(tests/graph_marginals_main.cc), built plain and under ASan + UBSan and run as a program: the options and every refusal, the plans
at batch_columns 1, 6, 7 and automatic at node_cap 1, 4096 and 65 536, size overflow; and against tests/graph_cov_model.py the
anchoring of random graphs — several components, inactive edges, with and without fixed nodes — and the column nodes of queries
with duplicates.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_cov_model as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("graph_marginals") / ("marginals_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "graph_marginals_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_options_refusals_plans_and_overflow(exe):
    out = _run(exe, "selftest")
    assert out.startswith("ok ") and int(out.split()[1]) > 80, out


def _random_graph(rng, n, e, n_fixed, p_active):
    ei = rng.integers(0, n, e)
    ej = (ei + 1 + rng.integers(0, max(n - 1, 1), e)) % n if n > 1 else ei
    fixed = np.zeros(n, np.int32)
    if n_fixed:
        fixed[rng.choice(n, size=min(n, n_fixed), replace=False)] = 1
    active = (rng.random(e) < p_active).astype(np.int32)
    edges = np.zeros(e, [("i", "<i4"), ("j", "<i4")])
    edges["i"], edges["j"] = ei, ej
    return fixed, edges, active


def test_anchoring_of_random_graphs_equals_the_model(exe):
    rng = np.random.default_rng(23)
    seen = set()
    for n, e, n_fixed, p in ((1, 0, 0, 1.0), (1, 0, 1, 1.0), (2, 1, 1, 1.0), (2, 1, 1, 0.0), (9, 5, 1, 1.0), (9, 5, 0, 1.0), (30, 20, 2, 0.7),
                             (30, 60, 1, 0.4), (200, 150, 3, 0.8), (200, 150, 0, 0.8), (500, 420, 4, 0.9), (500, 900, 1, 0.3)):
        fixed, edges, active = _random_graph(rng, n, e, n_fixed, p)
        want = gc.anchored(fixed, edges, active)
        args = [n] + fixed.tolist() + [e] + [v for k in range(e) for v in (int(edges["i"][k]), int(edges["j"][k]), int(active[k]))]
        got = [int(v) for v in _run(exe, "anchored", *args).split()]
        assert got == want.astype(int).tolist()
        seen.add((bool(want.any()), bool((~want).any())))
    assert seen == {(True, True), (True, False), (False, True)}          # mixed, all anchored, none anchored
    assert _run(exe, "anchored", 2, 1, 0, 1, 0, 2, 1).strip() == "refused"


def test_column_nodes_of_queries_with_duplicates(exe):
    rng = np.random.default_rng(29)
    for n, nq in ((1, 3), (6, 8), (40, 100), (300, 50)):
        fixed = (rng.random(n) < 0.2).astype(int)
        anc = ((rng.random(n) < 0.7) | (fixed != 0)).astype(int)
        q = rng.integers(0, n, nq)
        lines = _run(exe, "columns", n, *fixed.tolist(), *anc.tolist(), nq, *q.tolist()).split("\n")
        want = []
        for v in q.tolist():
            if not fixed[v] and anc[v] and v not in want:
                want.append(v)
        slot = [-1] * n
        for s, v in enumerate(want):
            slot[v] = s
        assert [int(v) for v in lines[0].split()] == want and [int(v) for v in lines[1].split()] == slot
    assert _run(exe, "columns", 3, 0, 0, 0, 1, 1, 1, 1, 3).strip() == "refused"
    assert _run(exe, "columns", 3, 0, 0, 0, 1, 1, 1, 1, -1).strip() == "refused"


def test_plans(exe):
    B = 256 << 20
    for cols, cap, batch, want in ((3, 1030, 1, (18, 1, 18)), (3, 1030, 6, (18, 6, 3)), (3, 1030, 7, (18, 7, 3)), (1, 1, 0, (6, 6, 1)),
                                   (8, 4096, 0, (48, 48, 1)), (4096, 4096, 0, (24576, 273, 91)), (8, 65536, 0, (48, 17, 3)), (1, 65536, 0, (6, 6, 1))):
        got = [int(v) for v in _run(exe, "plan", cols, cap, batch, B).split()]
        assert tuple(got[:3]) == want and got[3] == 30 * cap and got[4] == want[1] * 30 * cap * 8
        assert batch > 0 or got[4] <= B or want[1] == 6
    assert _run(exe, "plan", 1, 0, 0, B).strip() == "refused"
    assert _run(exe, "plan", 1, 2 ** 62, 0, B).strip() == "refused"
