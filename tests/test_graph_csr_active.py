"""The CSR and the preconditioner's chain of a pose graph with switched-off edges (liodom_amd/csrc/graph_csr.h: graph_build_csr with
an active mask, graph_chain_parents) in a program of its own (tests/graph_csr_active_main.cc), built plain and under ASan + UBSan and
run as a program: all inactive, the chain edge (n - 1, n) inactive beside an active duplicate, a node left without active edges, a
fixed node; random graphs with random masks against lists made here; and the mask nullptr against what graph_csr_main.cc's program
prints for the same graphs.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


def _build(tmp_path_factory, source, kind):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the CSR programs"
    if (source, kind) not in _EXE:
        out = str(tmp_path_factory.mktemp("graph_csr_active") / (source.replace(".cc", "_") + kind))
        flags = ["-O2"] if kind == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", source)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[(source, kind)] = out
    return _EXE[(source, kind)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    return _build(tmp_path_factory, "graph_csr_active_main.cc", request.param)


def test_the_designed_masks(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) >= 25


def _expected(n, ei, ej, act, fixed):
    lists = [[] for _ in range(n)]
    parent = [-1] * n
    for e, (i, j, a) in enumerate(zip(ei, ej, act)):
        if not a:
            continue
        lists[i].append(2 * e)
        lists[j].append(2 * e + 1)
        if j == i + 1 and j not in fixed and parent[j] < 0:
            parent[j] = e
    off = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(int).tolist()
    return off, [v for node in lists for v in node], parent


def _random_graph(rng, n, e):
    ei = rng.integers(0, n, e).tolist()
    ej = [int((i + 1 + rng.integers(0, max(n - 1, 1))) % n) for i in ei] if n > 1 else []
    for k in range(0, e, 3):                   # a third of the edges are chain edges (i, i + 1), some of them duplicates
        if ei[k] + 1 < n:
            ej[k] = ei[k] + 1
    return ei, ej


def _run(exe, n, mode, ei, ej, act, fixed=()):
    args = [exe, "csr", str(n), mode] + [str(v) for t in zip(ei, ej, act) for v in t] + (["fixed"] + [str(v) for v in fixed] if fixed else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return [[int(v) for v in line.split()] for line in r.stdout.split("\n")[:3]]


def test_random_graphs_with_random_masks(exe):
    rng = np.random.default_rng(23)
    for n, e in ((1, 0), (2, 1), (5, 12), (40, 200), (300, 299)):
        ei, ej = _random_graph(rng, n, e)
        fixed = sorted(set([0] + rng.integers(0, n, n // 8).tolist()))
        for act in ([1] * e, [0] * e, rng.integers(0, 2, e).tolist()):
            off, ent, par = _run(exe, n, "mask", ei, ej, act, fixed)
            assert [off, ent, par] == list(_expected(n, ei, ej, act, fixed)), (n, e)


def test_a_null_mask_is_what_it_always_was(exe, tmp_path_factory):
    """The graphs of test_graph_csr.py's random test through both programs: graph_csr_main.cc calls graph_build_csr as it did before
    a mask existed; this program reads flags of zero and passes nullptr.  Equal text; the parents are those of every edge."""
    old = _build(tmp_path_factory, "graph_csr_main.cc", "plain")
    rng = np.random.default_rng(17)
    for n, e in ((1, 0), (2, 1), (5, 12), (40, 200), (300, 299)):
        ei = rng.integers(0, n, e).tolist()
        ej = [int((i + 1 + rng.integers(0, max(n - 1, 1))) % n) for i in ei] if n > 1 else []
        r = subprocess.run([old, "csr", str(n)] + [str(v) for pair in zip(ei, ej) for v in pair], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        was = [[int(v) for v in line.split()] for line in r.stdout.split("\n")[:2]]
        off, ent, par = _run(exe, n, "null", ei, ej, [0] * e)
        assert [off, ent] == was
        assert par == _expected(n, ei, ej, [1] * e, ())[2]
    r = subprocess.run([exe, "csr", "3", "mask", "0", "3", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused"
