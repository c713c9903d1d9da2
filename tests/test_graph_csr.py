"""The host-side bookkeeping of a pose graph (liodom_amd/csrc/graph_csr.h) in a program of its own (tests/graph_csr_main.cc), built
plain and under ASan + UBSan and run as a program: every refusal of an edge (indices, i == j, Z, Omega), degrees 0, 1 and 1025, the
maximal indices and counts; and the CSR of random graphs against one made here.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the CSR program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("graph_csr") / ("csr_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "graph_csr_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def test_refusals_degrees_and_limits(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 300


def _csr(n, ei, ej):
    lists = [[] for _ in range(n)]
    for e, (i, j) in enumerate(zip(ei, ej)):
        lists[i].append(2 * e)
        lists[j].append(2 * e + 1)
    off = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(int).tolist()
    return off, [v for node in lists for v in node]


def test_the_csr_of_random_graphs(exe):
    rng = np.random.default_rng(17)
    for n, e in ((1, 0), (2, 1), (5, 12), (40, 200), (300, 299)):
        ei = rng.integers(0, n, e).tolist()
        ej = [int((i + 1 + rng.integers(0, max(n - 1, 1))) % n) for i in ei] if n > 1 else []
        args = [exe, "csr", str(n)] + [str(v) for pair in zip(ei, ej) for v in pair]
        r = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.split("\n")
        off, ent = _csr(n, ei, ej)
        assert [int(v) for v in lines[0].split()] == off and [int(v) for v in lines[1].split()] == ent
    r = subprocess.run([exe, "csr", "3", "0", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused"
