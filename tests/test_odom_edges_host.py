"""The plain-C++ half of liodom_chain_odometry_edges / liodom_get_odometry_edges (liodom_amd/csrc/odom_edges.h) in a program of
its own (tests/odom_edges_main.cc), built plain and under ASan + UBSan and run as a program: the options' defaults and every
refusal, the limit of a handle's log, the range rule first <= from < to < limit at each of its edges, and n at its limit of
2^20.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("odom_edges") / ("odom_edges_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "odom_edges_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


def test_options_refusals_range_edges_and_the_count_limit(exe):
    out = _run(exe, "selftest")
    assert out.startswith("ok ") and int(out.split()[1]) >= 50, out


def test_the_range_rule_of_a_handle(exe):
    # a 32-entry log with 12 scans enqueued, nothing reset: 0 <= a < b < 12
    assert _run(exe, "limit", 12, 32) == "12" and _run(exe, "limit", 40, 32) == "32" and _run(exe, "limit", 0, 32) == "0"
    assert _run(exe, "ranges", 0, 12, 3, 0, 3, 0, 11, 10, 11) == "ok"
    assert _run(exe, "ranges", 0, 12, 2, 0, 3, 0, 12) == "refused 1"             # b == limit
    assert _run(exe, "ranges", 0, 12, 1, 3, 3) == "refused 0"                    # a == b
    assert _run(exe, "ranges", 0, 12, 1, 4, 3) == "refused 0"                    # a > b
    assert _run(exe, "ranges", 0, 12, 1, -1, 3) == "refused 0"                   # a < 0
    # the same stream seeded when it had 12 scans, 3 more since: 12 <= a < b < 15
    assert _run(exe, "ranges", 12, 15, 2, 12, 13, 12, 14) == "ok"
    assert _run(exe, "ranges", 12, 15, 1, 11, 14) == "refused 0"                 # reaches back past the seed
    assert _run(exe, "ranges", 12, 15, 1, 0, 3) == "refused 0"                   # an earlier life's records
    assert _run(exe, "ranges", 12, 15, 1, 13, 15) == "refused 0"
    # past the capacity nothing is logged: limit = capacity
    assert _run(exe, "ranges", 0, 32, 1, 30, 31) == "ok" and _run(exe, "ranges", 0, 32, 1, 30, 32) == "refused 0"
    assert _run(exe, "ranges", 0, 0, 0) == "ok"                                  # n = 0
