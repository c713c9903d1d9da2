"""The one pose rule (liodom_amd/csrc/pose7.h: seven finite numbers, | |q| - 1 | <= 1e-6, the norm as sqrt(((q0^2 + q1^2) + q2^2) +
q3^2)) in a program of its own (tests/pose7_main.cc), built plain and under AddressSanitizer + UBSan and run as a program.  The
verdicts next to the threshold are worked out here with the same float64 expression, the normalised copy is compared bit for bit
with q / norm in NumPy.  The sites that use the header keep their own tests (test_reloc_candidates.py, test_graph_csr*.py,
test_place_state_format.py, test_place_model.py).  No GPU, nothing sanitized is loaded into Python."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OK, NON_FINITE, NOT_NORMALISED = 0, 1, 2
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("pose7") / ("pose7_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "pose7_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def norm_of(q):
    q0, q1, q2, q3 = (float(x) for x in q[:4])
    return math.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)


def verdict_of(pose):
    if not all(math.isfinite(float(x)) for x in pose):
        return NON_FINITE
    return OK if abs(norm_of(pose) - 1.0) <= 1e-6 else NOT_NORMALISED


def neighbours(x, n=3):
    """x and its n nearest float64 on either side, ascending."""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], -np.inf))
        hi.append(np.nextafter(hi[-1], np.inf))
    return [float(v) for v in lo[:0:-1] + hi]


def run(exe, poses, tmp_path):
    path = tmp_path / "poses.txt"
    path.write_text("".join(" ".join("%016x" % int(np.float64(x).view(np.uint64)) for x in p) + "\n" for p in poses))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stdout[-500:] + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(poses)
    out = []
    for line in lines:
        w = line.split()
        out.append((int(w[0]), np.array([int(x, 16) for x in w[1:]], np.uint64).view(np.float64)))
    return out


def test_finite_and_zero(exe, tmp_path):
    ident = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    poses, want = [ident, [0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0], [0.0, 0.0, 0.0, -1.0, -1e300, 5e-324, 1e300]], [OK, NOT_NORMALISED, OK]
    for i in range(7):
        for bad in (float("nan"), float("inf"), float("-inf")):
            poses.append(ident[:i] + [bad] + ident[i + 1:])
            want.append(NON_FINITE)
    got = run(exe, poses, tmp_path)
    assert [g[0] for g in got] == want
    assert got[0][1].tolist() == ident and got[2][1].tolist() == poses[2]


def test_threshold_and_normalised_copy(exe, tmp_path):
    """Quaternions whose norm is 1 - 1e-6 or 1 + 1e-6 to within a few units in the last place: along one axis (the norm is |w|
    rounded once) and along a general direction, scaled by the float64 neighbours of the two boundary values."""
    rng = np.random.default_rng(7)
    u = rng.normal(size=4)
    u /= norm_of(u)
    poses = []
    for edge in (1.0 - 1e-6, 1.0 + 1e-6):
        for s in neighbours(edge, 4):
            poses.append([0.0, 0.0, 0.0, s, 1.0, -2.0, 3.0])
            poses.append([0.0, -s, 0.0, 0.0, 1.0, -2.0, 3.0])
            poses.append(list(u * s) + [0.25, 1e9, -7.0])
    want = [verdict_of(p) for p in poses]
    n = len(poses) // 2
    for half in (want[:n], want[n:]):          # each boundary is seen from both sides
        assert OK in half and NOT_NORMALISED in half and NON_FINITE not in half, half
    got = run(exe, poses, tmp_path)
    assert [g[0] for g in got] == want
    for p, (v, out) in zip(poses, got):
        if v == OK:
            q = np.array(p[:4], np.float64) / np.float64(norm_of(p))
            assert np.array_equal(out[:4].view(np.uint64), q.view(np.uint64)) and out[4:].tolist() == p[4:], p
