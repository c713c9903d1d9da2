"""graph_loss of liodom_math.h — the robust losses of the pose graph, shared by host and device — compiled for the host in a program
of its own (tests/graph_loss_host.cc, -ffp-contract=off, ASan + UBSan; it has its own main, nothing sanitized is loaded into Python)
and held to mpmath at 50 digits on a grid: s = 0, 1e-300, c^2 (1 -+ 1e-15), c^2, 1e-8 ... 1e12 by decades, 1e300; c = 1e-3, 1, 5,
1e150.  (c^2 is taken as the double nearest to it; at c = 1e150 that is 1e300, the largest s of the grid.)

The bound, from the operation count of each formula.  u = 2^-53 is the relative error of one correctly rounded operation (+, -, *,
/, and sqrt: IEEE 754 rounds it correctly); log1p of the host's libm is within 1 ulp = 2 u (glibc documents 1 ulp for double).  A
relative error of an argument goes through a function times its condition number, which is <= 1 for 1 / (1 + x), x >= 0, and for
log1p(x), x >= 0 (x / ((1 + x) log1p(x)) <= 1).
  Huber, s > c^2     rho = c (2 sqrt(s) - c): sqrt u, doubled in 2 sqrt(s) - c >= sqrt(s): 2 u; the subtraction u; the product u    4 u
                     w = c / sqrt(s): sqrt u, the division u; and where | sqrt(s) - c | <= u c the code and the exact comparison
                     s <= c^2 may take different branches, which are then u apart (w) and u^2 apart (rho)                         3 u
  Cauchy             x = (s / c) / c: 2 u.   w = 1 / (1 + x): x 2 u, the sum u, the division u                                    4 u
                     rho = c (c log1p(x)): x 2 u, log1p 2 u, two products 2 u; and rho = s where x < 2^-54 (exact: s (1 - x / 2 +
                     ...), within u / 4)                                                                                          6 u
  Geman-McClure      q = 1 / (1 + x): 4 u as Cauchy's w.   rho = s q                                                              5 u
                     w = q q: 4 u twice and the product                                                                           9 u
  none, Huber s <= c^2, s = 0:  rho = s and w = 1 exactly                                                                          0
Added to each: 2^-1022, the underflow threshold — w = q q of Geman-McClure at s = 1e300, c = 1e-3 is 1e-612 and comes out 0.
These are bounds on the worst case, not estimates; the test prints the share of them that is used.  The device's libm (sqrt
correctly rounded, log1p within 2 ulp) adds 2 u to Cauchy's rho and nothing else: tests/test_gpu_pose_graph_robust.py uses 8 u."""
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
U = 2.0 ** -53
TINY = 2.0 ** -1022
LOSSES = ("none", "huber", "cauchy", "geman_mcclure")
BOUND_U = {"none": (0, 0), "huber": (4, 3), "cauchy": (6, 4), "geman_mcclure": (5, 9)}          # (rho, w) in units of u
SCALES = (1e-3, 1.0, 5.0, 1e150)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the loss program"
    out = str(tmp_path_factory.mktemp("graph_loss") / "graph_loss_host")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + SAN +
                       ["-o", out, os.path.join(ROOT, "tests", "graph_loss_host.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def grid():
    """[(loss number, c, s)]"""
    mp.mp.dps = 50
    out = []
    for c in SCALES:
        c2 = float(mp.mpf(c) * mp.mpf(c))                      # the double nearest to c^2 (1e300 at c = 1e150; no overflow on the way)
        ss = [0.0, 1e-300, c2 * (1.0 - 1e-15), c2 * (1.0 + 1e-15), c2] + [10.0 ** k for k in range(-8, 13)] + [1e300]
        assert all(np.isfinite(ss))
        for s in ss:
            for l in range(4):
                out.append((l, c, float(s)))
    return out


def exact(loss, c, s):
    """(rho, w) of the table of include/liodom_hip.h in 50 digits, c and s the doubles themselves."""
    mp.mp.dps = 50
    c, s = mp.mpf(c), mp.mpf(s)
    name = LOSSES[loss]
    if name == "none" or s <= 0:
        return s, mp.mpf(1)
    if name == "huber":
        return (s, mp.mpf(1)) if s <= c * c else (2 * c * mp.sqrt(s) - c * c, c / mp.sqrt(s))
    if name == "cauchy":
        return c * c * mp.log1p(s / (c * c)), 1 / (1 + s / (c * c))
    return s * c * c / (c * c + s), (c * c / (c * c + s)) ** 2


def run(exe, cases):
    text = "".join("%d %s %s\n" % (l, float(c).hex(), float(s).hex()) for l, c, s in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [line.split() for line in r.stdout.strip().split("\n")]
    assert len(rows) == len(cases)
    return [(float.fromhex(a), float.fromhex(b)) for a, b in rows]


def test_rho_and_w_on_the_grid_against_fifty_digits(exe):
    cases = grid()
    got = run(exe, cases)
    worst = {}
    for (l, c, s), (rho, w) in zip(cases, got):
        name = LOSSES[l]
        assert not np.isnan(rho) and not np.isnan(w), (name, c, s)
        assert 0.0 <= w <= 1.0 and rho <= s and rho >= 0.0, (name, c, s, rho, w)
        er, ew = exact(l, c, s)
        for which, value, ref, units in (("rho", rho, er, BOUND_U[name][0]), ("w", w, ew, BOUND_U[name][1])):
            err = float(abs(mp.mpf(value) - ref))
            bound = units * U * float(abs(ref)) + TINY
            if units == 0:
                assert err == 0.0, (name, which, c, s, value)
                continue
            share = err / bound
            key = (name, which)
            if share > worst.get(key, (0.0,))[0]:
                worst[key] = (share, c, s)
            assert err <= bound, (name, which, c, s, value, float(ref), share)
    for key in sorted(worst):
        print("%s %s: %.2f of the bound of %d u used, at c = %g, s = %g" % (key[0], key[1], worst[key][0], BOUND_U[key[0]][0 if key[1] == "rho" else 1], worst[key][1], worst[key][2]))


def test_out_of_table_inputs_are_quadratic(exe):
    """An unknown loss, the code of an inactive edge (-1), and s <= 0 (an indefinite Omega): rho = s, w = 1."""
    cases = [(4, 1.0, 7.0), (-1, 1.0, 7.0), (99, 2.0, 1e9), (1, 1.0, -3.0), (2, 1.0, -3.0), (3, 1.0, -3.0), (3, 1.0, 0.0)]
    for (l, c, s), (rho, w) in zip(cases, run(exe, cases)):
        assert rho == s and w == 1.0, (l, c, s, rho, w)
