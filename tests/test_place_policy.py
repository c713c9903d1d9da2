"""The key-frame policy of a place database (liodom_amd/csrc/place_policy.h) in a program of its own (tests/place_policy_main.cc),
built plain and under ASan + UBSan and run as a program: the first pose, distance and rotation thresholds that are exactly met, a
pose measured from the last KEY FRAME (not the last pose), poses that are no poses.  The Python restatement (api.PlacePolicy) is
held equal on random walks.  No GPU, nothing sanitized is loaded into Python."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the policy program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("place_policy") / ("policy_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "place_policy_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def pose(x=0.0, y=0.0, z=0.0, yaw=0.0):
    return (0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0), x, y, z)


def _run(exe, min_dist, min_yaw, poses):
    args = [exe, "%.17g" % min_dist, "%.17g" % min_yaw if math.isfinite(min_yaw) else "inf"] + ["%.17g" % v if math.isfinite(v) else repr(float(v)) for p in poses for v in p]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [int(v) for v in r.stdout.split()]
    assert len(out) == len(poses)
    return out


def test_the_first_pose_and_the_distance_threshold(exe):
    inf = float("inf")
    assert _run(exe, 2.0, inf, [pose(), pose(1.0), pose(1.9), pose(2.0), pose(2.5), pose(4.0)]) == [1, 0, 0, 1, 0, 1]      # exactly met counts
    assert _run(exe, 5.0, inf, [pose(1, 2, 3), pose(4, 6, 3), pose(4, 6, 3.0001)]) == [1, 1, 0]                          # 3-4-5
    assert _run(exe, 0.0, inf, [pose()] * 3) == [1, 1, 1]
    # measured from the last key frame, not from the last pose: steps of 0.6 against 1.0
    assert _run(exe, 1.0, inf, [pose(0.6 * i) for i in range(6)]) == [1, 0, 1, 0, 1, 0]


def test_the_rotation_threshold(exe):
    assert _run(exe, 100.0, 0.5, [pose(), pose(yaw=0.3), pose(yaw=0.49), pose(yaw=0.51), pose(yaw=0.8), pose(yaw=1.2)]) == [1, 0, 0, 1, 0, 1]
    assert _run(exe, 100.0, 0.5, [pose(yaw=3.0), pose(yaw=-3.0)]) == [1, 0]              # 0.283 rad apart across +-pi
    q = pose(yaw=0.2)
    assert _run(exe, 100.0, 0.5, [q, tuple(-v for v in q[:4]) + q[4:], tuple(3 * v for v in q[:4]) + q[4:]]) == [1, 0, 0]      # -q and 3 q are the same rotation
    assert _run(exe, 100.0, float("inf"), [pose(), pose(yaw=3.0)]) == [1, 0]             # infinity switches the angle off
    assert _run(exe, 100.0, 0.0, [pose(), pose()]) == [1, 1]


def test_poses_that_are_none_change_nothing(exe):
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, inf, 0, 0), (0, 0, 0, 1, 0, 0, -inf), (0, 0, 0, 0, 9, 9, 9)]
    assert _run(exe, 1.0, inf, bad) == [0, 0, 0, 0]
    assert _run(exe, 1.0, inf, bad + [pose(9, 9, 9)]) == [0, 0, 0, 0, 1]                 # the first finite pose is the first key frame
    assert _run(exe, 1.0, inf, [pose()] + bad + [pose(0.5), pose(1.0)]) == [1, 0, 0, 0, 0, 0, 1]


def test_the_python_restatement_answers_the_same(exe):
    rng = np.random.default_rng(8)
    for min_dist, min_yaw in ((1.0, float("inf")), (2.5, 0.3), (0.7, 0.05), (1e9, 0.2)):
        poses, x, yaw = [], np.zeros(3), 0.0
        for _ in range(80):
            x = x + rng.normal(0, 0.5, 3)
            yaw += rng.normal(0, 0.08)
            p = pose(*x, yaw=yaw)
            if rng.random() < 0.05:
                p = p[:4] + (float("nan"),) + p[5:]
            poses.append(tuple(float(v) for v in p))
        twin = api.PlacePolicy(min_dist, min_yaw)
        mine = [1 if twin.feed(p) else 0 for p in poses]
        assert mine == _run(exe, min_dist, min_yaw, poses), (min_dist, min_yaw)
        assert 1 < sum(mine) < 80
