"""The candidate grid of liodom_map_search_pose (liodom_amd/csrc/reloc_candidates.h) in a program of its own, built plain and under
host sanitizers, against the NumPy grid of tests/reloc_model.py: matrices and poses within 1e-12 (the two sides call different
cos / sin), the index order exactly, invalid and over-limit grids refused.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reloc_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}

ROLL_PITCH = [0.12, -0.07, 0.31, 0.94]                     # not normalised: |q| = 1.0002...
_n = np.array(ROLL_PITCH) / np.linalg.norm(ROLL_PITCH)
NEARLY = list(_n * (1.0 + 5e-7))                           # within 1e-6 of unit length
GRIDS = {
    "all half counts 0": dict(centre=[0, 0, 0, 1, 1.5, -2.5, 0.25], step_xy=0.4, step_z=0.4, step_yaw=0.02, nx=0, ny=0, nz=0, nyaw=0),
    "steps unused where the count is 0": dict(centre=[0, 0, 0, 1, 0, 0, 0], step_xy=-1.0, step_z=0.0, step_yaw=-3.0, nx=0, ny=0, nz=0, nyaw=0),
    "x only": dict(centre=[0, 0, 0.1, 0.99498743710662], step_xy=0.4, step_z=0.4, step_yaw=0.02, nx=3, ny=0, nz=0, nyaw=0, t=[3, 4, 5]),
    "yaw only": dict(centre=[0, 0, 0, 1, -7.25, 3.5, 1.0], step_xy=0.4, step_z=0.4, step_yaw=0.05, nx=0, ny=0, nz=0, nyaw=4),
    "nz > 0": dict(centre=[0, 0, 0, 1, 10, 20, 30], step_xy=0.4, step_z=0.25, step_yaw=0.02, nx=1, ny=2, nz=2, nyaw=1),
    "roll and pitch": dict(centre=list(_n) + [100.5, -50.25, 2.0], step_xy=0.1, step_z=0.4, step_yaw=0.005, nx=2, ny=2, nz=0, nyaw=2),
    "unnormalised within 1e-6": dict(centre=NEARLY + [1, 2, 3], step_xy=0.4, step_z=0.4, step_yaw=0.02, nx=1, ny=1, nz=1, nyaw=1),
}
REFUSED = {
    "radius 2": dict(centre=[0, 0, 0, 1, 0, 0, 0], radius=2),
    "negative count": dict(centre=[0, 0, 0, 1, 0, 0, 0], ny=-1),
    "zero xy step": dict(centre=[0, 0, 0, 1, 0, 0, 0], step_xy=0.0, ny=1),
    "negative z step": dict(centre=[0, 0, 0, 1, 0, 0, 0], step_z=-0.4, nz=1),
    "nan yaw step": dict(centre=[0, 0, 0, 1, 0, 0, 0], step_yaw=float("nan"), nyaw=1),
    "inf xy step": dict(centre=[0, 0, 0, 1, 0, 0, 0], step_xy=float("inf"), nx=1),
    "non-finite centre": dict(centre=[0, 0, 0, 1, float("inf"), 0, 0]),
    "nan quaternion": dict(centre=[float("nan"), 0, 0, 1, 0, 0, 0]),
    "quaternion off by 1e-5": dict(centre=[0, 0, 0, 1.00001, 0, 0, 0]),
    "zero quaternion": dict(centre=[0, 0, 0, 0, 0, 0, 0]),
    "2^20 + 1 candidates": dict(centre=[0, 0, 0, 1, 0, 0, 0], nx=1 << 19),
    "over the limit by product": dict(centre=[0, 0, 0, 1, 0, 0, 0], nx=50, ny=50, nyaw=60),
    "one huge count": dict(centre=[0, 0, 0, 1, 0, 0, 0], nz=2147483647),
}


def _argv(g):
    c = list(g["centre"]) + list(g.get("t", []))
    return ["%.17g" % v for v in c + [g.get("step_xy", 0.4), g.get("step_z", 0.4), g.get("step_yaw", 0.02)]] + \
           [str(g.get(k, 0)) for k in ("nx", "ny", "nz", "nyaw")] + [str(g.get("radius", 1))]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("reloc") / ("candidates_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "reloc_candidates_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_against_the_model(exe, name):
    g = GRIDS[name]
    r = subprocess.run([exe] + _argv(g), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    centre = list(g["centre"]) + list(g.get("t", []))
    T, poses, idx = rm.candidate_grid(centre, **{k: v for k, v in g.items() if k not in ("centre", "t")})
    assert lines[0] == "n %d" % T.shape[0]
    got = np.array([[float(v) for v in ln.split()] for ln in lines[1:] if ln])
    assert got.shape == (T.shape[0], 5 + 12 + 7)
    assert np.array_equal(got[:, 0], np.arange(T.shape[0])) and np.array_equal(got[:, 1:5].astype(np.int64), idx)      # the order: exact
    assert np.abs(got[:, 5:17] - T).max() <= 1e-12 and np.abs(got[:, 17:] - poses).max() <= 1e-12
    assert np.abs(np.linalg.norm(got[:, 17:21], axis=1) - 1.0).max() <= 1e-15
    # what the grid means: the candidate's rotation is Rz(ia step_yaw) R_c, its pose's quaternion gives the same rotation
    Rc = rm.rot_of_quat(centre[:4])
    for row, (ix, iy, ia, iz) in zip(got, idx):
        a = ia * g["step_yaw"] if ia else 0.0
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Tm = row[5:17].reshape(3, 4)
        assert np.abs(Tm[:, :3] - Rz @ Rc).max() <= 1e-12 and np.abs(rm.rot_of_quat(row[17:21]) - Tm[:, :3]).max() <= 1e-12
        assert np.array_equal(Tm[:, 3], row[21:24])


@pytest.mark.parametrize("name", list(REFUSED))
def test_invalid_and_over_limit_grids_are_refused(exe, name):
    r = subprocess.run([exe] + _argv(REFUSED[name]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and r.stdout.startswith("refused: ") and len(r.stdout.strip()) > len("refused:"), (r.returncode, r.stdout, r.stderr)


def test_the_largest_grid_is_taken(exe):
    g = dict(centre=[0, 0, 0, 1, 0, 0, 0], nx=(1 << 19) - 1)      # 2^20 - 1 candidates; only the last one is printed
    r = subprocess.run([exe] + _argv(g) + ["last"], capture_output=True, text=True, timeout=300)
    n = (1 << 20) - 1
    assert r.returncode == 0 and r.stdout.startswith("n %d\n%d %d 0 0 0 " % (n, n - 1, (1 << 19) - 1)), r.stdout[:200] + r.stderr
    assert abs(float(r.stdout.split()[2 + 5 + 3]) - 0.4 * ((1 << 19) - 1)) <= 1e-9
