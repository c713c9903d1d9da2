"""The round-based branch-and-bound driver (liodom_amd/csrc/reloc_bnb.h) in a program of its own (tests/reloc_bnb_main.cc), built
plain and under host sanitizers, on synthetic scores: the result is the exhaustive arg-max with ties to the lowest index whatever
the batch and however loose the bounds, every candidate is scored at most once, and the counters add up.  Also the level of a node
against the NumPy model's, and the candidate limit of the search.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import reloc_bnb_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("reloc_bnb") / ("bnb_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "reloc_bnb_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _search(exe, wx, wy, slabs, batch, kind, seed=1, slack=0):
    r = subprocess.run([exe, "search"] + [str(v) for v in (wx, wy, slabs, batch, kind, seed, slack)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want, best = r.stdout.strip().split("\n")
    w, b = want.split(), best.split()
    assert w[0] == "want" and b[0] == "best"
    out = dict(want=(int(w[1]), int(w[2])), best=int(b[1]), hits=(int(b[2]), int(b[3])), rounds=int(b[5]), bounded=int(b[7]), scored=int(b[9]),
               twice=int(b[11]), calls=(int(b[13]), int(b[14])), largest=(int(b[16]), int(b[17])))
    n = wx * wy * slabs
    assert out["best"] == out["want"][0] and sum(out["hits"]) == out["want"][1], out
    assert out["twice"] == 0 and 1 <= out["scored"] <= n and out["rounds"] >= 1
    assert out["calls"][0] <= out["rounds"] and out["calls"][1] <= out["rounds"] and out["rounds"] <= out["calls"][0] + out["calls"][1]
    assert out["largest"][0] <= 4 * batch and out["largest"][1] <= batch      # what the library sizes its buffers by
    return out


GRIDS = [(13, 7, 5), (9, 15, 5), (1, 1, 1), (1, 1, 7), (1, 9, 2), (16, 16, 1), (17, 16, 3), (3, 33, 2)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind", ["table", "equal", "last"])
def test_result_is_the_exhaustive_argmax(exe, grid, kind):
    for batch in (1, 3, 64, 65536):
        for slack in (0, 4):
            for seed in (1, 2):
                out = _search(exe, *grid, batch, kind, seed, slack)
                if kind == "equal":
                    # (roots are never bounded: in a grid of roots alone every candidate is scored)
                    assert out["best"] == 0 and (batch > 1 or slack > 0 or max(grid[:2]) == 1 or out["scored"] == 1)
                if kind == "last":
                    assert out["best"] == grid[0] * grid[1] * grid[2] - 1


def test_exact_bounds_and_one_node_a_round_score_one_path(exe):
    """All scores equal and exact bounds: after the first leaf nothing else can win, so one node a round walks one root-to-leaf path."""
    out = _search(exe, 13, 7, 1, 1, "equal")
    assert (out["scored"], out["rounds"], out["bounded"]) == (1, 5, 2 + 4 + 4 + 4)      # K = 4; the first split is clipped to 2 tiles


@pytest.mark.parametrize("batch", [1, 256, 4096])
def test_a_grid_above_the_exhaustive_limit(exe, batch):
    """1501 x 1401 x 3 = 6 308 703 candidates, a closed-form score with a plateau of equal maxima: few candidates are scored."""
    out = _search(exe, 1501, 1401, 3, batch, "closed", seed=5, slack=2)
    assert out["want"][1] == 1000 and out["scored"] < 20000 and out["bounded"] < 200000


def test_loose_bounds_cost_work_not_correctness(exe):
    tight = _search(exe, 200, 150, 2, 64, "closed", seed=3, slack=0)
    loose = _search(exe, 200, 150, 2, 64, "closed", seed=3, slack=40)
    assert loose["best"] == tight["best"] and loose["scored"] >= tight["scored"] and loose["bounded"] >= tight["bounded"]


@pytest.mark.parametrize("args", [(0.4, 0.4, 1), (0.4, 0.4, 0), (0.15, 0.4, 1), (1.0, 0.4, 0), (0.1, 0.05, 1), (25.0, 0.4, 1)])
def test_level_of_a_node_equals_the_models(exe, args):
    r = subprocess.run([exe, "levels"] + ["%.17g" % args[0], "%.17g" % args[1], str(args[2])], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in r.stdout.split()]
    assert got == [bm.level_of(1 << k, *args) for k in range(32)]
    assert min(got) >= 1 and max(got) <= bm.LEVEL_MAX and got == sorted(got)


def test_the_search_takes_grids_up_to_2_31_minus_1(exe):
    def count(*half):
        r = subprocess.run([exe, "count"] + [str(v) for v in half], capture_output=True, text=True, timeout=60)
        return r.returncode, r.stdout.strip()

    assert count(100, 100, 0, 78) == (0, "n 6342957 grid 201 201 157 8")
    assert count(100, 100, 0, 157) == (0, "n 12726315 grid 201 201 315 8")
    assert count((1 << 30) - 1, 0, 0, 0) == (0, "n 2147483647 grid 2147483647 1 1 31")
    assert count(0, 0, 0, (1 << 30) - 1) == (0, "n 2147483647 grid 1 1 2147483647 0")
    for half in ((1 << 30, 0, 0, 0), (0, 0, 2147483647, 0), (32768, 32768, 0, 0), (1000, 1000, 10, 100), (-1, 0, 0, 0)):
        rc, out = count(*half)
        assert rc == 3 and out.startswith("refused: ") and len(out) > len("refused: "), (half, out)
