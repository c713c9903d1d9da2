"""tests/register_model.py (liodom_map_register_poses on the CPU oracle's pieces), without a GPU:
  1. register_pass_converged of liodom_math.h, compiled for the host, gives the model's two norms and verdict;
  2. two passes are localize_model.seeded_first_scan: the same poses and correspondences;
  3. the convergence table the feature was designed on: scans 0 and 5 of the localising traversal from starts A and B reach, within
     10 passes at stops 1e-6 m / 1e-7, the pose the true start reaches (to the project's pose tolerance of 1e-4 m / 1e-4 rad: the
     three runs end in the same basin, not on the same bits), with the z error below 0.03 m; scan 10 from A runs out of passes;
  4. no pass of those cases moves by an amount within a factor 10 of either threshold, so the verdicts do not hang on rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import localize_model as lm
import register_model as rm
from mapper_lag_common import POSE_TOL_R, POSE_TOL_T, rot_angle

HERE = os.path.dirname(os.path.abspath(__file__))
TIGHT = dict(stop_translation=1e-6, stop_rotation=1e-7)
STARTS = dict(A=rm.START_A, B=rm.START_B)


@pytest.fixture(scope="module")
def leaf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("register") / "libregister_hostcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, os.path.join(HERE, "register_hostcheck.cc")])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.rh_pass_converged.restype = C.c_int
    L.rh_pass_converged.argtypes = [dp, dp, dp, dp, C.c_double, C.c_double, dp]

    def call(q0, t0, q1, t1, stop_t, stop_r):
        a = [np.ascontiguousarray(v, np.float64) for v in (q0, t0, q1, t1)]
        mv = np.zeros(2)
        ok = L.rh_pass_converged(*[v.ctypes.data_as(dp) for v in a], stop_t, stop_r, mv.ctypes.data_as(dp))
        return bool(ok), mv[0], mv[1]
    return call


def test_the_leaf_function_gives_the_models_norms(orc, synth, leaf):
    r = rm.site_case(orc, synth, 0, rm.START_A, **TIGHT)
    prev = rm.normalised(r["start"])
    for pose, (mt, mr) in zip(r["poses"], r["moves"]):
        ok, gt, gr = leaf(prev[:4], prev[4:], pose[:4], pose[4:], 1e-6, 1e-7)
        assert abs(gt - mt) <= 1e-15 and abs(gr - mr) <= 1e-15
        assert ok == (mt <= 1e-6 and mr <= 1e-7)
        # the sign of either quaternion does not matter, the thresholds are inclusive, a NaN never converges
        assert leaf(-prev[:4], prev[4:], pose[:4], pose[4:], 1e-6, 1e-7)[1:] == (gt, gr)
        assert leaf(prev[:4], prev[4:], pose[:4], pose[4:], gt, gr)[0]
        if gt > 0:
            assert not leaf(prev[:4], prev[4:], pose[:4], pose[4:], np.nextafter(gt, 0), gr)[0]
        prev = pose
    assert leaf(prev[:4], prev[4:], prev[:4], prev[4:], 0.0, 0.0) == (True, 0.0, 0.0)
    assert not leaf(prev[:4], prev[4:], prev[:4], prev[4:] * np.nan, 1.0, 1.0)[0]


@pytest.mark.parametrize("which", ["truth", "perturbed"])
def test_two_passes_are_the_seeded_first_scan(orc, synth, which):
    seed = lm.seeds(orc, synth)[which]
    first = lm.seeded_first_scan(orc, synth, seed)
    r = rm.register(orc, lm.site_map(orc, synth), first["edges"], seed, max_passes=2, stop_translation=0.0, stop_rotation=0.0)
    assert r["passes"] == 2 and r["termination"] == rm.MAX_PASSES
    assert np.array_equal(r["pose"], first["pose"])
    assert np.array_equal(r["local"].view(np.uint32), first["recv"].view(np.uint32))
    v, ia, ib = first["passes"][1]["corr"]      # (the seeded scan searches with the kd-tree, the model by brute force: same result)
    assert np.array_equal(r["corr"][:, 0], np.where(v != 0, ia, -1)) and np.array_equal(r["corr"][:, 1], np.where(v != 0, ib, -1))
    assert r["matches"] == first["passes"][1]["matches"]


@pytest.mark.parametrize("scan", [0, 5])
@pytest.mark.parametrize("start", ["A", "B"])
def test_starts_reach_the_pose_the_truth_reaches(orc, synth, scan, start):
    ref = rm.site_case(orc, synth, scan, None, **TIGHT)
    r = rm.site_case(orc, synth, scan, STARTS[start], **TIGHT)
    assert ref["termination"] == rm.CONVERGED and r["termination"] == rm.CONVERGED and r["passes"] <= 10
    dt, dr = np.linalg.norm(r["pose"][4:] - ref["pose"][4:]), rot_angle(r["pose"][:4], ref["pose"][:4])
    z0, z1 = abs(r["start"][6] - r["truth"][6]), abs(r["pose"][6] - r["truth"][6])
    print("scan %d from %s: %d passes, %.3e m / %.3e rad from the truth's fixed point, z error %.3f -> %.4f m" % (scan, start, r["passes"], dt, dr, z0, z1))
    assert dt <= POSE_TOL_T and dr <= POSE_TOL_R
    assert z0 >= 0.05 and z1 < 0.03
    assert r["last_move_t"] <= 1e-6 and r["last_move_r"] <= 1e-7 and r["matches"] == ref["matches"]


def test_scan_10_from_a_runs_out_of_passes(orc, synth):
    r = rm.site_case(orc, synth, 10, rm.START_A, **TIGHT)
    assert r["termination"] == rm.MAX_PASSES and r["passes"] == 10
    assert r["last_move_t"] > 1e-3      # the limit cycle: 2.5 mm at pass 10


def test_no_pass_moves_near_a_threshold(orc, synth):
    cases = [(0, None), (0, "A"), (0, "B"), (5, None), (5, "A"), (5, "B"), (10, "A")]
    for scan, start in cases:
        for mt, mr in rm.site_case(orc, synth, scan, STARTS.get(start), **TIGHT)["moves"]:
            assert not (1e-7 < mt < 1e-5) and not (1e-8 < mr < 1e-6), (scan, start, mt, mr)


def test_rows_that_end_early(orc, synth):
    _, edges, gt = lm.traversal(orc, synth, 1)[0]
    mo = lm.site_map(orc, synth)
    far = gt.copy()
    far[4:6] += 1000.0
    r = rm.register(orc, mo, edges, far)
    assert r["termination"] == rm.NO_MAP and r["local_points"] == 0 and r["passes"] == 0 and (r["corr"] == -1).all()
    r = rm.register(orc, mo, edges[:0], gt)
    assert r["termination"] == rm.FEW_MATCHES and r["passes"] == 0 and np.array_equal(r["pose"], rm.normalised(gt))
    r = rm.register(orc, mo, edges, gt, min_matches=10000)
    assert r["termination"] == rm.FEW_MATCHES and r["matches"] > 200 and np.isnan(r["information"]).all()
