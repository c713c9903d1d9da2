"""The "lost" policy (liodom_amd/csrc/track_policy.h) in a program of its own (tests/track_policy_main.cc), built plain and under
ASan + UBSan and run as a program: lost_after 1 and 3, a streak broken by one scan above, n_edges = 0, records that are not valid,
the reset after LOST, and a fraction exactly equal to min_fraction (tracking).  The Python restatement (api.TrackPolicy) is held equal
on random sequences.  No GPU, nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}
V, NV = api.HIT_VALID, 0
N = 100
BELOW, ABOVE = (40, 19, N, V), (60, 45, N, V)      # fractions 0.295 and 0.525 against min_fraction 0.5


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the policy program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("track_policy") / ("policy_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "track_policy_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _run(exe, min_fraction, lost_after, records):
    """[(answer, streak)] per record: 0 tracking / 1 lost."""
    args = [exe, "%.17g" % min_fraction, str(lost_after)] + [str(int(v)) for rec in records for v in rec]
    r = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.strip().split("\n")] if records else []
    assert len(out) == len(records)
    return out


def _answers(exe, min_fraction, lost_after, records):
    return [a for a, _ in _run(exe, min_fraction, lost_after, records)]


def test_lost_after_one(exe):
    assert _answers(exe, 0.5, 1, [ABOVE, BELOW, ABOVE, BELOW, BELOW]) == [0, 1, 0, 1, 1]
    assert _answers(exe, 0.5, 0, [BELOW]) == [1] and _answers(exe, 0.5, -3, [BELOW]) == [1]      # (below 1 counts as 1)


def test_lost_after_three(exe):
    assert _run(exe, 0.5, 3, [ABOVE, BELOW, BELOW, BELOW]) == [(0, 0), (0, 1), (0, 2), (1, 0)]


def test_a_streak_broken_by_one_scan_above(exe):
    assert _answers(exe, 0.5, 3, [BELOW, BELOW, ABOVE, BELOW, BELOW, BELOW]) == [0, 0, 0, 0, 0, 1]


def test_no_edges_counts_as_below(exe):
    none = (0, 0, 0, V)
    assert _answers(exe, 0.5, 2, [none, none]) == [0, 1]
    assert _answers(exe, 0.0, 1, [none]) == [1]                 # whatever the threshold
    assert _answers(exe, 0.5, 2, [BELOW, none]) == [0, 1]       # and it continues a streak


def test_records_that_are_not_valid_change_nothing(exe):
    no_reader = (0, 0, 0, api.HIT_NO_READER)
    unsolved_only = (0, 0, N, api.HIT_NO_SOLVE)
    got = _run(exe, 0.5, 2, [BELOW, no_reader, unsolved_only, (0, 0, N, NV), BELOW])
    assert got == [(0, 1), (0, 1), (0, 1), (0, 1), (1, 0)]      # neither counted nor a break
    assert _answers(exe, 0.5, 1, [(0, 0, 0, NV)] * 3) == [0, 0, 0]
    assert _answers(exe, 0.5, 1, [(0, 0, N, V | api.HIT_NO_SOLVE)]) == [1]      # NO_SOLVE beside VALID is a valid record


def test_the_state_starts_over_after_lost(exe):
    assert _run(exe, 0.5, 2, [BELOW] * 5) == [(0, 1), (1, 0), (0, 1), (1, 0), (0, 1)]


def test_a_fraction_equal_to_the_threshold_is_tracking(exe):
    # (hits_r + hits_0) / (2 n) with exactly representable results: 0.5, 0.25, 0.75
    for frac, rec in ((0.5, (60, 40, 100, V)), (0.25, (3, 1, 8, V)), (0.75, (2, 1, 2, V))):
        assert _answers(exe, frac, 1, [rec, rec]) == [0, 0], frac
        under = (rec[0], rec[1] - 1, rec[2], V)
        assert _answers(exe, frac, 1, [under]) == [1], frac
    # ... and with the threshold computed as the program computes the fraction: 74 hits of the 222 an edge cloud of 111 can give
    rec = (41, 33, 111, V)
    assert _answers(exe, (41.0 + 33.0) / (2.0 * 111.0), 1, [rec]) == [0]


def test_the_python_restatement_answers_the_same(exe):
    rng = np.random.default_rng(5)
    for lost_after in (1, 2, 3, 5):
        for min_fraction in (0.3, 0.5, 41.0 / 64.0):
            recs = []
            for _ in range(60):
                n = int(rng.choice([0, 1, 64, 100]))
                hr = int(rng.integers(0, n + 1))
                h0 = int(rng.integers(0, hr + 1))
                recs.append((hr, h0, n, int(rng.choice([V, V, V, NV, api.HIT_NO_READER, V | api.HIT_NO_SOLVE]))))
            p = api.TrackPolicy(min_fraction, lost_after)
            mine = [(1 if p.feed(*r) == api.LOST else 0, p.below) for r in recs]
            assert mine == _run(exe, min_fraction, lost_after, recs), (lost_after, min_fraction)
            assert 1 in [a for a, _ in mine]
