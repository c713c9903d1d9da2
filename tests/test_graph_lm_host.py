"""The Levenberg-Marquardt controller of liodom_graph_optimize (liodom_amd/csrc/graph_lm.h) in a program of its own
(tests/graph_lm_main.cc), built plain and under ASan + UBSan and run as a program.  The program is played a script of the device's
answers — a solve's flag, iterations and max |g|, or a candidate's cost — and prints every solve it asks for (iterations, lambda),
every verdict and the final report.  What it must print comes from _restate below — the rules of include/liodom_hip.h and DESIGN.md
"Host side" written down once more in Python — and, for the designed graphs, from graph_model.lm, never from the C++; lambda and the
costs are compared bit for bit: both sides do the same double operations.  No GPU, nothing sanitized is loaded into Python."""
import itertools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}

CONVERGED, MAX_ITER, BREAKDOWN, GRADIENT_EXIT = 0, 1, 2, 3                        # GRAPH_PCG_*
TERM = dict(gradient=0, cost=1, max_iterations=2, lambda_=3, breakdown=4)       # LIODOM_GRAPH_TERM_*
DEFAULTS = (20, 0, 1e-8, 1e-9, 1e-10)          # max_iterations, max_pcg_iterations, pcg_, gradient_, cost_tolerance


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("graph_lm") / ("lm_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "graph_lm_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _run(exe, *args, script=""):
    r = subprocess.run([exe] + [a.hex() if isinstance(a, float) else str(a) for a in args], input=script, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _restate(opt, initial, n_free, n_active, answers):
    """The rules, from the documents -> (what the controller does, its report, the answers it used up).  answers: an iterable of
    ("p", flag, iterations, gmax) and ("c", candidate cost[, cost after linearising there])."""
    max_iterations, max_pcg, _, _, cost_tolerance = opt
    cap = max_pcg if max_pcg > 0 else min(6 * n_free, 65536)
    rep = dict(initial_cost=initial, final_cost=initial, max_gradient=0.0, final_lambda=1e-4, iterations=0, accepted_steps=0, pcg_iterations=0,
               termination=TERM["gradient"])
    does, used = [], []
    if n_free == 0 or n_active == 0:
        return does, rep, used
    answers = iter(answers)

    def answer(kind):
        a = next(answers)
        assert a[0] == kind, (a, kind)
        used.append(a)
        return a[1:]
    lam, cost, pending = 1e-4, initial, None
    while True:
        reporting = pending is not None or rep["iterations"] >= max_iterations          # that launch solves nothing
        does.append(("pcg", 0 if reporting else cap, lam))
        flag, its, rep["max_gradient"] = answer("p")
        if pending is not None:
            rep["termination"] = pending
        elif flag == GRADIENT_EXIT:
            rep["termination"] = TERM["gradient"]
        elif rep["iterations"] >= max_iterations:
            rep["termination"] = TERM["max_iterations"]
        elif flag == BREAKDOWN:
            rep["pcg_iterations"] += its
            rep["termination"] = TERM["breakdown"]
        else:
            rep["pcg_iterations"] += its
            rep["iterations"] += 1
            does.append("try")
            cand = answer("c")
            if cand[0] < cost:
                decrease = (cost - cand[0]) / abs(cost) if cost != 0.0 else 0.0
                lam = max(lam / 10.0, 1e-12)
                cost = cand[-1]
                rep["accepted_steps"] += 1
                rep["final_lambda"], rep["final_cost"] = lam, cost
                if decrease <= cost_tolerance:
                    pending = TERM["cost"]
                does.append("accepted")
                continue
            lam = lam * 10.0
            rep["final_lambda"] = lam
            if lam > 1e12:
                rep["termination"] = TERM["lambda_"]
                does.append("done")
                return does, rep, used
            does.append("rejected")
            continue
        does.append("done")
        return does, rep, used


def _same(a, b):
    """bit for bit, a NaN equal to a NaN"""
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def _play(exe, opt, initial, n_free, n_active, answers):
    """Restates, plays the answers the restatement used up to the program, compares every line -> (does, report)."""
    does, rep, used = _restate(opt, initial, n_free, n_active, answers)
    script = "".join(" ".join(v.hex() if isinstance(v, float) else str(v) for v in a) + "\n" for a in used)
    lines = _run(exe, "run", *opt, float(initial), n_free, n_active, script=script).split("\n")
    assert lines[-1] == "" and lines[-2].startswith("report "), lines
    got = lines[-2].split()[1:]
    for k, name in enumerate(("initial_cost", "final_cost", "max_gradient", "final_lambda")):
        assert _same(float.fromhex(got[k]), rep[name]), (name, got[k], rep[name])
    assert [int(v) for v in got[4:]] == [rep["iterations"], rep["accepted_steps"], rep["pcg_iterations"], rep["termination"]], (got, rep)
    assert len(lines) - 2 == len(does), (lines, does)
    for line, want in zip(lines, does):
        if isinstance(want, tuple):
            word, its, lam = line.split()
            assert word == "pcg" and int(its) == want[1] and _same(float.fromhex(lam), want[2]), (line, want)
        else:
            assert line == want
    return does, rep


def test_defaults_refusals_and_the_cap(exe):
    assert any(p.endswith(os.sep + "graph_lm.h") for p in gm.api._SRC)          # a change to it rebuilds the library
    got = _run(exe, "defaults").split()
    assert (int(got[0]), int(got[1])) + tuple(float.fromhex(v) for v in got[2:]) == DEFAULTS
    assert _run(exe, "refusal", *DEFAULTS).strip() == "ok"
    assert _run(exe, "refusal", 0, 0, 0.0, 0.0, 0.0).strip() == "ok"
    assert _run(exe, "refusal", 2 ** 31 - 1, 2 ** 31 - 1, math.inf, math.inf, math.inf).strip() == "ok"
    for k in range(5):
        for bad in ((-1,) if k < 2 else (-1e-300, -math.inf, math.nan)):
            opt = list(DEFAULTS)
            opt[k] = bad
            assert _run(exe, "refusal", *opt).strip() == "refused", opt
            assert _run(exe, "run", *opt, 1.0, 1, 1).strip() == "refused", opt
    for max_pcg, n_free, want in ((0, 0, 0), (0, 1, 6), (0, 10922, 65532), (0, 10923, 65536), (0, 65536, 65536), (0, 2 ** 31 - 1, 65536), (7, 1000, 7),
                                  (100000, 1, 100000)):
        assert int(_run(exe, "cap", max_pcg, n_free)) == want


def test_nothing_free_or_nothing_active_returns_at_once(exe):
    for n_free, n_active in ((0, 5), (3, 0), (0, 0)):
        does, rep = _play(exe, DEFAULTS, 12.5, n_free, n_active, [])
        assert does == [] and rep["initial_cost"] == rep["final_cost"] == 12.5 and rep["termination"] == TERM["gradient"]
        assert rep["final_lambda"] == 1e-4 and rep["iterations"] == 0


def test_gradient_exit_on_the_first_launch(exe):
    does, rep = _play(exe, DEFAULTS, 3.0, 4, 5, [("p", GRADIENT_EXIT, 0, 1e-12)])
    assert does == [("pcg", 24, 1e-4), "done"] and rep["termination"] == TERM["gradient"] and rep["max_gradient"] == 1e-12 and rep["iterations"] == 0
    does, rep = _play(exe, (20, 9, 1e-8, 1e-9, 1e-10), 3.0, 4, 5, [("p", GRADIENT_EXIT, 0, 0.0)])
    assert does[0] == ("pcg", 9, 1e-4)


def test_max_iterations_0_and_1(exe):
    opt = (0,) + DEFAULTS[1:]
    does, rep = _play(exe, opt, 3.0, 4, 5, [("p", MAX_ITER, 0, 0.5)])
    assert does == [("pcg", 0, 1e-4), "done"] and rep["termination"] == TERM["max_iterations"] and rep["max_gradient"] == 0.5
    does, rep = _play(exe, opt, 3.0, 4, 5, [("p", GRADIENT_EXIT, 0, 0.0)])          # the gradient is asked first
    assert rep["termination"] == TERM["gradient"]
    opt = (1,) + DEFAULTS[1:]
    does, rep = _play(exe, opt, 3.0, 4, 5, [("p", CONVERGED, 5, 0.5), ("c", 2.0), ("p", MAX_ITER, 0, 0.25)])
    assert [d[1] for d in does if isinstance(d, tuple)] == [24, 0]                   # the second launch solves nothing
    assert rep["termination"] == TERM["max_iterations"] and rep["iterations"] == 1 and rep["pcg_iterations"] == 5 and rep["max_gradient"] == 0.25
    does, rep = _play(exe, opt, 3.0, 4, 5, [("p", CONVERGED, 5, 0.5), ("c", 4.0), ("p", MAX_ITER, 0, 0.5)])          # ... after a rejected one too
    assert does[-2] == ("pcg", 0, 1e-3) and rep["termination"] == TERM["max_iterations"] and rep["accepted_steps"] == 0


def test_breakdown_counts_the_broken_solve(exe):
    does, rep = _play(exe, DEFAULTS, 3.0, 4, 5, [("p", BREAKDOWN, 3, 0.5)])
    assert rep["termination"] == TERM["breakdown"] and rep["pcg_iterations"] == 3 and rep["iterations"] == 0 and rep["final_cost"] == 3.0
    does, rep = _play(exe, DEFAULTS, 3.0, 4, 5, [("p", CONVERGED, 4, 0.5), ("c", 2.0), ("p", BREAKDOWN, 6, 0.25)])
    assert rep["termination"] == TERM["breakdown"] and rep["pcg_iterations"] == 10 and rep["iterations"] == 1 and rep["accepted_steps"] == 1
    assert rep["final_cost"] == 2.0 and rep["final_lambda"] == 1e-4 / 10.0


def test_every_step_rejected_until_lambda(exe):
    does, rep = _play(exe, (1000,) + DEFAULTS[1:], 3.0, 4, 5, itertools.cycle([("p", MAX_ITER, 24, 0.5), ("c", 3.0)]))          # equal is not lower
    assert rep["termination"] == TERM["lambda_"] and rep["accepted_steps"] == 0 and rep["final_lambda"] > 1e12 and rep["final_cost"] == 3.0
    assert rep["iterations"] == does.count("rejected") + 1 and rep["pcg_iterations"] == 24 * rep["iterations"] and does[-1] == "done"
    lam, n = 1e-4, 0
    while lam <= 1e12:
        lam, n = lam * 10.0, n + 1
    assert rep["iterations"] == n and rep["final_lambda"] == lam


def test_candidates_that_are_not_lower_are_rejected(exe):
    for initial, cand in ((3.0, math.nan), (0.0, 0.0), (0.0, math.nan), (-1.0, -1.0), (3.0, math.inf)):
        does, rep = _play(exe, DEFAULTS, initial, 4, 5, [("p", CONVERGED, 1, 0.5), ("c", cand), ("p", GRADIENT_EXIT, 0, 0.0)])
        assert does[2] == "rejected" and does[3] == ("pcg", 24, 1e-4 * 10.0) and rep["final_cost"] == initial and rep["accepted_steps"] == 0


def test_a_negative_cost_and_a_cost_of_zero(exe):
    does, rep = _play(exe, DEFAULTS, -1.0, 4, 5, [("p", CONVERGED, 1, 0.5), ("c", -2.0), ("p", GRADIENT_EXIT, 0, 0.0)])
    assert does[2] == "accepted" and does[3][1] == 24 and rep["final_cost"] == -2.0 and rep["termination"] == TERM["gradient"]          # a decrease of 1: no COST
    does, rep = _play(exe, DEFAULTS, -1.0, 4, 5, [("p", CONVERGED, 1, 0.5), ("c", -1.0 - 2.0 ** -40), ("p", MAX_ITER, 0, 0.125)])
    assert does[2] == "accepted" and does[3][1] == 0 and rep["termination"] == TERM["cost"]
    does, rep = _play(exe, DEFAULTS, 0.0, 4, 5, [("p", CONVERGED, 1, 0.5), ("c", -1.0), ("p", MAX_ITER, 0, 0.125)])          # from 0 the decrease counts as 0
    assert does[2] == "accepted" and rep["termination"] == TERM["cost"] and rep["final_cost"] == -1.0


def test_a_decrease_of_exactly_cost_tolerance_ends_with_cost(exe):
    opt = DEFAULTS[:4] + (0.25,)
    does, rep = _play(exe, opt, 1.0, 4, 5, [("p", CONVERGED, 2, 0.5), ("c", 0.75), ("p", MAX_ITER, 0, 0.125)])
    assert does == [("pcg", 24, 1e-4), "try", "accepted", ("pcg", 0, 1e-4 / 10.0), "done"]
    assert rep["termination"] == TERM["cost"] and rep["max_gradient"] == 0.125 and rep["final_cost"] == 0.75 and rep["pcg_iterations"] == 2
    does, rep = _play(exe, opt, 1.0, 4, 5, [("p", CONVERGED, 2, 0.5), ("c", 0.75 - 2.0 ** -53), ("p", GRADIENT_EXIT, 0, 0.0)])          # one ulp more: goes on
    assert does[3][1] == 24 and rep["termination"] == TERM["gradient"]
    # the cost kept is the one found by linearising at the accepted poses
    answers = [("p", CONVERGED, 2, 0.5), ("c", 0.5, 0.625), ("p", CONVERGED, 2, 0.5), ("c", 0.5625), ("p", CONVERGED, 2, 0.5), ("c", 0.5625), ("p", GRADIENT_EXIT, 0, 0.0)]
    does, rep = _play(exe, DEFAULTS, 1.0, 4, 5, answers)
    assert [d for d in does if isinstance(d, str) and d != "try"] == ["accepted", "accepted", "rejected", "done"] and rep["final_cost"] == 0.5625


def test_lambda_stops_at_its_floor(exe):
    answers = []
    for k in range(13):
        answers += [("p", CONVERGED, 1, 0.5), ("c", 2.0 ** -(k + 1))]
    does, rep = _play(exe, DEFAULTS, 1.0, 4, 5, answers + [("p", GRADIENT_EXIT, 0, 0.0)])
    assert rep["accepted_steps"] == 13 and rep["final_lambda"] == 1e-12 and rep["termination"] == TERM["gradient"]
    lams = [d[2] for d in does if isinstance(d, tuple)]
    assert len(lams) == 14 and all(b < a for a, b in zip(lams[:8], lams[1:9])) and min(lams) == 1e-12 and lams[-4:] == [1e-12] * 4


def _designed():
    hubs = []
    for side in (0, 1):
        poses, fixed, edges = gm.hub(3, side, seed=5)
        fixed[0] = 1
        hubs.append(("hub(3, %d)" % side, poses, fixed, edges, {}))
    ring = gm.drifted_ring(8, 1)[1:]
    return [("chain(4)",) + gm.chain(4) + ({},), ("drifted_ring(8, 1)",) + ring + ({},), ("drifted_ring(8, 1), 2 steps",) + ring + (dict(max_iterations=2),),
            ("chain(4), cost_tolerance 0.5",) + gm.chain(4) + (dict(cost_tolerance=0.5),)] + hubs


@pytest.fixture(scope="module")
def designed():
    """[(name, options, model's report, its trace, free nodes, edges)]: graph_model.lm once per graph"""
    out = []
    for name, poses, fixed, edges, kw in _designed():
        trace = []
        _, rep = gm.lm(poses, fixed, edges, trace=trace, **kw)
        opt = (kw.get("max_iterations", 20), 0, 1e-8, 1e-9, kw.get("cost_tolerance", 1e-10))
        out.append((name, opt, rep, trace, int(np.sum(np.asarray(fixed) == 0)), len(edges)))
    return out


def test_traces_of_designed_graphs_give_the_models_report(exe, designed):
    seen = set()
    for name, opt, want, trace, n_free, n_edges in designed:
        answers = []
        for k, (what, value) in enumerate(trace):
            if what == "cost":
                answers.append(("c", value))
            else:                                    # what the device would say of that gradient; a solve that runs takes 7 iterations
                solved = k + 1 < len(trace) and trace[k + 1][0] == "cost"
                flag = CONVERGED if solved else GRADIENT_EXIT if value <= opt[3] else BREAKDOWN if want["termination"] == "breakdown" else MAX_ITER
                answers.append(("p", flag, 7 if solved else 0, value))
        does, rep = _play(exe, opt, want["initial_cost"], n_free, n_edges, answers)
        assert len(answers) == len([d for d in does if isinstance(d, tuple) or d == "try"]), name          # every answer was asked for
        for key in ("iterations", "accepted_steps"):
            assert rep[key] == want[key], (name, key)
        for key in ("final_lambda", "final_cost", "max_gradient", "initial_cost"):
            assert _same(rep[key], want[key]), (name, key, rep[key], want[key])
        assert rep["termination"] == TERM[want["termination"].replace("lambda", "lambda_")], (name, want["termination"])
        assert rep["pcg_iterations"] == 7 * want["iterations"]
        seen.add(want["termination"])
    assert {"gradient", "max_iterations", "cost"} <= seen, seen
