"""The conditions of tests/designed_solves.py, proved on the oracle alone (CPU): every case gives its stated correspondence
counts and its pinned (termination, iterations, accepted) in both solves; the solves are reproduced by orc.lm_solve on blocks
rebuilt from the oracle's correspondences; every decision has margin (same trace from the reversed block order and from the
product's controller compiled for the host, tests/hostcheck.cc, to test_hostcheck's bars); Huber cases have their count of
residuals beyond 0.2 at the start, rank cases their condition number.  tests/test_gpu_designed_solve.py relies on all of it."""
import ctypes as C

import numpy as np
import pytest

import designed_solves as ds
from test_hostcheck import hc, _dp      # noqa: F401  (hc: the fixture that builds and binds tests/hostcheck.cc)

IDENT_Q, IDENT_T = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
RANK_COND = 1e8
_runs = {}


def run_of(orc, name):
    if name not in _runs:
        _runs[name] = ds.oracle_run(orc, ds.CASES[name])
    return _runs[name]


def hc_solve(hc, blocks, q, t, apply_on_ftol=0):
    b = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1, 9) if len(blocks) else np.zeros((1, 9))
    q, t = np.array(q, dtype=np.float64), np.array(t, dtype=np.float64)
    it, acc_n = C.c_int(), C.c_int()
    ic, fc = C.c_double(), C.c_double()
    term = hc.hc_lm_solve(_dp(b), len(blocks), _dp(q), _dp(t), 3.0, 75.0, apply_on_ftol, C.byref(it), C.byref(acc_n), C.byref(ic), C.byref(fc))
    return q, t, (term, it.value, acc_n.value), ic.value, fc.value


def test_every_listed_trace_has_its_case():
    assert set(ds.TRACES) == set(ds.CASES)
    want = {(1, 2, 1), (1, 1, 0), (1, 3, 2), (1, 4, 3), (2, 1, 0), (2, 2, 1), (2, 3, 2), (2, 4, 3), (3, 0, 0), (3, 1, 1), (3, 3, 3), (3, 4, 4),
            (0, 4, 4), (0, 4, 1), (0, 4, 2), (0, 4, 3), (4, 0, 0), (5, 0, 0)}
    assert set(ds.TRACE_SHOWN) == want
    for trace, (name, solve) in ds.TRACE_SHOWN.items():
        assert ds.TRACES[name][1 + solve] == trace, (trace, name)
    for k in (0, 1, 32, 64):
        assert ds.CASES["huber%d" % k].huber == k and ds.CASES["huber%d" % k].C == 64
    for n in ds.COUNTS:
        assert ds.CASES["c%d" % n].C == ds.CASES["c%d" % n].E == n
        if n < 1056:
            assert ds.CASES["s%d" % n].C == n and ds.CASES["s%d" % n].E == 1056


def test_the_designed_mask():
    """positions(): the named bits of the validity mask are set whenever C allows, on both shapes; build() is deterministic and
    puts exactly the valid edges near a segment."""
    for E, C_ in ((1056, 5), (1056, 6), (1056, 63), (1056, 513), (2100, 72)):
        pos = set(ds.positions(E, C_, 3).tolist())
        assert len(pos) == C_ and {E - 1, 0, 7, 3, E - 8}.issubset(pos)
        if C_ >= 6:
            assert E - 4 in pos
        if E > 2056:
            assert set(range(2048, 2056)).issubset(pos)
    assert ds.positions(1056, 1).tolist() == [1055] and ds.positions(1056, 2).tolist() == [0, 1055]
    assert ds.positions(64, 64).tolist() == list(range(64)) and len(ds.positions(64, 0)) == 0
    big = ds.CASES["big_sparse"]
    assert big.E > 2048 and ds.edge_capacity(big.shape) == 8704 and ds.edge_capacity(ds.SMALL) == 1056
    nb = (big.E + 7) // 8
    assert nb > 256 and (nb + 3) // 4 > 64          # more than 256 k_knn workgroups: a second round of 64 mask words
    for name in ("s5", "big_sparse", "c65", "t_nores"):
        a, b = ds.build(ds.CASES[name]), ds.build(ds.CASES[name])
        assert np.array_equal(a["edges"].view(np.uint32), b["edges"].view(np.uint32)) and np.array_equal(a["map"], b["map"])
        case = ds.CASES[name]
        world_pts = a["edges"][:, :3].astype(np.float64) @ a["R"].T + a["t"]
        d = np.sqrt(((world_pts[:, None, :] - a["centres"][None, :, :]) ** 2).sum(-1)).min(axis=1) if len(world_pts) else np.zeros(0)
        assert np.array_equal(d < 1.0, a["valid"]) and int(a["valid"].sum()) == case.C
        assert np.all(d[~a["valid"]] > 3.0 + 0.4)
        r = np.linalg.norm(a["map"][:, :3], axis=1)
        assert r.min() >= 6.0 and r.max() <= 60.0
        c = a["centres"]
        if len(c) > 1:
            dc = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)) + 1e9 * np.eye(len(c))
            assert dc.min() >= 4.0


@pytest.mark.parametrize("name", list(ds.CASES))
def test_case_on_the_oracle(orc, hc, name):
    case = ds.CASES[name]
    want_matches, want0, want1 = ds.TRACES[name]
    r = run_of(orc, name)
    info, edges = r["info"], r["built"]["edges"]
    # 1. counts and traces
    assert r["matches"] == want_matches and r["matches"][0] == case.C, (name, r["matches"])
    if name not in ("t_maxit_4_3", "t_maxit_4_2", "t_maxit_4_1"):
        assert r["matches"] == [case.C, case.C], name
    assert r["traces"] == [want0, want1], (name, r["traces"])
    assert [len(b) for b in r["blocks"]] == r["matches"]
    # 2. the odometer's solves are orc.lm_solve on the rebuilt blocks: trace, costs, and the pose (solve 0: through the float
    # queries of the second pass, which are the edges under that pose; solve 1: the returned pose)
    q0, t0, tr0 = orc.lm_solve(r["blocks"][0], IDENT_Q, IDENT_T)
    assert ds.trace_of(tr0) == want0 and tr0.initial_cost == info.lm[0].initial_cost and tr0.final_cost == info.lm[0].final_cost
    T0, _ = orc.pose_ops(q0, t0)
    if len(edges):
        assert np.array_equal(orc.transform(T0, edges)[:, :3].view(np.uint32), r["queries1"].view(np.uint32)), name
    q1, t1, tr1 = orc.lm_solve(r["blocks"][1], q0, t0)
    assert ds.trace_of(tr1) == want1 and tr1.initial_cost == info.lm[1].initial_cost and tr1.final_cost == info.lm[1].final_cost
    assert np.allclose(r["pose"][4:], t1, atol=1e-12) and min(np.abs(r["pose"][:4] - q1).max(), np.abs(r["pose"][:4] + q1).max()) <= 1e-12
    # 3. margin: reversed block order, and the product's controller on the host (test_lm_controller_matches_oracle's bars)
    for it, (bl, qs, ts, qo, to, tr) in enumerate(((r["blocks"][0], IDENT_Q, IDENT_T, q0, t0, tr0), (r["blocks"][1], q0, t0, q1, t1, tr1))):
        _, _, trr = orc.lm_solve(bl[::-1], qs, ts)
        assert ds.trace_of(trr) == ds.trace_of(tr), (name, it, "reversed order")
        qh, th, trh, ic, fc = hc_solve(hc, bl, qs, ts)
        assert trh == ds.trace_of(tr), (name, it, trh)
        if len(bl) == 0 or tr.termination == 5:
            continue
        if it == 0:
            assert abs(ic - tr.initial_cost) <= 1e-12 * tr.initial_cost, (name, ic, tr.initial_cost)
            assert abs(fc - tr.final_cost) <= 1e-9 * max(tr.final_cost, 1e-12), (name, fc, tr.final_cost)
        Hm, n_lin = ds.normal_matrix(orc, bl, qo, to)
        cond = np.linalg.cond(Hm)
        if cond <= RANK_COND:
            tol = 1e-9 if it == 0 else 1e-8
            assert np.allclose(qh, qo, atol=tol) and np.allclose(th, to, atol=tol), (name, it)
        # 5. rank: the flag of the case is the condition of the finalising solve's normal equations at its solution
        if it == 1:
            assert case.rank == bool(cond > RANK_COND), (name, cond)
    if case.group == "rank" and not case.dup:
        assert case.rank
    if case.dup:
        assert want0[0] == 5 and want1[0] == 5
    # 4. Huber: the number of residuals in the linear branch at the start pose
    if case.huber is not None:
        _, n_lin = ds.normal_matrix(orc, r["blocks"][0], IDENT_Q, IDENT_T)
        assert n_lin == case.huber, (name, n_lin)


def test_stale_sequence_on_the_oracle(orc):
    """The static sequence of the GPU's stale-state test: every scan matches exactly its C edges in both passes, and the pose
    stays within 5 cm and 2 mrad of the identity (scans of 5, 0 and 1 edges barely hold it; the gate is 1 m), so the next scan
    meets the same world."""
    steps = ds.stale_steps()
    od = orc.Odometer(ds.oracle_params(orc, ds.CASES["c1056"]))
    for f in steps[0]["frames"]:
        od.step(f)
    assert len(steps[0]["frames"]) + len(steps) <= ds.PREV_FRAMES          # nothing is evicted
    for k, b in enumerate(steps):
        assert int(b["valid"].sum()) == ds.STALE_COUNTS[k] and len(b["edges"]) == (ds.STALE_COUNTS[k] or 64)
        pose, info = od.step(b["edges"])
        assert list(info.matches) == [ds.STALE_COUNTS[k]] * 2, (k, list(info.matches))
        for it in (0, 1):
            v, _, _ = od.last_corr(it)
            assert np.array_equal(v.astype(bool), b["valid"]), (k, it)
        assert np.abs(pose[4:]).max() < 0.05 and np.abs(pose[:3]).max() < 1e-3, (k, pose)
    od.close()
