"""LoopCloser(refine=...) (liodom_amd/loop.py) with the stubs of test_loop_closer.py and a stub register_poses: a refined loop
edge carries the registered Z, a registration that fails adds no edge, refine=None adds exactly the edge it adds today, and
loop_info="solve" is B^-T (H / sigma2) B^-1 with B held to a finite-difference Jacobian of tests/graph_model.py.  No GPU."""
import numpy as np
import pytest

import graph_model as gm
from liodom_amd import api, loop
from test_loop_closer import StubGraph, StubMap, StubPlaces, _cloud, _walk

OFFSET = gm.from_axis_angle((1.0, 2.0, -1.0), 0.02, (0.03, -0.02, 0.3))      # what the registration adds to a searched pose


def _spd(seed):
    a = np.random.default_rng(seed).normal(size=(6, 6))
    return a @ a.T + 6.0 * np.eye(6)


class RefiningMap(StubMap):
    """register_poses moves the searched pose by OFFSET (applied on the right) and ends as `termination` with `matches`."""

    def __init__(self, reach, termination=api.REG_CONVERGED, matches=40, flags=api.COV_VALID):
        super().__init__(reach)
        self.termination, self.matches, self.flags, self.registered, self.options = termination, matches, flags, [], None

    def register_poses(self, edges, poses, want_corr=False, **options):
        self.options = options
        out = []
        for p in np.asarray(poses, np.float64).reshape(-1, 7):
            taken = self.termination in (api.REG_CONVERGED, api.REG_MAX_PASSES)
            pose = gm.compose(p, OFFSET) if taken else p.copy()
            self.registered.append(pose)
            out.append(dict(pose=pose, termination=self.termination, matches=self.matches, passes=3, cov_flags=self.flags,
                            information=_spd(len(self.registered)), sigma2=0.004, n_residuals=self.matches))
        return out


def _run(mp, **kw):
    db, gr = StubPlaces(), StubGraph()
    lc = loop.LoopCloser(mp, db, [dict(step_xy=0.4)], graph=gr, min_dist=4.0, min_gap=5, k=3, min_fraction=0.5, **kw)
    loops = []
    for p in _walk():
        loops += lc.feed(p, _cloud(p[4:]))["loops"]
    return lc, gr, loops


def test_a_refined_edge_carries_the_registered_pose():
    mp = RefiningMap(3.0)
    lc, gr, loops = _run(mp, refine=dict(max_passes=7, stop_translation=1e-5, min_fraction=0.5))
    edges = [e for e in gr.edge_list if e["kind"] == 1]
    assert edges and len(edges) == len(loops) == len(lc.loops) == len(mp.registered)
    assert mp.options == dict(max_passes=7, stop_translation=1e-5)      # min_fraction is the LoopCloser's, the rest go to the map
    for e, l, reg in zip(edges, loops, mp.registered):
        i = int(e["i"])
        assert np.array_equal(l["pose"], reg) and np.max(np.abs(gm.compose(l["searched_pose"], OFFSET) - reg)) <= 1e-15
        assert np.max(np.abs(e["z"] - gm.between(gr.nodes[i], reg))) <= 1e-15
        assert abs(gm.compose(gr.nodes[i], e["z"])[6] - reg[6]) <= 1e-12 and abs(reg[6] - l["searched_pose"][6]) > 0.2      # z is measured now
        assert np.array_equal(e["info"], loop.LOOP_INFO) and l["registration"]["passes"] == 3


@pytest.mark.parametrize("termination, matches", [(api.REG_FEW_MATCHES, 3), (api.REG_NO_MAP, 0), (api.REG_EVAL_FAILURE, 40),
                                                  (api.REG_CONVERGED, 10), (api.REG_MAX_PASSES, 24)])
def test_a_failed_or_thin_registration_adds_no_edge(termination, matches):
    mp = RefiningMap(3.0, termination=termination, matches=matches)      # the clouds hold 50 edges: 24 / 50 < 0.5
    lc, gr, loops = _run(mp, refine=dict(min_fraction=0.5))
    assert mp.registered and loops == [] and lc.loops == [] and all(e["kind"] == 0 for e in gr.edge_list)


def test_max_passes_rows_with_enough_matches_are_kept():
    lc, gr, loops = _run(RefiningMap(3.0, termination=api.REG_MAX_PASSES, matches=25), refine=dict(min_fraction=0.5))
    assert loops and len(loops) == len([e for e in gr.edge_list if e["kind"] == 1])


def test_without_refine_every_path_is_as_before():
    plain_lc, plain_gr, plain = _run(StubMap(3.0))
    mp = RefiningMap(3.0)
    lc, gr, loops = _run(mp, refine=None)
    assert mp.registered == [] and len(gr.edge_list) == len(plain_gr.edge_list) and lc.loops == plain_lc.loops
    for a, b in zip(gr.edge_list, plain_gr.edge_list):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(loops, plain):
        assert sorted(a) == sorted(b) == ["fraction", "match", "node", "place", "pose"] and np.array_equal(a["pose"], b["pose"])
    with pytest.raises(ValueError):
        lc.refine_loop(_cloud((0, 0, 0)), plain_lc.key_poses[0], plain_lc.key_poses[0])
    with pytest.raises(ValueError):
        loop.LoopCloser(mp, StubPlaces(), [], graph=StubGraph(), loop_info="solve")
    with pytest.raises(ValueError):
        loop.LoopCloser(mp, StubPlaces(), [], graph=StubGraph(), loop_info="other", refine={})


def test_information_from_the_solve():
    mp = RefiningMap(3.0)
    lc, gr, loops = _run(mp, refine=dict(min_fraction=0.5), loop_info="solve")
    edges = [e for e in gr.edge_list if e["kind"] == 1]
    assert edges
    for n, (e, l) in enumerate(zip(edges, loops)):
        Xi, Xj, Z = gr.nodes[int(e["i"])], l["pose"], np.array(e["z"])
        H, s2 = l["registration"]["information"], l["registration"]["sigma2"]
        B = loop.edge_jacobian_j(Xi, Xj, Z)
        _, Bn = gm.numeric_jacobians(Xi, Xj, Z)
        assert np.max(np.abs(B - Bn)) <= 1e-6                                  # central differences with h = 1e-6 on entries of size 1
        assert np.max(np.abs(B - gm.edge_jacobians(Xi, Xj, Z)[2])) <= 1e-13
        Bi = np.linalg.inv(Bn)
        want = Bi.T @ (H / s2) @ Bi
        om = np.array(e["info"]).reshape(6, 6)
        assert np.max(np.abs(om - want)) <= 1e-5 * np.max(np.abs(want))
        assert np.array_equal(om, om.T) and np.linalg.eigvalsh(om).min() > 0     # symmetric; positive definite as H is
        # what it means: the edge's chi2 of a small move of node j is the registration's own
        d = 1e-3 * np.random.default_rng(n).normal(size=6)
        err = gm.edge_error(Xi, gm.retract(Xj, d), Z)
        assert err @ om @ err == pytest.approx(d @ (H / s2) @ d, rel=2e-2)
    # a registration whose final evaluation is not valid keeps the constant
    lc2, gr2, loops2 = _run(RefiningMap(3.0, flags=api.COV_VALID | api.COV_SINGULAR), refine=dict(min_fraction=0.5), loop_info="solve")
    assert loops2 and all(np.array_equal(e["info"], loop.LOOP_INFO) for e in gr2.edge_list if e["kind"] == 1)


def test_relocalize_picks_the_best_registered_row():
    """Liodom._refine_poses (relocalize / relocalize_global with refine=): one register_poses call; the row with the most matches
    among the CONVERGED ones, failing that among the MAX_PASSES ones, None if neither; ties go to the earlier row."""
    class Rows:
        def __init__(self, rows):
            self.rows, self.calls = rows, []

        def register_poses(self, edges, poses, **options):
            self.calls.append((np.asarray(poses).shape, options))
            return [dict(termination=t, matches=m) for t, m in self.rows]

    C, M, F = api.REG_CONVERGED, api.REG_MAX_PASSES, api.REG_FEW_MATCHES
    poses = np.tile([0.0, 0, 0, 1, 0, 0, 0], (3, 1))
    for rows, want in (([(M, 90), (C, 40), (C, 55)], 2), ([(C, 55), (M, 90), (C, 55)], 0), ([(F, 3), (M, 20), (M, 30)], 2),
                       ([(F, 3), (api.REG_NO_MAP, 0), (api.REG_EVAL_FAILURE, 50)], None)):
        mp = Rows(rows)
        best, out = api.Liodom._refine_poses(mp, _cloud((0, 0, 0)), poses, dict(max_passes=4))
        assert best == want and len(out) == 3 and mp.calls == [((3, 7), dict(max_passes=4))]
