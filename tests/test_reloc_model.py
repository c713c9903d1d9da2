"""The relocalisation score on the CPU (tests/reloc_model.py): on the oracle's site map the ground truth is the unique best
candidate of a grid around it under score = hits_r + hits_0, the 27-probe count alone does not rank it first, and the designed
cases give the counts written down by hand.  CPU only."""
import numpy as np
import pytest

import localize_model as lm
import reloc_model as rm

GRID = dict(step_xy=0.4, step_yaw=0.05, nx=5, ny=5, nyaw=4)      # 11 x 11 x 9 = 1089 candidates, the truth at index 544
_CACHE = {}


def _site_occupancy(orc, synth):
    if "occ" not in _CACHE:
        _CACHE["occ"] = rm.Occupancy(rm.state_from_points(lm.site_map(orc, synth).all()))
    return _CACHE["occ"]


def test_the_site_occupancy(orc, synth):
    occ = _site_occupancy(orc, synth)
    assert occ.n_cells == 29 and occ.occ.size == 2640          # one point per leaf: what VoxelGrid leaves
    assert (occ.gx, occ.gy, occ.gz, occ.words) == (105, 105, 130, 44790)


@pytest.mark.parametrize("scan", [0, 5, 11])
def test_truth_is_the_unique_best_on_the_grid(orc, synth, scan):
    occ = _site_occupancy(orc, synth)
    _, edges, gt = lm.traversal(orc, synth, 1)[scan]
    T, poses, idx = rm.candidate_grid(gt, **GRID)
    assert T.shape[0] == 1089 and tuple(idx[544]) == (0, 0, 0, 0) and np.allclose(poses[544], lm.normalised(gt), atol=1e-15)
    hits = occ.hits(edges, T, radius=1).astype(np.int64)
    score = hits[:, 0] + hits[:, 1]
    order = np.argsort(-score, kind="stable")
    print("scan %d: %d edges, truth %d = %d + %d, runner-up %d, median %d; best by hits_r alone: index %d (%d vs %d at the truth)"
          % (scan, edges.shape[0], score[544], hits[544, 0], hits[544, 1], score[order[1]], int(np.median(score)), int(np.argmax(hits[:, 0])),
             hits[:, 0].max(), hits[544, 0]))
    assert rm.best_of(hits) == 544 and order[0] == 544
    assert score[order[1]] < score[544]                         # unique
    if scan in (5, 11):
        # why the score is the sum: ranked by the 27-probe count alone, a neighbour one leaf away beats the truth
        assert int(np.argmax(hits[:, 0])) != 544 and hits[:, 0].max() > hits[544, 0]


def test_designed_cases_against_hand_written_counts(orc):
    mo = orc.Map()
    mo.update(rm.DESIGNED_MAP, np.eye(4)[:3])
    state = rm.state_from_points(mo.all())
    occ = rm.Occupancy(state)
    assert occ.n_cells == rm.DESIGNED_CELLS and occ.occ.size == rm.DESIGNED_MAP.shape[0] - 1      # two points shared a leaf
    edges, want = rm.designed_edges()
    T = rm.designed_candidates()
    for radius in (0, 1):
        hits = occ.hits(edges, T, radius=radius)
        assert tuple(hits[0]) == want[radius], (radius, hits[0])
        assert tuple(hits[1]) == (0, 0)
        # edge by edge, so that a wrong case names itself
        for i, (p, h0, hr) in enumerate(rm.DESIGNED_EDGES):
            one = occ.hits(edges[i:i + 1], T[:1], radius=radius)[0]
            assert tuple(one) == ((hr if radius else h0), h0), (radius, i, p, one)
    assert want[0] == (10, 10) and want[1] == (13, 10)
    # radius 0: hits_r == hits_0 for every candidate
    h = occ.hits(edges, T, radius=0)
    assert np.array_equal(h[:, 0], h[:, 1])


def test_crafted_first_and_last_word():
    blob, edges, want, (leaves, words) = rm.crafted_state_blob()
    from liodom_amd import api
    occ = rm.Occupancy(api.parse_map_state(blob))
    assert sorted(occ.occ.tolist()) == [0, 2 * leaves - 1] and (2 * leaves - 1 - leaves) // 32 == words - 1
    for radius in (0, 1):
        assert tuple(occ.hits(edges, np.eye(4)[:3].reshape(1, 12), radius=radius)[0]) == want[radius]


def test_ties_and_empty_inputs():
    occ = rm.Occupancy(rm.state_from_points(rm.DESIGNED_MAP))
    T = rm.designed_candidates()
    assert occ.hits(np.zeros((0, 4), np.float32), T).tolist() == [[0, 0]] * 4
    assert rm.best_of(np.zeros((7, 2), np.int32)) == 0 and rm.best_of(np.array([[1, 0], [2, 1], [3, 0]])) == 1
