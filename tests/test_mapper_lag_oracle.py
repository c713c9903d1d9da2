"""The lagged mapper's loop on the CPU oracle alone (orc.Odometer + orc.Map; mapper_lag_common.oracle_lagged_run): guards the
inputs of tests/test_gpu_mapper_lag.py — with a mapper that holds only what has left the sliding window the solves run, their
correspondences reach into the map, and the stream moves.  No GPU."""
import numpy as np

from mapper_lag_common import K, P, map_part_correspondences, oracle_lagged_run


def test_lagged_loop_solves_on_the_oracle(orc, synth):
    run = oracle_lagged_run(orc, synth)
    assert len(run) == K
    for j, rec in enumerate(run):
        assert rec["n_recv"] == 0 or j > P, j        # the first received map is the one scan P leaves behind
        if j > P:
            assert rec["n_recv"] > 0 and rec["map_points"] == rec["n_window"] + rec["n_recv"], j
        if j >= P:                                   # the window is full: no solve gives up (termination 5 is the degenerate replay's)
            assert 5 not in rec["term"], (j, rec["term"])
    used_map = sum(map_part_correspondences(rec) for rec in run[P + 1:])
    assert used_map > 50, used_map
    assert np.linalg.norm(run[-1]["pose"][4:]) > 0.5
