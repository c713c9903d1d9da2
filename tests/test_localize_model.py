"""The localisation model on the CPU oracle (tests/localize_model.py): what the GPU tests of liodom_attach_map_reader and
liodom_seed_stream compare against is itself a run that solves against the map.  CPU only."""
import numpy as np

import localize_model as lm
from mapper_lag_common import map_part_correspondences


def test_the_site_map(orc, synth):
    mo = lm.site_map(orc, synth)
    assert mo.num_cells() == 29 and mo.all().shape[0] == 2640


def test_the_reader_loop_solves_against_the_map(orc, synth):
    run = lm.oracle_reader_run(orc, synth)
    assert len(run) == 14
    assert run[0]["recv"].shape[0] == 0 and np.array_equal(run[0]["pose"], [0, 0, 0, 1, 0, 0, 0])      # the reference's first frame
    for j, rec in enumerate(run[1:], start=1):
        assert rec["recv"].shape[0] == 1609, j
        assert rec["term"] == [2, 2], (j, rec["term"])
        for it in (0, 1):
            v = rec["corr"][it][0]
            n = int(v.sum())
            assert n == rec["matches"][it] and 116 <= n <= 540, (j, it, n)
        in_map = map_part_correspondences(rec)      # both passes together
        assert 120 <= in_map <= 360, (j, in_map)


def test_the_seeded_first_scan_solves(orc, synth):
    for name, seed in lm.seeds(orc, synth).items():
        m = lm.seeded_first_scan(orc, synth, seed)
        assert m["recv"].shape[0] == 1609, name
        for p in m["passes"]:
            assert p["trace"][0] == 2 and p["matches"] >= 1, (name, p["trace"], p["matches"])
