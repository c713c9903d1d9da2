"""The per-scan hit record and the kidnap run on the CPU alone (tests/map_hits_model.py: reloc_model.Occupancy at the poses of the
oracle's reader loop): the record's invariants, that the kidnap scenario separates a tracking reader from a lost one by at least 0.2
in the hit fraction, and what the "lost" policy answers on it with min_fraction = (f_track + f_lost) / 2.  No GPU."""
import numpy as np

from liodom_amd import api
import localize_model as lm
import map_hits_model as mh
from mapper_lag_common import rot_angle


def test_records_of_the_reader_loop(orc, synth):
    r1, r0 = mh.reader_records(orc, synth, 1), mh.reader_records(orc, synth, 0)
    tr = lm.traversal(orc, synth, 1)
    assert len(r1) == len(r0) == len(tr)
    for k, (a, b) in enumerate(zip(r1, r0)):
        assert a["scan_index"] == b["scan_index"] == k and a["n_edges"] == b["n_edges"] == tr[k][1].shape[0]
        assert 0 <= a["hits_0"] <= a["hits_r"] <= a["n_edges"]
        assert b["hits_r"] == b["hits_0"] == a["hits_0"]              # radius 0: one probe; the centre probe does not depend on the radius
        assert np.array_equal(a["T"], b["T"]) and a["T"].shape == (3, 4)
    print("fractions of the reader loop, radius 1:", [round(r["fraction"], 3) for r in r1])
    assert min(r["fraction"] for r in r1[1:]) > 0.8                  # a reader that tracks lies in its map


def test_the_kidnap_run_separates(orc, synth):
    run = mh.kidnap_run(orc, synth)
    print("f_track %.4f  f_lost %.4f  min_fraction %.4f" % (run["f_track"], run["f_lost"], run["min_fraction"]))
    print("fractions:", [round(r["fraction"], 3) for r in run["records"]], "at the truth:", [round(v, 3) for v in run["at_truth"]])
    assert run["f_track"] - run["f_lost"] >= 0.2
    assert run["f_lost"] < run["min_fraction"] < run["f_track"]
    # the scenario is what it says: the tracked scans end near their truth, the kidnapped ones do not, although their truth
    # scores above the threshold (the place is in the map: a recovery can succeed)
    scans = mh.kidnap_scans(orc, synth)
    assert [s[3] for s in scans] == list(range(mh.TRACKED)) + list(range(mh.KIDNAP_AT, mh.KIDNAP_AT + mh.KIDNAPPED))
    for j, (_, _, gt, _) in enumerate(scans):
        dt, dr = np.linalg.norm(run["poses"][j][4:] - gt[4:]), rot_angle(run["poses"][j][:4], gt[:4])
        assert (dt < 0.1 and dr < 0.01) == (j < mh.TRACKED), (j, dt, dr)
        assert run["at_truth"][j] >= run["min_fraction"], j
    jump = np.linalg.norm(scans[mh.TRACKED][2][4:] - scans[mh.TRACKED - 1][2][4:])
    assert 2.0 < jump < 3.0


def test_what_the_policy_answers_on_the_kidnap_run(orc, synth):
    run = mh.kidnap_run(orc, synth)
    for lost_after in (1, 2, 3):
        states = mh.predicted_states(run["records"], run["min_fraction"], lost_after)
        assert states[:mh.TRACKED + lost_after - 1] == [api.TRACKING] * (mh.TRACKED + lost_after - 1)
        assert states[mh.TRACKED + lost_after - 1] == api.LOST, (lost_after, states)
    assert mh.predicted_states(run["records"][:mh.TRACKED], run["min_fraction"], 1) == [api.TRACKING] * mh.TRACKED
