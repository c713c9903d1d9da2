"""Shared by the map-hit tests: the per-scan hit record on the CPU — reloc_model.Occupancy of the site map at the pose the oracle's
reader loop (localize_model.py) returned — and the kidnap run.  Everything here is computed once and never modified.

The record of scan k: edges = the scan's edge cloud (sensor frame), T = T_of(pose_k), (hits_r, hits_0) = Occupancy.hits(edges, T,
radius), fraction = (hits_r + hits_0) / (2 n_edges).

The kidnap run: an unseeded reader of the site map is fed scans 0 .. TRACKED - 1 of the localising traversal (synth stream 1), then
scans KIDNAP_AT .. KIDNAP_AT + KIDNAPPED - 1 of the same stream, and is not reseeded.  Scan KIDNAP_AT = 30 was taken 2.5 m and
0.22 rad from scan 5 — still on the site (its ground-truth pose scores 0.72), but beyond what the solve's correspondences reach:
neither the window nor the local map, transformed by the predicted pose, puts a line within a query's neighbourhood, so the solve
stays where the prediction put it and slides along its own window.
  f_track   the smallest fraction over the tracked scans
  f_lost    the largest fraction over the kidnapped scans
  min_fraction = (f_track + f_lost) / 2: what every test gives its policy."""
import numpy as np

from liodom_amd import api
import localize_model as lm
import reloc_model as rm
from mapper_lag_common import H, W, T_of

TRACKED, KIDNAP_AT, KIDNAPPED = 6, 30, 4
LOST_AFTER = 2
RADIUS = 1
# the recovery's search: a branch-and-bound level wide enough for the jump, then the relocaliser's fine level
LEVELS = [dict(bnb=True, step_xy=0.4, step_yaw=0.02, nx=12, ny=12, nyaw=20), dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]

_CACHE = {}


def site_occupancy(orc, synth):
    if "occ" not in _CACHE:
        _CACHE["occ"] = rm.Occupancy(rm.state_from_points(lm.site_map(orc, synth).all()))
    return _CACHE["occ"]


def record(occ, k, edges, pose, radius=RADIUS):
    """The hit record of a scan as a dict: what liodom_map_hit_t holds, plus the fraction."""
    T = T_of(pose)
    hr, h0 = (int(v) for v in occ.hits(edges, T.reshape(1, 12), radius=radius)[0])
    n = int(edges.shape[0])
    return dict(scan_index=k, n_edges=n, hits_r=hr, hits_0=h0, radius=radius, T=T, flags=api.HIT_VALID,
                fraction=api.TrackPolicy.fraction(hr, h0, n))


def reader_records(orc, synth, radius=RADIUS):
    """One record per scan of localize_model.oracle_reader_run."""
    key = ("reader", radius)
    if key not in _CACHE:
        occ, run = site_occupancy(orc, synth), lm.oracle_reader_run(orc, synth)
        _CACHE[key] = [record(occ, k, e, run[k]["pose"], radius) for k, (_, e, _) in enumerate(lm.traversal(orc, synth, 1))]
    return _CACHE[key]


def kidnap_scans(orc, synth):
    """[(scan, edges, gt pose[7], its number in stream 1)] of the kidnap run."""
    if "scans" not in _CACHE:
        cfg, po = synth.make_cfg(H, W, 0), lm.params(orc)
        out = []
        for k in list(range(TRACKED)) + list(range(KIDNAP_AT, KIDNAP_AT + KIDNAPPED)):
            x, gt = synth.scan(cfg, 1, k)
            out.append((x, orc.extract(po, x, H, W)["edges"], gt.copy(), k))
        _CACHE["scans"] = out
    return _CACHE["scans"]


def kidnap_run(orc, synth):
    """The oracle's reader loop over the kidnap run, never reseeded: dict(records, poses, f_track, f_lost, min_fraction, at_truth)
    — at_truth: the fraction of each scan under its ground-truth pose (what a recovery can reach)."""
    if "kidnap" not in _CACHE:
        mo, occ = lm.site_map(orc, synth), site_occupancy(orc, synth)
        od = orc.Odometer(lm.params(orc))
        recs, poses, at_truth = [], [], []
        for j, (_, e, gt, _) in enumerate(kidnap_scans(orc, synth)):
            pose, _ = od.step(e)
            recs.append(record(occ, j, e, pose))
            at_truth.append(record(occ, j, e, gt)["fraction"])
            poses.append(pose.copy())
            od.set_received_map(mo.local(T_of(pose), *lm.CELLS))
        od.close()
        f_track = min(r["fraction"] for r in recs[:TRACKED])
        f_lost = max(r["fraction"] for r in recs[TRACKED:])
        _CACHE["kidnap"] = dict(records=recs, poses=poses, f_track=f_track, f_lost=f_lost, min_fraction=0.5 * (f_track + f_lost), at_truth=at_truth)
    return _CACHE["kidnap"]


def predicted_states(records, min_fraction, lost_after=LOST_AFTER):
    """What a TrackPolicy answers for the records, in order."""
    p = api.TrackPolicy(min_fraction, lost_after)
    return [p.feed(r["hits_r"], r["hits_0"], r["n_edges"], r["flags"]) for r in records]
