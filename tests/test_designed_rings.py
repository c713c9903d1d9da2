"""The designed rings of tests/designed_rings.py against the oracle and the Python transcription alone (no GPU): on every ring
orc.extract == pyref.extract (as ring 8 of a 16-line cloud and as a row of a lidar_type 1 cloud), the oracle's smoothness
equals the generator's own bit for bit, and the ring shows what its family says it shows — taken from that smoothness and those
picks, so that no family passes by being empty.  The two rules a kernel deciding on its 32-bit keys alone would follow are
transcribed (designed_rings.select_ring) and shown to disagree with the oracle on the family aimed at each."""
import numpy as np
import pytest

import designed_rings as dr
import pyref


def ring8(orc, case, i):
    """Ring i of the case as the only ring (8) of a 16-line cloud: (picks in output order, smoothness)."""
    row = case.rows[i]
    p = orc.make_params(scan_lines=16, scan_regions=case.R, edges_per_region=case.epr)
    o = orc.extract(p, row, 16, 0, want_curv=True)
    ref = pyref.extract(row, 16, 0, lidar_type=0, scan_lines=16, scan_regions=case.R, edges_per_region=case.epr)
    assert list(zip(o["ring"].tolist(), o["idx_in_ring"].tolist(), o["src"].tolist())) == ref
    assert (o["ring"] == 8).all() and np.array_equal(o["edges"].view(np.uint32), row[o["src"]].view(np.uint32))
    offs, order = orc.split(p, row, 16, 0)
    assert offs[8] == 0 and offs[9] == len(row) and np.array_equal(order, np.arange(len(row))), "not all of it in ring 8"
    c, mine = o["curv"][:len(row)], dr.smoothness(row)
    if len(row) < case.R * case.epr + 10:                         # a ring below min_points_per_scan is skipped: no smoothness
        assert np.isnan(c).all() and not ref
        return [], mine
    assert np.array_equal(np.isnan(c), np.isnan(mine)) and np.array_equal(c[5:-5].view(np.uint64), mine[5:-5].view(np.uint64))
    return o["idx_in_ring"].tolist(), c


def as_rows(orc, case):
    """The case as one lidar_type 1 cloud: picks per row, in output order."""
    x, H, W = dr.pack(case.rows)
    p = orc.make_params(lidar_type=1, scan_lines=H, scan_regions=case.R, edges_per_region=case.epr)
    o = orc.extract(p, x, H, W)
    ref = pyref.extract(x, H, W, lidar_type=1, scan_lines=H, scan_regions=case.R, edges_per_region=case.epr)
    assert list(zip(o["ring"].tolist(), o["idx_in_ring"].tolist(), o["src"].tolist())) == ref
    return [o["idx_in_ring"][o["ring"] == r].tolist() for r in range(H)]


def check_both_ways(orc, case):
    rows = as_rows(orc, case)
    out = []
    for i in range(len(case.rows)):
        picks, c = ring8(orc, case, i)
        assert picks == rows[i], (case.name, i)
        assert picks == dr.select_ring(case.rows[i], case.R, case.epr), (case.name, i)
        out.append((picks, c))
    return out


def by_region(picks, n, R):
    regs = dr.regions_of(n, R)
    return [[j for j in picks if a <= j < b] for a, b in regs]


@pytest.mark.parametrize("R", [4, 6])
def test_ties(orc, R):
    case = dr.ties(R)
    (picks, c), = check_both_ways(orc, case)
    info = case.info[0]
    for lo, hi, placement in info["pairs"]:
        assert c[hi] > c[lo] and np.float32(c[hi]) == np.float32(c[lo]) and lo < hi, placement
        assert c[lo] == 1.5625 and c[hi] == 1.5625 + 100.0 * 2.0 ** -32
        assert lo in picks and hi in picks, "a tie whose two candidates are not both picked"
        olo, ohi = (lo - 5) % info["sector"], (hi - 5) % info["sector"]
        for ipl in (16, 24):
            same_lane, same_quad = olo // ipl == ohi // ipl, olo // (4 * ipl) == ohi // (4 * ipl)
            assert (same_lane, same_quad) == {"lane": (True, True), "quad": (False, True), "quads": (False, False)}[placement]
    for a, b in info["equal"]:
        assert c[a] == c[b] and a < b and a in picks and b in picks
    got = by_region(picks, len(case.rows[0]), R)
    for g, order in info["order"].items():
        assert got[g] == order, g                    # largest double first; lowest index among equal doubles
    assert all(not got[g] for g in range(4, R))
    g2 = info["order"][2]
    assert len({np.float32(c[j]).tobytes() for j in g2}) == 1 and len(g2) == 3       # one image, three items
    assert c[info["order"][1][0]] > c[info["order"][1][1]]                          # the tie of region 1 is among picks 2 and 3
    # the rule without the doubles is observable here
    wrong = dr.select_ring(case.rows[0], R, case.epr, "image_lowest_index")
    assert wrong != picks and sorted(wrong) == sorted(picks)


def test_cutoff(orc):
    case = dr.cutoff()
    res = check_both_ways(orc, case)
    tenth = np.float32(0.1)
    for (picks, c), info, row in zip(res, case.info, case.rows):
        j = info["j"]
        assert c[j] == info["c"] and np.float32(c[j]) == tenth
        assert (c[j] < 0.1) == (info["kind"] == "below")
        assert np.nanmax(np.delete(c, j)) < 0.05                  # nothing else near the cut-off
        assert picks == info["edges"]
        assert dr.select_ring(row, case.R, case.epr, "cutoff_on_image") == [j]
    below, at_least = case.info
    assert below["c"] < 0.1 <= at_least["c"] and at_least["c"] - below["c"] < 1e-9
    # the cut-off on the float image is observable on `below`
    assert dr.select_ring(case.rows[0], case.R, case.epr, "cutoff_on_image") != res[0][0]


@pytest.mark.parametrize("R", [2, 4])
def test_gaps(orc, R):
    case = dr.gaps(R)
    res = check_both_ways(orc, case)
    seen = set()
    for (picks, c), info, row in zip(res, case.info, case.rows):
        n = len(row)
        for j in [info["j"]] + ([info["j2"]] if "j2" in info else []):
            nf, nb = dr.extents(row, j)
            assert (nf, nb) == (info["nf"], info["nb"]), info
            g = [x <= j < y for x, y in dr.regions_of(n, R)].index(True)
            assert by_region(picks, n, R)[g][0] == j, "the designed pick is not its region's first"
            assert [q for q in picks if j - nb <= q <= j + nf] == [j], info
            for q, inside in ((j + nf, True), (j + nf + 1, False), (j - nb, True), (j - nb - 1, False)):
                if 5 <= q < n - 5 and q != j:
                    assert c[q] >= 0.1, (info, q)                 # a candidate sits on either side of the extent's end
                    assert (q in picks) != inside, (info, q)
        if info["kind"] == "gap":
            assert (info["j"] - 4) % 32 == info["shift"]
            assert int((~dr.continuity(row)[1:]).sum()) == 1 and not dr.continuity(row)[info["j"] + info["pos"]]
            seen.add((info["shift"], info["pos"]))
        if info["kind"] == "threshold":
            f = np.float32(info["step"])
            d = float(row[info["j"] + 3, 1] - row[info["j"] + 2, 1])
            assert d == float(f) and (d * d <= 0.05) == (info["nf"] == 5)
        if info["kind"] == "lane":
            assert (info["j"] - 5) % 80 in (15, 16, 23, 24)
    assert seen == {(s, p) for s in dr.GAP_SHIFTS for p in dr.GAP_POSITIONS}
    f = dr.threshold_step()
    steps = [i["step"] for i in case.info if i["kind"] == "threshold"]
    assert steps == [float(f), float(np.nextafter(f, np.float32(1)))] and steps[0] ** 2 <= 0.05 < steps[1] ** 2
    assert any(i["kind"] == "ends" and i["j"] == 5 and i["j2"] == len(case.rows[-1]) - 6 for i in case.info)


CASCADES = [(8, "base"), (16, "base"), (64, "base"), (4, "base"), (8, "twice"), (16, "twice"), (8, "sector5"), (16, "sector5")]


@pytest.mark.parametrize("R,variant", CASCADES)
def test_cascade(orc, R, variant):
    case = dr.cascade(R, variant)
    (picks, c), = check_both_ways(orc, case)
    row = case.rows[0]
    assert dr.continuity(row)[1:].all() and case.epr == 1
    rounds, final, history, remarks = dr.jacobi(row, R, 1)
    assert [j for p in final for j in p] == picks, "the fixed point is not the in-order walk"
    assert dr.jacobi_rounds(row, R, 1) == rounds
    if variant == "base":
        assert rounds == R - 1
        assert picks == case.info[0]["C"]                         # every region picks C, and only C
        spec = [j for g, (a, b) in enumerate(dr.regions_of(len(row), R)) for j in [a + 1] if g]
        assert all(c[a] > c[a + 5] >= 0.1 for a in spec)          # A is the stronger one: the spill-free run picks it
    elif variant == "twice":
        assert rounds >= 2
        assert any(old and new and old != new for _, old, new in remarks), remarks
        twice = {g for g, old, new in remarks if old and new}
        assert any(len({h[g] for h in history}) >= 3 for g in twice)                 # 0 is not among them: three masks
    else:
        assert rounds >= 2
        regs = dr.regions_of(len(row), R)
        whole = [g for g in range(1, R) if history[-1][g] == 31]
        assert whole and all(not [j for j in picks if regs[g][0] <= j < regs[g][1]] for g in whole)
        assert all(regs[g][1] - 1 in picks and np.nanmax(c[regs[g][0]:regs[g][1]]) >= 0.1 for g in [w - 1 for w in whole])


BOUNDARIES = {c.name: c for c in dr.boundaries()}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_boundary(orc, name):
    case = BOUNDARIES[name]
    (picks, c), = check_both_ways(orc, case)
    row, info = case.rows[0], case.info[0]
    n, R = len(row), case.R
    assert dr.continuity(row)[1:].all() and info["fast"] == dr.register_path(n, R, info["ipl"])
    if n < R * case.epr + 10:
        assert picks == [] and np.nanmax(c) >= 0.1                # skipped for its length, not for want of candidates
        return
    # suppression is active: candidates stronger than their region's weakest pick are passed over (they were marked)
    marked = 0
    for a, b in dr.regions_of(n, R):
        got = [j for j in picks if a <= j < b]
        if got:
            marked += sum(1 for q in range(a, b) if q not in got and c[q] > min(c[j] for j in got))
        if len(got) <= case.epr:                                  # (picks left: every candidate that is not picked was marked)
            marked += int((c[a:b] >= 0.1).sum()) - len(got)
    assert marked > 0 and len(picks) > 0


def test_boundary_shapes_straddle_the_predicate():
    fast = {c.name: c.info[0]["fast"] for c in dr.boundaries()}
    for inside, outside in (("len256", "len257"), ("len384", "len385"), ("sector5", "sector4"), ("r64", "r65"), ("nr16384", "nr16385")):
        assert fast[inside] and not fast[outside]
    shape = {name: (R, epr, n) for name, R, epr, n, _ in dr.BOUNDARY_SHAPES}
    for name, longest in (("len256", 256), ("len257", 257), ("len384", 384), ("len385", 385)):
        R, _, n = shape[name]
        assert max(b - a for a, b in dr.regions_of(n, R)) == longest
    assert dr.register_path(shape["len257"][2], 4, 24) and not dr.register_path(shape["len385"][2], 4, 24)
    R, epr, n = shape["r6_long_last"]
    regs = dr.regions_of(n, R)
    assert (regs[-1][1] - regs[-1][0]) - (regs[0][1] - regs[0][0]) == R - 1
    assert shape["r6_min"][2] == 6 * 5 + 10 and shape["r6_below_min"][2] == 6 * 5 + 9 and shape["r7"][0] % 4 and R % 4
    assert max(abs(dr.base_y(16385))) <= 64 and np.nanmax(dr.smoothness(dr.base_ring(16385).astype(np.float32))) < 0.1


@pytest.mark.parametrize("epr", [2, 0])
@pytest.mark.parametrize("pattern", dr.COUNT_PATTERNS)
@pytest.mark.parametrize("H", [16, 129, 254])
def test_counts(orc, H, pattern, epr):
    case = dr.counts(H, pattern, epr)
    want = case.info[0]["want"]
    x, h, W = dr.pack(case.rows, W=dr.COUNT_W)
    assert (h, W) == (H, dr.COUNT_W)
    p = orc.make_params(lidar_type=1, scan_lines=H, scan_regions=case.R, edges_per_region=epr)
    o = orc.extract(p, x, H, W)
    assert np.array_equal(np.bincount(o["ring"], minlength=H), want)
    full = case.R * (epr + 1)
    if pattern == "full":
        assert len(o["ring"]) == H * full
    else:
        assert (want == 0).any() and want.max() == full
        assert {"ends_empty": want[0] == 0 and want[-1] == 0 and want[1] > 0, "last_only": want[:-1].sum() == 0,
                "middle_run": (want[H // 2 - 1:H // 2 + 2] == 0).all() and want[0] > 0 and want[-1] > 0}[pattern]
        assert any(r is None for r in case.rows)
    if H == 16 or (pattern, epr) == ("middle_run", 2):
        ref = pyref.extract(x, H, W, lidar_type=1, scan_lines=H, scan_regions=case.R, edges_per_region=epr)
        assert list(zip(o["ring"].tolist(), o["idx_in_ring"].tolist(), o["src"].tolist())) == ref


def test_stream_families(orc):
    """What the streams of one launch carry in tests/test_gpu_designed_extract.py (one parameter set for all: R = 4, epr = 5): the
    families keep what they are designed for, and no two inputs have the same answer."""
    R, epr, H, W = dr.STREAM_R, dr.STREAM_EPR, dr.STREAM_H, dr.STREAM_W
    p = orc.make_params(lidar_type=1, scan_lines=H, scan_regions=R, edges_per_region=epr)
    answers = {}
    for name, rows in dr.stream_families():
        x = dr.pack(rows, H=H, W=W)[0]
        o = orc.extract(p, x, H, W)
        ref = pyref.extract(x, H, W, lidar_type=1, scan_lines=H, scan_regions=R, edges_per_region=epr)
        assert list(zip(o["ring"].tolist(), o["idx_in_ring"].tolist(), o["src"].tolist())) == ref
        answers[name] = (o["ring"].tobytes(), o["idx_in_ring"].tobytes())
        if name == "ties":
            assert o["idx_in_ring"].tolist() == [j for g in range(4) for j in dr.ties(R).info[0]["order"][g]]
        if name == "cutoff":
            assert o["ring"].tolist() == [1]
        if name == "cascade":
            assert [dr.jacobi_rounds(r, R, epr) for r in rows[:2]] == [R - 1, R - 1] and dr.jacobi(rows[1], R, epr)[3]
    assert len(set(answers.values())) == len(answers)
    p0 = orc.make_params(scan_lines=16, scan_regions=R, edges_per_region=epr)
    rings = dr.stream_rings()
    got = [orc.extract(p0, r, 16, 0)["idx_in_ring"].tobytes() for _, r in rings]
    assert len(set(got)) == len(rings) >= 16
