"""The NumPy restatement of Map::getLocalMap (tests/local_map_model.py) against the CPU oracle, and the conditions its designed
worlds were built for, so that no case of tests/test_gpu_designed_local.py passes by being empty.  CPU only.

The oracle maps are built from the worlds' points through orc.Map.update (the reference's VoxelGrid included), the model reads
the worlds' states: local() must equal orc.Map.local bit for bit for every pose and extent the GPU tests use."""
import numpy as np
import pytest

import local_map_model as lmm

def cases(name):
    """(pose, cells_xy, cells_z) of every local map the GPU tests ask of the world."""
    if name == "counts":
        return [(T, cxy, cz) for T in lmm.COUNTS_POSES for cxy, cz in lmm.COUNTS_EXTENTS + [lmm.STEP_EXTENTS]]
    if name == "frac":
        c = lmm.frac_cells_xy()
        return [(T, cxy, lmm.FRAC_CELLS_Z) for T in lmm.FRAC_POSES for cxy in (c, c + 1)]
    if name == "ones":
        return [(lmm.ones_pose(), 40, 0)]
    if name == "ones-65x63":
        return [(lmm.ones_pose(65, 63), 40, 0)]
    return [(lmm.GUARD_POSE, 127, 0), (lmm.GUARD_POSE, 128, 0)]


@pytest.mark.parametrize("name", ["counts", "frac", "ones", "ones-65x63", "guard"])
def test_model_equals_the_oracle_bit_for_bit(orc, name):
    w, mo = lmm.world(name), lmm.oracle_map(orc, name)
    sizes = []
    for T, cxy, cz in cases(name):
        want = mo.local(T, cxy, cz)
        got = lmm.local(w["state"], T, w["sizes"], cxy, cz)
        assert lmm.same(got, want), (name, T[:, 3], cxy, cz, got.shape, want.shape)
        assert lmm.visit_size(T, w["sizes"], cxy, cz) == len(lmm.visit(T, w["sizes"], cxy, cz))
        sizes.append(got.shape[0])
    print("%s: local map sizes %s" % (name, sizes))
    assert max(sizes) > 0


def test_counts_reaches_what_it_was_designed_for():
    w = lmm.world("counts")
    st, sz = w["state"], w["sizes"]
    origin = lmm.COUNTS_POSES[0]
    assert lmm.centre_of(origin, sz) == (2, 2, 2)
    # the deal, read back from the state in visit order
    keys = lmm.visit(origin, sz, 3, 0)
    assert len(keys) == 50 and keys[49] == keys[lmm.COUNTS_CENTRE] == (2, 2, 2)
    by = dict(zip(st["keys"], st["cells"]))
    got = [by[k].shape[0] if k in by else 0 for k in keys[:49]]
    assert got == lmm.counts_deal() and [i for i, n in enumerate(got) if n == 0] == list(lmm.COUNTS_HOLES)
    assert got[24:27] == [257, 1, 1000] and set(got) - {0} == set(lmm.COUNT_SET)
    assert by[(2, 2, 7)].shape[0] == 65 and by[(2, 2, -2)].shape[0] == 513 and len(st["keys"]) == 48
    assert st["keys"] != sorted(st["keys"]) and [st["keys"].index(k) for k in keys[:49] if k in by] != sorted(st["keys"].index(k) for k in keys[:49] if k in by)
    # distinct leaf centres inside their cell, ascending (z, y, x); the intensity is the running index
    allp = np.concatenate(st["cells"])
    assert np.array_equal(allp[:, 3], np.arange(len(allp), dtype=np.float32))
    for k, c in zip(st["keys"], st["cells"]):
        leaf = np.floor(c[:, :3].astype(np.float64) * 4.0).astype(np.int64)
        assert np.array_equal(c[:, :3].astype(np.float64), (leaf + 0.5) * 0.25)
        lin = (leaf[:, 2] * (1 << 20) + leaf[:, 1]) * (1 << 20) + leaf[:, 0]
        assert (np.diff(lin) > 0).all()
        lo = np.array([k[0] - 2, k[1] - 2, {2: 0, 7: 5, -2: -5}[k[2]]])
        assert (c[:, :3] > lo).all() and (c[:, :3] < lo + [4, 4, 5]).all()
    # the extents of the host-call tests: (0, 0) and (1, 0) visit the centre twice, (1, 0) and (2, 1) scan over holes, (2, 1) reaches
    # the cell below through the column, (3, 2)'s column lands on no cell
    assert lmm.visit(origin, sz, 0, 0) == [(2, 2, 2), (2, 2, 2)]
    assert lmm.visit(origin, sz, 1, 0).count((2, 2, 2)) == 2 and (2, -2, 2) not in by and (2, -2, 2) in lmm.visit(origin, sz, 1, 0)
    assert lmm.visit(origin, sz, 2, 1)[25:] == [(2, 2, -2), (2, 2, 3)] and (-6, 2, 2) not in by and (-6, 2, 2) in lmm.visit(origin, sz, 2, 1)
    assert lmm.visit(origin, sz, 3, 2)[49:] == [(2, 2, -6), (2, 2, -1), (2, 2, 4), (2, 2, 9)]
    # the poses: +-0.9 is the origin's visit (truncation, not floor); the boundary poses differ from each other; one is empty, one
    # finds some but not all of the square
    for T in lmm.COUNTS_POSES[1:7]:
        assert lmm.visit(T, sz, 3, 2) == lmm.visit(origin, sz, 3, 2)
    assert lmm.centre_of(lmm.COUNTS_POSES[7], sz) == (6, -2, 2) and lmm.centre_of(lmm.COUNTS_POSES[8], sz) == (2, -2, 7)
    full = lmm.local(st, origin, sz, 3, 0).shape[0]
    assert lmm.local(st, lmm.COUNTS_POSES[10], sz, 3, 2).shape[0] == 0
    assert 0 < lmm.local(st, lmm.COUNTS_POSES[9], sz, 3, 0).shape[0] < full
    assert np.array_equal(lmm.COUNTS_POSES[11], lmm.COUNTS_POSES[1])
    assert len(lmm.COUNTS_POSES) == 12 and all(lmm.rows_fit(sz, cxy, cz) for cxy, cz in lmm.COUNTS_EXTENTS + [lmm.STEP_EXTENTS])


def test_step_capacities_cut_where_they_should():
    """Every capacity of the step tests against the plan of the origin's local map with STEP_EXTENTS, and the slices a
    k_map_local_rows launch deals the truncated row to."""
    w = lmm.world("counts")
    en = lmm.entries(w["state"], lmm.COUNTS_POSES[0], w["sizes"], *lmm.STEP_EXTENTS)
    caps = lmm.step_caps(w)
    total = en[-1][1] + en[-1][2]
    assert len(en) == 47 and total > 16 * 256 and total == lmm.local(w["state"], lmm.COUNTS_POSES[0], w["sizes"], *lmm.STEP_EXTENTS).shape[0]
    ends = [o + n for _, o, n in en]
    inside = lambda cap: [e for e in en if e[1] < cap < e[1] + e[2]]      # noqa: E731  the entry the cut falls into
    first, second = [e for e in en if e[0] == en[-1][0]]
    assert first[2] == second[2] == 257 and second is en[-1] and first[1] + 257 < second[1]
    assert (caps["one"], caps["256"], caps["257"]) == (1, 256, 257) and inside(256) and inside(257)
    assert caps["entry_end"] in ends and caps["entry_end"] % 256 != 0 and caps["entry_end+1"] - 1 == caps["entry_end"]
    assert not inside(caps["entry_end"]) and inside(caps["entry_end+1"]) == [en[3]] and en[3][1] == caps["entry_end"]      # one point of the next
    assert inside(caps["in_first_copy"]) == [first] and inside(caps["in_second_copy"]) == [second]
    assert (caps["total-1"], caps["total"], caps["total+1"]) == (total - 1, total, total + 1) and inside(total - 1) == [second]
    assert len(set(caps.values())) == 10 and tuple(caps) == lmm.STEP_CAP_NAMES
    print("counts, origin, %s: %d points in %d entries; capacities %s" % (lmm.STEP_EXTENTS, total, len(en), caps))
    # the slices: at the full size a row uses all 16 workgroups; slices start and end inside cells, hold entries smaller than
    # themselves (the one-point neighbour of the centre among them) and cut the centre's copies
    starts_inside, whole_inside = 0, 0
    for name, cap in caps.items():
        sl = lmm.rows_slices(total, cap)
        n = min(total, cap)
        assert sl[0][0] == 0 and max(hi for _, hi in sl) == n and all(a[1] == b[0] or b[0] == b[1] == n for a, b in zip(sl, sl[1:]))
        if cap >= 16 * 256:
            assert len(sl) == 16 and all(hi > lo for lo, hi in sl)
        starts_inside += sum(1 for lo, _ in sl[1:] if lo < n and inside(lo))
        whole_inside += sum(1 for lo, hi in sl for _, o, c in en if lo < o and o + c < hi)
    assert starts_inside >= 10 and whole_inside >= 10
    sl = lmm.rows_slices(total, total)
    one = [e for e in en if e[2] == 1 and e[1] == first[1] + 257][0]
    assert any(lo < one[1] and one[1] + 1 < hi for lo, hi in sl)
    # the lock-step test's capacity: the origin's local map with LOCKSTEP_EXTENTS fits it exactly; its slices are shorter than the
    # centre cell, so a slice edge falls inside the centre's first copy and another inside its second
    cap = lmm.lockstep_cap(w)
    en = lmm.entries(w["state"], lmm.COUNTS_POSES[0], w["sizes"], *lmm.LOCKSTEP_EXTENTS)
    first, second = [e for e in en if e[0] == en[-1][0]]
    sl = lmm.rows_slices(cap, cap)
    assert cap == second[1] + 257 and 1 < len(sl) < 16 and sl[0][1] < 257
    for copy in (first, second):
        assert any(copy[1] < lo < copy[1] + 257 for lo, _ in sl), copy
    assert cap < total and any(lo < caps["entry_end"] < hi for lo, hi in lmm.rows_slices(total, cap))


def test_the_plan_worlds_meet_their_limits():
    # ones: more found cells than the plan holds; the device keeps the first 4096 in visit order
    w = lmm.world("ones")
    T = lmm.ones_pose()
    assert len(w["state"]["keys"]) == 4200 and all(c.shape[0] == 1 for c in w["state"]["cells"])
    assert len(lmm.visit(T, w["sizes"], 40, 0)) == 81 * 81 + 1 and not lmm.rows_fit(w["sizes"], 40, 0)
    assert lmm.local(w["state"], T, w["sizes"], 40, 0).shape[0] == 4201 > lmm.ENTRIES_MAX
    got, over = lmm.local_device(w["state"], T, w["sizes"], 40, 0)
    assert over and lmm.same(got, lmm.local(w["state"], T, w["sizes"], 40, 0)[:4096])
    # ones-65x63: exactly as many entries as it holds (4095 cells, the centre twice)
    w = lmm.world("ones-65x63")
    T = lmm.ones_pose(65, 63)
    got, over = lmm.local_device(w["state"], T, w["sizes"], 40, 0)
    assert not over and got.shape[0] == 4096 == len(w["state"]["keys"]) + 1 and lmm.same(got, lmm.local(w["state"], T, w["sizes"], 40, 0))
    # guard: 127 stays under the loop guard, 128 is cut where guard_world says
    w = lmm.world("guard")
    st, sz, T = w["state"], w["sizes"], lmm.GUARD_POSE
    assert lmm.centre_of(T, sz) == (500, 500, 0) and 30 <= len(st["keys"]) <= 48
    keys, cut = lmm.visit_cut(T, sz, 127, 0)
    assert not cut and keys == lmm.visit(T, sz, 127, 0) and len(keys) == 255 * 255 + 1 and len(keys) + 255 < lmm.VISIT_MAX
    keys, cut = lmm.visit_cut(T, sz, 128, 0)
    full = lmm.visit(T, sz, 128, 0)
    assert cut and len(full) == 257 * 257 + 1 and keys == full[:len(keys)] and keys[-1] == (626, 375, 0) and full[len(keys)] == (626, 376, 0)
    assert len(keys) + 254 == lmm.VISIT_MAX
    got, over = lmm.local_device(st, T, sz, 128, 0)
    want = lmm.local(st, T, sz, 128, 0)
    assert over and want.shape[0] == len(st["keys"]) + 1 and lmm.same(got, want[:got.shape[0]])
    left_out = want.shape[0] - got.shape[0]
    assert left_out == 10 + 2 + 1          # the cells at x offsets 127 and 128, (126, -124) and (126, 0), the centre's second copy
    got127, over127 = lmm.local_device(st, T, sz, 127, 0)
    assert not over127 and lmm.same(got127, lmm.local(st, T, sz, 127, 0)) and 0 < got127.shape[0] < got.shape[0]


SIZES = [(2.5, 1.5), (1.0, 1.0), (1.5, 1.0), (40.0, 50.0), (3.0, 7.25)]


def translations(size):
    """Both sides of 0, +-0.9, exact integers, cell boundaries and integers +- 1e-9, and a few far values, on one axis."""
    v = {0.0, 0.9, -0.9, 0.5, -0.5, 1e-9, -1e-9, 1000.3, -1000.7, 12345.0, -12345.0}
    for k in range(-4, 5):
        v.update((float(k), k + 1e-9, k - 1e-9, k * size, k * size + 1e-9, k * size - 1e-9, (k + 0.5) * size, 17 * k * size + 0.9))
    return sorted(v)


@pytest.mark.parametrize("sizes", SIZES)
def test_rows_bound_holds_for_every_pose_and_extent(sizes):
    """len(visit) <= nx * nx + nz of map_rows_fit, restated here:
        nx = floor((2 * cells_xy * xy + 2) / floor(xy)) + 1,  nz = floor((2 * cells_z * xy + 2) / floor(z)) + 1
    for cells_xy in 0 .. 16, cells_z in 0 .. 3 and every translation of the grid (x and y over the xy list, z over the z list)."""
    xy, z = sizes
    tx, tz = translations(xy), translations(z)
    worst, worst_wide = (0.0, None), (0.0, None)          # over every extent, and over those with cells_xy >= 1
    for cxy in range(17):
        for cz in range(4):
            nx = np.floor((2.0 * cxy * xy + 2.0) / np.floor(xy)) + 1.0
            nz = np.floor((2.0 * cz * xy + 2.0) / np.floor(z)) + 1.0
            bound = nx * nx + nz
            assert bound == lmm.rows_bound((xy, z, 0.25), cxy, cz)
            most = (0, 0.0, 0.0, 0.0)
            for a, x in enumerate(tx):
                for b, y in enumerate(tx):
                    t = tz[(a + b) % len(tz)]
                    n = lmm.visit_size(lmm.pose([x, y, t]), (xy, z, 0.25), cxy, cz)
                    assert n <= bound, (sizes, cxy, cz, x, y, t, n, bound)
                    most = max(most, (n, x, y, t))
            for t in tz:          # every z with the x, y that fill the square most (the column's count depends on z alone)
                n = lmm.visit_size(lmm.pose([most[1], most[2], t]), (xy, z, 0.25), cxy, cz)
                assert n <= bound, (sizes, cxy, cz, most[1], most[2], t, n, bound)
                most = max(most, (n, most[1], most[2], t))
            rec = (most[0] / bound, (cxy, cz) + most[1:] + (most[0], int(bound)))
            worst = max(worst, rec, key=lambda r: r[0])
            if cxy >= 1:
                worst_wide = max(worst_wide, rec, key=lambda r: r[0])
    for what, w in (("any extent", worst), ("cells_xy >= 1", worst_wide)):
        print("sizes %s, %s: largest share of the map_rows_fit bound used %.3f (cells_xy, cells_z, x, y, z, keys, bound = %s)" % (sizes, what, w[0], w[1]))
    assert 0.0 < worst_wide[0] <= worst[0] <= 1.0
    # a spot check that visit_size is len(visit)
    T = lmm.pose([worst[1][2], worst[1][3], 0.9])
    assert lmm.visit_size(T, (xy, z, 0.25), 5, 2) == len(lmm.visit(T, (xy, z, 0.25), 5, 2))
