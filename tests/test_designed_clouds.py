"""The designed clouds of tests/designed_clouds.py against the oracle alone (no GPU): every world meets the conditions the GPU
tests rely on, and the oracle's three searches agree on it — brute force (knn_mode 0) = kd-tree (knn_mode 1) on every query,
= plain float64 NumPy brute force on every clearly ordered query.  Run with -s to see the table of the module docstring."""
import numpy as np
import pytest

import designed_clouds as dc

N_Q = 3000
CASES = [(w, o) for w in dc.WORLDS for o in dc.ALL_ORIGINS] + [("dense", None), ("sparse", None)]


def _case_id(c):
    return c[0] if c[1] is None else "%s-%s" % (c[0], dc.origin_id(c[1]))


def oracle_agreement(orc, m, q):
    """valid flags of the brute-force loop; asserts kd-tree = brute force (five neighbours, distances, line points) and
    float64 = float on the clearly ordered queries.  Returns (valid, share left out by the float64 leg)."""
    q4 = np.zeros((len(q), 4), np.float32)
    q4[:, :3] = q[:, :3]
    ib, db = orc.knn5(m, q4, 0)
    ik, dk = orc.knn5(m, q4, 1)
    assert np.array_equal(ib, ik) and np.array_equal(db.view(np.uint32), dk.view(np.uint32))
    vb, ab, bb = orc.match_edges(orc.make_params(knn_mode=0), m, q[:, :3])
    vk, ak, bk = orc.match_edges(orc.make_params(knn_mode=1), m, q[:, :3])
    assert np.array_equal(vb, vk) and np.array_equal(ab, ak) and np.array_equal(bb, bk)
    i64, d64 = dc.neighbours_f64(m, q, k=6)
    clear = dc.clearly_ordered(d64)
    k = min(5, i64.shape[1])
    assert np.array_equal(ib[clear, :k], i64[clear, :k]), "float and float64 neighbours differ on a clearly ordered query"
    return vb, 1.0 - float(clear.mean())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_world_meets_its_conditions(orc, case):
    name, origin = case
    m, q = dc.world(name, origin, N_Q)
    assert len(q) == N_Q and m.dtype == np.float32 and q.dtype == np.float32
    valid, left_out = oracle_agreement(orc, m, q)
    share = float(valid.mean())
    t6, t01 = dc.tie_shares(m, q)
    fifth = dc.fifth_sensitive_share(m, q) if name == "decoys" else float("nan")
    cells = len(np.unique(np.floor(m[:, :3]).astype(np.int64), axis=0))
    print("\n  %-13s %-24s points %6d cells %5d valid %.3f tied6 %.3f tied01 %.3f fifth-sensitive %.3f left out %.3f" % (
        name, "-" if origin is None else dc.origin_id(origin), len(m), cells, share, t6, t01, fifth, left_out))
    assert share >= dc.MIN_VALID[name]
    if name in dc.MIN_TIED:
        assert t6 >= dc.MIN_TIED[name]
    if name == "decoys":
        assert fifth >= dc.MIN_FIFTH_SENSITIVE
    # the float64 leg may leave out at most 5 % of the untied worlds — where a float holds the 1/64 m lattice: on the float
    # grid of the two largest origins every query is a snapped one
    if name in ("poles", "decoys", "dense", "sparse") and (origin is None or dc.lattice_step(origin) == 1.0 / 64.0):
        assert left_out <= dc.MAX_LEFT_OUT
    if name == "dense":
        _, cnt = np.unique(np.floor(m[:, :3]).astype(np.int64), axis=0, return_counts=True)
        assert cnt.max() == 2000 and len(cnt) == 7            # six cells of the four poles + the 512-point run's
        leaves = np.floor(m[:, :3] * (np.float32(1.0) / np.float32(0.4))).astype(np.int64)
        _, lc = np.unique(leaves, axis=0, return_counts=True)
        assert lc.max() > 512 and (lc == 512).any()
    if name == "sparse":
        assert cells > 5000
        _, d5 = orc.knn5(m, np.concatenate([q[:, :3], np.zeros((len(q), 1), np.float32)], axis=1), 0)
        print("  sparse: %d of %d queries within 1e-3 of the gate" % (int((np.abs(d5[:, 4] - 1.0) < 1e-3).sum()), len(q)))


def test_alias_origin_aliases():
    """The second group of poles at ALIAS_ORIGIN lies in cells whose 21-bit keys equal the first group's."""
    m, _ = dc.poles(dc.ALIAS_ORIGIN, 100)
    c = np.floor(m[:, :3].astype(np.float64)).astype(np.int64)
    half = len(c) // 2
    assert np.abs(c[:half, 0]).min() >= 2 ** 20 and np.abs(c[half:, 0]).max() < 2 ** 20
    assert np.array_equal(c[:half, :2] & 0x1FFFFF, c[half:, :2] & 0x1FFFFF)
    assert not np.array_equal(c[:half, :2], c[half:, :2])


def test_gate_edge_sits_on_the_gate(orc):
    m, q, labels = dc.gate_edge()
    q4 = np.zeros((len(q), 4), np.float32)
    q4[:, :3] = q[:, :3]
    idx, d = orc.knn5(m, q4, 0)
    assert np.array_equal(idx, orc.knn5(m, q4, 1)[0])
    valid, _, _ = orc.match_edges(orc.make_params(knn_mode=0), m, q[:, :3])
    seen = set()
    for i, (kind, case) in enumerate(labels):
        assert sorted(idx[i]) == list(range(5 * i, 5 * i + 5)), i              # the group's own five points
        dcell = np.abs(np.floor(m[idx[i, 4], :3]).astype(np.int64) - np.floor(q[i, :3]).astype(np.int64))
        adjacency = GATE_ADJ.get(tuple(sorted(int(v) for v in dcell)))
        if case == "below":
            assert d[i, 4] == np.float32(1.0 - 2.0 ** -23) and valid[i] == 1 and adjacency == kind
        elif case == "exact":
            assert d[i, 4] == np.float32(1.0) and valid[i] == 0 and adjacency == kind
        else:
            assert d[i, 4] > np.float32(1.0) and valid[i] == 0 and dcell.max() == 2
        seen.add((kind, case, bool(q[i, :3].min() < 0)))
    assert len(seen) == 3 * 3 * 2                # each side of the gate for each adjacency kind, on both sides of 0
    print("\n  gate_edge: %d points, %d of %d queries valid" % (len(m), int(valid.sum()), len(q)))


GATE_ADJ = {(0, 0, 1): "face", (0, 1, 1): "edge", (1, 1, 1): "corner"}


def test_few_and_sequence_and_leaf_clouds(orc):
    sizes = [len(m) for m, _ in dc.few()]
    assert sizes == [0, 1, 4, 5, 6]
    for m, q in dc.few():
        v, _, _ = orc.match_edges(orc.make_params(knn_mode=0), m, q[:, :3]) if len(m) else (np.zeros(len(q), np.int32), 0, 0)
        assert (v.sum() > 0) == (len(m) >= 5)
    frames = dc.sequence_frames(dc.ORIGINS[2], 5)
    assert len({len(f) for f in frames}) == 1 and len(frames[0]) == (72 + 4) * 12
    # leaf-aligned cloud: every coordinate is k * 0.4f or the float above it, on both sides of 0
    x = dc.leaf_aligned()
    lf = np.float32(0.4)
    k = np.round(x[:, :3] / lf)
    base = (k.astype(np.float32) * lf).astype(np.float32)
    assert ((x[:, :3] == base) | (x[:, :3] == np.nextafter(base, np.float32(np.inf)))).all()
    assert (k < 0).any() and (k > 0).any() and (k == 0).any()


def test_sequence_world_is_not_vacuous(orc):
    """The sequence world of the GPU test, oracle alone: with the true pose at identity the oracle matches at least half of
    the edges on every scan and both passes, near the origin and 4 km away."""
    P, K = 6, 10
    for origin in (dc.ORIGINS[0], dc.ORIGINS[2]):
        od = orc.Odometer(orc.make_params(scan_lines=64, scan_regions=8, edges_per_region=10, prev_frames=P, knn_mode=1))
        for k, f in enumerate(dc.sequence_frames(origin, K)):
            _, info = od.step(f)
            if k > 0:
                assert min(info.matches) >= len(f) // 2, (origin, k, list(info.matches))
