"""Designed problems for the pose solve (k_lm_solve): worlds of short straight segments with ONE edge per segment, so that the
number of accepted correspondences C, the validity mask, the number of residuals in Huber's linear branch and the rank of the
normal equations are chosen by the generator instead of falling out of a scene.

NumPy only, seeded, no file I/O.  build(case) returns the map (as window frames), the edge cloud and the designed mask.

The world     n segments of 9 points at 0.1 m spacing; centres on a 4 m lattice (x, y in 4 * [-14, 14], z in 4 * [-2, 2]), every
              centre at range 6.5 .. 59.5 m, so segments are at least 4 - 0.8 = 3.2 m apart and every point lies inside 6 .. 60 m.
              Directions are random unit vectors ('parallel': all along z).  Coordinates are rounded to float32 once, and
              everything else (lines, residuals) is derived from the rounded values.
The map       the segments in generation order, 9 consecutive points each.  It is the start of a stream: it enters the window
              raw, the pose is the identity.  A map larger than one frame's edge capacity is fed as several frames of whole
              segments: a later frame finds no point of an earlier one within 3 m, its solves have no residual, the pose stays
              the identity and the window is the designed map bit for bit (asserted by the tests).
The edges     one point per chosen segment at centre + 0.03 m along the segment + N(0, noise), the first `out` of them moved
              `outmag` metres off their line, all taken into the sensor frame of the case's rigid motion (w: rotation vector,
              t: translation; world = R sensor + t) and rounded to float32.  A residual is the distance to the line times the
              range weight 1.01 - (horizontal range - 3) / 72, so the Huber cases keep their world within 20 m (weight >= 0.77):
              0.4 m off the line is a residual norm of 0.31 or more, Huber's linear branch (> 0.2), asserted at the start pose.
Invalid       edges at unused lattice sites: at least 3.2 m from every map point (asserted: > 3 m), so no five neighbours
              within the 1 m gate in either pass.
The mask      `positions(E, C)`: where in the edge list the C valid edges sit.  With C < E the list always takes, in this order of
              priority, E-1 (the last edge, top bit of the last byte of a Q = 8 mask), 0 and 7 (bits 0 and Q-1 of the first k_knn
              workgroup), 3 (bit Q-1 on lock-step batches, Q = 4), E-8 and E-4 (first query of the last workgroup) and, on the
              8704-edge shape, 2048 .. 2055 (the 257th k_knn workgroup: second round of lm_compact_bits) — then random places.

Cases (CASES, by name; every case pins matches and the (termination, iterations, accepted) of both solves in TRACES, values
recorded from the oracle and proved by tests/test_designed_solves.py on the oracle alone, with margin: the same trace from the
blocks in reversed order and from the product's host-compiled controller):

  group    cases                                                                   what they are for
  count    cN, N in COUNTS: E = C = N                                              share / wave arithmetic at every boundary
  sparse   sN, N in COUNTS (N < 1056): E = 1056, C = N at positions(1056, N)       lm_compact_bits, rows beyond ceil(E/Q)
  big      big_sparse: E = 2100 on the 8704-edge shape, C = 72                     second round of lm_compact_bits
  trace    t_<termination>_<iterations>_<accepted>[_s<solve>]                      every reachable end of the controller
  rank     parallel, c1, c2, s1, s2 (H singular), dup (NN0 == NN1: termination 5)  singular / failed evaluations
  huber    huber0, huber1, huber32, huber64: C = 64, that many residuals > 0.2     the loss's two branches

Terminations: 0 max iterations, 1 parameter tolerance, 2 function tolerance, 3 gradient tolerance, 4 no residuals,
5 evaluation failure.  (6 trust-region radius and 7 invalid steps cannot be reached within four iterations.)
"""
import numpy as np

SMALL = (16, 6, 10)        # (scan_lines, scan_regions, edges_per_region): edge capacity 16 * 6 * 11 = 1056
BIG = (64, 8, 16)          # edge capacity 64 * 8 * 17 = 8704
PREV_FRAMES = 16           # window frames: ten map frames of the 1056-segment world and six scans on top never evict
SEG_PTS = 9
SPACING = 0.1
ALONG = 0.03               # the edge's place on its segment, metres from the centre
HUBER_A = 0.2
COUNTS = (1, 2, 3, 5, 6, 63, 64, 65, 128, 129, 192, 193, 256, 257, 513, 1056)
TERMINATION = {0: "maxit", 1: "ptol", 2: "ftol", 3: "gtol", 4: "nores", 5: "evalfail"}


def edge_capacity(shape):
    return shape[0] * shape[1] * (shape[2] + 1)


def _sites():
    k = np.arange(-14, 15) * 4.0
    z = np.arange(-2, 3) * 4.0
    g = np.stack(np.meshgrid(k, k, z, indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.linalg.norm(g, axis=1)
    return g[(r >= 6.5) & (r <= 59.5)]


SITES = _sites()


def rot(w):
    """Rotation matrix of the rotation vector w (Rodrigues)."""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def xyzi(a):
    out = np.zeros((len(a), 4), np.float32)
    out[:, :3] = np.asarray(a, dtype=np.float64).reshape(-1, 3) + 0.0       # (no -0.0)
    return out


def world(n, seed, parallel=False, reach=60.0):
    """(centres [n, 3], directions [n, 3], map float32 [9 n, 4], spare lattice sites) of a seeded world; reach < 60: centres
    (and spare sites) within that range only, for cases whose rotation would carry a far edge out of its segment's reach."""
    sites = SITES if reach >= 60.0 else SITES[np.linalg.norm(SITES, axis=1) <= reach]
    assert 0 < n <= len(sites) - 64
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(sites))
    cs, spare = sites[perm[:n]], sites[perm[n:]]
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    if parallel:
        dirs[:] = [0.0, 0.0, 1.0]
    k = (np.arange(SEG_PTS) - SEG_PTS // 2) * SPACING
    m = xyzi((cs[:, None, :] + k[None, :, None] * dirs[:, None, :]).reshape(-1, 3))
    return cs, dirs, m, spare


def positions(E, C, seed=0):
    """Sorted places of the C valid edges in a list of E (module docstring: 'The mask')."""
    assert 0 <= C <= E
    if C == E:
        return np.arange(E)
    first = [E - 1, 0, 7, 3, E - 8, E - 4] + (list(range(2048, 2056)) if E > 2056 else [])
    take = []
    for p in first:
        if 0 <= p < E and p not in take and len(take) < C:
            take.append(p)
    rest = np.setdiff1d(np.arange(E), take)
    rng = np.random.default_rng(1000 + seed)
    more = rng.choice(rest, size=C - len(take), replace=False)
    return np.sort(np.concatenate([np.array(take, dtype=np.int64), more])).astype(np.int64)


class Case:
    def __init__(self, name, group, C, E=None, shape=SMALL, seed=0, w=(0.0, 0.0, 0.004), t=(0.05, 0.02, 0.0), noise=0.01, out=0,
                 outmag=0.6, parallel=False, dup=0, n_seg=None, rank=False, huber=None, apply_on_ftol=0, reach=60.0):
        self.name, self.group, self.C, self.E, self.shape, self.seed = name, group, C, C if E is None else E, shape, seed
        self.w, self.t, self.noise, self.out, self.outmag = tuple(w), tuple(t), noise, out, outmag
        self.parallel, self.dup, self.rank, self.huber, self.apply_on_ftol = parallel, dup, rank, huber, apply_on_ftol
        self.n_seg = max(C, 8) if n_seg is None else n_seg
        self.reach = reach

    def __repr__(self):
        return self.name


def build(case, step=0):
    """dict(frames, map, edges, valid, pos, centres, dirs, R, t).  frames: the map as window frames of whole segments;
    edges: float32 [E, 4] in the sensor frame; valid: the designed mask; step > 0: the same world and mask with fresh noise
    and other invalid sites (a static sequence)."""
    cap = edge_capacity(case.shape)
    assert case.E <= cap
    cs, dirs, m, spare = world(case.n_seg, case.seed, case.parallel, case.reach)
    if case.dup:
        # duplicates of the centre points of the first `dup` segments, at the end of the map: the nearest two neighbours of their
        # edges are one point twice, a line of length zero (a non-finite residual: the evaluation fails)
        m = np.concatenate([m, m[SEG_PTS // 2::SEG_PTS][:case.dup]])
    per = (cap // SEG_PTS) * SEG_PTS
    frames = [m[i:i + per] for i in range(0, len(m), per)]
    assert len(frames) + 6 <= PREV_FRAMES
    C, E = case.C, case.E
    rng = np.random.default_rng(7919 * (case.seed + 1) + 104729 * step)
    pw = cs[:C] + ALONG * dirs[:C] + rng.normal(size=(C, 3)) * case.noise
    if case.out:
        n = np.cross(dirs[:case.out], [0.0, 0.0, 1.0]) if not case.parallel else np.cross(dirs[:case.out], [1.0, 0.0, 0.0])
        n /= np.linalg.norm(n, axis=1)[:, None]
        pw[:case.out] += n * case.outmag
    pos = positions(E, C, case.seed)
    allw = np.zeros((E, 3))
    valid = np.zeros(E, dtype=bool)
    valid[pos] = True
    allw[pos] = pw
    n_inv = E - C
    if n_inv:
        pick = (np.arange(n_inv) + 1201 * step) % len(spare)
        inv = spare[pick] + rng.uniform(-0.2, 0.2, size=(n_inv, 3))
        d2 = np.min(((inv[:, None, :] - cs[None, :, :]) ** 2).sum(-1), axis=1) if n_inv * len(cs) < 4e6 else \
            np.array([np.min(((cs - p) ** 2).sum(-1)) for p in inv])
        assert np.sqrt(d2.min()) - 0.4 > 3.0, "an invalid edge is within 3 m of a segment"
        allw[~valid] = inv
    R, t = rot(case.w), np.asarray(case.t, dtype=np.float64)
    edges = xyzi((allw - t) @ R)            # sensor frame: world = R sensor + t
    return dict(frames=frames, map=m, edges=edges, valid=valid, pos=pos, centres=cs, dirs=dirs, R=R, t=t)


STALE_COUNTS = (1056, 5, 0, 1056, 1, 257)


def stale_steps():
    """The static sequence of the stale-state test: the world of 1056 segments, then scans of C = 1056, 5, 0, 1056, 1, 257 edges
    near the first C segments with fresh 5 mm noise each (the same bits twice would put two coincident points into the window:
    a line of length zero), no motion.  E = C, and 64 invalid edges where C = 0: a short scan after a long one leaves the partial
    rows and mask bytes of the long one behind."""
    base = dict(seed=77, w=(0, 0, 0), t=(0, 0, 0), noise=0.005, n_seg=1056)
    return [build(Case("stale%d" % k, "stale", c, E=c if c else 64, **base), step=k) for k, c in enumerate(STALE_COUNTS)]


def blocks_of(edges, local_map, valid, ia, ib):
    """[C, 9] float64 residual blocks (p, a, b) of the accepted correspondences, in edge order."""
    sel = np.nonzero(valid)[0]
    out = np.zeros((len(sel), 9))
    out[:, 0:3] = edges[sel, :3]
    out[:, 3:6] = local_map[ia[sel], :3]
    out[:, 6:9] = local_map[ib[sel], :3]
    return out


def rho1(s):
    """Huber (a = 0.2) rho'(s) of the squared residual norm s."""
    return 1.0 if s <= HUBER_A * HUBER_A else max(HUBER_A / np.sqrt(s), np.finfo(float).tiny)


def normal_matrix(orc, blocks, q, t):
    """sum rho' J^T J over the blocks at (q, t) in float64 with the oracle's autodiff Jacobians, and the number of blocks whose
    residual norm exceeds the Huber threshold there."""
    Hs = np.zeros((6, 6))
    n_lin = 0
    for b in blocks:
        r, J, _ = orc.point2line(q, t, b[0:3], b[3:6], b[6:9])
        s = float(r @ r)
        n_lin += int(np.sqrt(s) > HUBER_A)
        Hs += rho1(s) * (J.T @ J)
    return Hs, n_lin


def trace_of(tr):
    return (int(tr.termination), int(tr.iterations), int(tr.accepted))


def oracle_params(orc, case, knn_mode=1):
    h, r, epr = case.shape
    return orc.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=PREV_FRAMES, knn_mode=knn_mode,
                           lm_apply_step_on_ftol=case.apply_on_ftol)


def oracle_run(orc, case, built=None):
    """The oracle's odometer on the case: map frames, then the edges.  dict(pose, info, matches, traces, blocks (per solve,
    from its own correspondences), window (the map as the oracle held it), queries1, built)."""
    b = build(case) if built is None else built
    od = orc.Odometer(oracle_params(orc, case))
    for f in b["frames"]:
        pose, info = od.step(f)
    assert np.array_equal(pose, [0, 0, 0, 1, 0, 0, 0]), "the map frames moved the pose"
    win = od.window().copy()
    assert np.array_equal(win.view(np.uint32), b["map"].view(np.uint32)), "the window is not the designed map"
    pose, info = od.step(b["edges"])
    queries1 = od.last_queries(1)           # the edges under the pose that solve 0 left, as floats
    blocks = []
    for it in (0, 1):
        v, ia, ib = od.last_corr(it)
        blocks.append(blocks_of(b["edges"], win, v, ia, ib))
    od.close()
    return dict(pose=pose, info=info, matches=[int(info.matches[0]), int(info.matches[1])],
                traces=[trace_of(info.lm[0]), trace_of(info.lm[1])], blocks=blocks, window=win, queries1=queries1, built=b)


def _cases():
    cs = []
    for n in COUNTS:
        cs.append(Case("c%d" % n, "count", n, seed=n, rank=n <= 2))
    for n in COUNTS:
        if n < 1056:
            cs.append(Case("s%d" % n, "sparse", n, E=1056, seed=2000 + n, rank=n <= 2))
    cs.append(Case("big_sparse", "big", 72, E=2100, shape=BIG, seed=31))
    cs.append(Case("parallel", "rank", 64, seed=41, parallel=True, rank=True, w=(0, 0, 0), t=(0.1, 0.0, 0.0)))
    cs.append(Case("dup", "rank", 64, seed=42, dup=4, w=(0, 0, 0), t=(0.1, 0.0, 0.0)))
    for k in (0, 1, 32, 64):
        cs.append(Case("huber%d" % k, "huber", 64, seed=50 + k, out=k, outmag=0.4, huber=k, w=(0, 0, 0), t=(0, 0, 0), reach=20.0))
    cs.extend(TRACE_CASES)
    return cs


# One pinned (C, seed, motion, noise, outliers) per reachable end of the controller; found by a search on the oracle alone
# (C = 6, 16, 64 in turn; C = 1, 2, 3 for the gradient-tolerance and rejected-step ends, which larger problems never reach;
# seeds, four motions, noise 0 .. 0.3 m, outliers) that kept the first candidate whose two traces also come out of the reversed
# block order and of the host-compiled controller.  TRACE_SHOWN says which solve of which case shows a trace.
def _t(name, C, seed, w=(0, 0, 0), t=(0, 0, 0), noise=0.0, out=0, outmag=0.0, reach=60.0, rank=False):
    return Case(name, "trace", C, seed=seed, w=w, t=t, noise=noise, out=out, outmag=outmag, reach=reach, rank=rank)


TRACE_CASES = [
    _t("t_ptol_3_2", 6, 101, w=(0, 0, 0.004), t=(0.05, 0.02, 0), noise=0.001),
    _t("t_ptol_4_3", 6, 102, w=(0, 0, 0.004), t=(0.5, 0.25, 0.1), noise=0.001),
    _t("t_ptol_2_1_s1", 6, 100, w=(0, 0, 0.01), t=(0.05, 0.02, 0), noise=0.001),
    _t("t_ptol_1_0_s1", 6, 102, t=(0.05, 0.02, 0), noise=0.001),
    _t("t_ftol_3_2", 6, 100, noise=0.01),
    _t("t_ftol_2_1", 6, 101, noise=0.001),
    _t("t_ftol_4_3", 6, 100, t=(0.5, 0.25, 0.1), out=3, outmag=0.3),
    _t("t_gtol_1_1", 1, 101, rank=True),
    _t("t_gtol_3_3", 1, 100, t=(0.3, 0, 0), rank=True),
    _t("t_gtol_4_4", 3, 100, t=(0.05, 0.02, 0), noise=0.05),
    _t("t_gtol_0_0_s1", 1, 100, noise=0.001, rank=True),
    _t("t_maxit_4_4", 6, 103, noise=0.1, out=3, outmag=0.8),
    _t("t_maxit_4_3", 3, 303, noise=0.02, out=1, outmag=0.9, reach=20.0, rank=True),
    _t("t_maxit_4_2", 3, 307, t=(0.3, 0, 0), noise=0.3, reach=20.0, rank=True),
    _t("t_maxit_4_1", 3, 305, noise=0.05, out=2, outmag=0.7, reach=20.0, rank=True),
    Case("t_nores", "trace", 0, E=64, seed=60),
]

# every end of the controller that four iterations can reach -> (case, solve) that shows it
TRACE_SHOWN = {
    (1, 2, 1): ("t_ptol_2_1_s1", 1), (1, 1, 0): ("t_ptol_1_0_s1", 1), (1, 3, 2): ("t_ptol_3_2", 0), (1, 4, 3): ("t_ptol_4_3", 0),
    (2, 1, 0): ("t_ftol_3_2", 1), (2, 2, 1): ("t_ftol_2_1", 0), (2, 3, 2): ("t_ftol_3_2", 0), (2, 4, 3): ("t_ftol_4_3", 0),
    (3, 0, 0): ("t_gtol_0_0_s1", 1), (3, 1, 1): ("t_gtol_1_1", 0), (3, 3, 3): ("t_gtol_3_3", 0), (3, 4, 4): ("t_gtol_4_4", 0),
    (0, 4, 4): ("t_maxit_4_4", 0), (0, 4, 1): ("t_maxit_4_1", 0), (0, 4, 2): ("t_maxit_4_2", 0), (0, 4, 3): ("t_maxit_4_3", 0),
    (4, 0, 0): ("t_nores", 0), (5, 0, 0): ("dup", 0),
}

# name -> (matches, trace of solve 0, trace of solve 1); trace = (termination, iterations, accepted)
TRACES = {
    "c1": ([1, 1], (1, 3, 2), (1, 2, 1)), "c2": ([2, 2], (3, 3, 3), (3, 1, 1)), "c3": ([3, 3], (1, 4, 3), (3, 2, 2)),
    "c5": ([5, 5], (2, 3, 2), (2, 1, 0)), "c6": ([6, 6], (2, 3, 2), (2, 1, 0)), "c63": ([63, 63], (1, 3, 2), (2, 1, 0)),
    "c64": ([64, 64], (1, 3, 2), (2, 1, 0)), "c65": ([65, 65], (2, 3, 2), (2, 1, 0)), "c128": ([128, 128], (1, 3, 2), (2, 1, 0)),
    "c129": ([129, 129], (1, 3, 2), (2, 1, 0)), "c192": ([192, 192], (1, 3, 2), (2, 1, 0)), "c193": ([193, 193], (1, 3, 2), (2, 1, 0)),
    "c256": ([256, 256], (1, 3, 2), (2, 1, 0)), "c257": ([257, 257], (1, 3, 2), (2, 1, 0)), "c513": ([513, 513], (1, 3, 2), (2, 1, 0)),
    "c1056": ([1056, 1056], (1, 3, 2), (2, 1, 0)),
    "s1": ([1, 1], (1, 3, 2), (1, 1, 0)), "s2": ([2, 2], (3, 3, 3), (1, 2, 1)), "s3": ([3, 3], (1, 4, 3), (1, 1, 0)),
    "s5": ([5, 5], (2, 3, 2), (2, 1, 0)), "s6": ([6, 6], (2, 3, 2), (2, 1, 0)), "s63": ([63, 63], (1, 3, 2), (2, 1, 0)),
    "s64": ([64, 64], (2, 3, 2), (2, 1, 0)), "s65": ([65, 65], (1, 3, 2), (2, 1, 0)), "s128": ([128, 128], (1, 3, 2), (2, 1, 0)),
    "s129": ([129, 129], (1, 3, 2), (2, 1, 0)), "s192": ([192, 192], (1, 3, 2), (2, 1, 0)), "s193": ([193, 193], (1, 3, 2), (2, 1, 0)),
    "s256": ([256, 256], (1, 3, 2), (2, 1, 0)), "s257": ([257, 257], (1, 3, 2), (2, 1, 0)), "s513": ([513, 513], (1, 3, 2), (2, 1, 0)),
    "big_sparse": ([72, 72], (1, 3, 2), (2, 1, 0)),
    "parallel": ([64, 64], (1, 3, 2), (1, 1, 0)), "dup": ([64, 64], (5, 0, 0), (5, 0, 0)),
    "huber0": ([64, 64], (2, 2, 1), (2, 1, 0)), "huber1": ([64, 64], (2, 3, 2), (2, 1, 0)),
    "huber32": ([64, 64], (0, 4, 4), (2, 3, 2)), "huber64": ([64, 64], (0, 4, 4), (0, 4, 4)),
    "t_ptol_3_2": ([6, 6], (1, 3, 2), (2, 1, 0)), "t_ptol_4_3": ([6, 6], (1, 4, 3), (1, 2, 1)),
    "t_ptol_2_1_s1": ([6, 6], (2, 3, 2), (1, 2, 1)), "t_ptol_1_0_s1": ([6, 6], (1, 3, 2), (1, 1, 0)),
    "t_ftol_3_2": ([6, 6], (2, 3, 2), (2, 1, 0)), "t_ftol_2_1": ([6, 6], (2, 2, 1), (2, 1, 0)), "t_ftol_4_3": ([6, 6], (2, 4, 3), (2, 1, 0)),
    "t_gtol_1_1": ([1, 1], (3, 1, 1), (3, 0, 0)), "t_gtol_3_3": ([1, 1], (3, 3, 3), (3, 0, 0)),
    "t_gtol_4_4": ([3, 3], (3, 4, 4), (1, 3, 2)), "t_gtol_0_0_s1": ([1, 1], (3, 2, 2), (3, 0, 0)),
    "t_maxit_4_4": ([6, 6], (0, 4, 4), (2, 2, 1)),
    # three segments, one or two edges far off their lines or 0.3 m of noise: steps are rejected, and the second pass loses the
    # edges that the first solve left more than 1 m from their segment (stated counts)
    "t_maxit_4_3": ([3, 2], (0, 4, 3), (3, 3, 3)), "t_maxit_4_2": ([3, 1], (0, 4, 2), (1, 3, 2)), "t_maxit_4_1": ([3, 2], (0, 4, 1), (3, 3, 3)),
    "t_nores": ([0, 0], (4, 0, 0), (4, 0, 0)),
}

CASES = {c.name: c for c in _cases()}
