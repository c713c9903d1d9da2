"""The correspondence search on designed clouds (tests/designed_clouds.py): k_knn<256>, k_knn<128>, k_knn8 + k_knn8_exact and
k_line_gate fed through liodom_odometry_step with clouds at kilometre scale, on cell faces, with exact multi-way ties, with
cells of thousands of points and with fifth neighbours on the distance gate — instead of edge clouds of synthetic scenes.

Bar (the project's): status 0 and (valid, NN0, NN1) of both passes EXACTLY equal to the oracle's loop (laser_odometry.cc:320-361,
brute force) on the GPU's own queries and local map.  On top, the plain high-precision leg: on clearly ordered queries (the six
smallest float64 squared distances pairwise more than 1e-5 relative apart) NN0 and NN1 equal the float64 NumPy neighbours.
The conditions of designed_clouds (valid / tied / fifth-sensitive shares) are asserted on the oracle's output for the GPU's
own first-pass inputs before the GPU's answer is looked at, so that no case passes by being empty.

One handle per (kernel path, mapping) serves every world and origin (liodom_reset between them).  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

import liodom_amd as la
import designed_clouds as dc

pytestmark = pytest.mark.gpu

POSE_TOL_T = 1e-4   # metres
POSE_TOL_R = 1e-4   # radians
N_Q = 400
H, R, EPR, P = 64, 8, 16, 3          # edge capacity 64 * 8 * 17 = 8704 >= 5632: dense() fits one frame
EDGE_CAP = H * R * (EPR + 1)
RECV_CAP = 1 << 17
OTHER_STREAM = 7

# kernel path -> stream count, environment, and what liodom_get_modes must report (liodom_hip.hip: lock-step = 16 streams or
# more).  hash_build of a one-stream handle is "streamed" on the window alone and "global" with a received map.
PATHS = {
    "s1": (1, {}, {"knn_instance": "256", "knn8": "0", "knn_exact_only": "0"}, ("streamed", "global")),
    "s5": (5, {}, {"knn_instance": "256", "knn8": "0", "knn_exact_only": "0"}, ("global", "global")),
    "s16": (16, {}, {"knn_instance": "128", "knn8": "1", "knn_exact_only": "0"}, ("lds", "lds")),
    "s16_knn8off": (16, {"LIODOM_KNN8": "0"}, {"knn_instance": "128", "knn8": "0", "knn_exact_only": "0"}, ("lds", "lds")),
    "s1_exact": (1, {"LIODOM_KNN_EXACT_ONLY": "1"}, {"knn_instance": "256", "knn8": "0", "knn_exact_only": "1"}, ("streamed", "global")),
    "s16_exact": (16, {"LIODOM_KNN_EXACT_ONLY": "1"}, {"knn_instance": "128", "knn8": "1", "knn_exact_only": "1"}, ("lds", "lds")),
}
PLACEMENTS = ("one", "frames", "recv")
CASES = [(w, o) for w in dc.WORLDS for o in dc.ALL_ORIGINS] + [("dense", None), ("sparse", None), ("gate_edge", None), ("few", None)]
TIE_CASES = [(w, o) for w in dc.TIE_WORLDS for o in dc.ALL_ORIGINS]


def _case_id(c):
    return c[0] if c[1] is None else "%s-%s" % (c[0], dc.origin_id(c[1]))


def rot_angle(qa, qb):
    d = abs(float(np.dot(qa, qb)) / (np.linalg.norm(qa) * np.linalg.norm(qb)))
    return 2.0 * np.arccos(min(1.0, d))


class _Env:
    """The LIODOM_* environment of one liodom_create: everything cleared, then `env`; restored afterwards."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: v for k, v in os.environ.items() if k.startswith("LIODOM_")}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)
        os.environ.update(self.saved)


_handles = {}


def open_handle(orc, path, mapping, shape=(H, R, EPR, P)):
    """The handle of (path, mapping, shape), created once; its code paths asserted from liodom_get_modes."""
    key = (path, mapping, shape)
    if key not in _handles:
        S, env, want, hash_build = PATHS[path]
        h, r, epr, p = shape
        with _Env(env):
            g = la.Liodom(la.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=p, mapping=1 if mapping else 0),
                          la.make_config(n_streams=S, max_points=h * 1024, max_width=1024, debug_buffers=1,
                                         recv_capacity=RECV_CAP if mapping else 0))
        modes = g.modes()
        assert modes["n_streams"] == str(S) and modes["mapping"] == ("1" if mapping else "0"), modes
        assert {k: modes[k] for k in want} == want, (path, modes)
        assert modes["hash_build"] == hash_build[1 if mapping else 0], (path, modes)
        po = orc.make_params(scan_lines=h, scan_regions=r, edges_per_region=epr, prev_frames=p, knn_mode=0, mapping=2 if mapping else 0)
        _handles[key] = (g, po, modes)
    g, po, modes = _handles[key]
    g.reset()
    return g, po, modes


def close_handles():
    for g, _, _ in _handles.values():
        g.close()
    _handles.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    close_handles()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_pass(orc, po, g, it, stream, map_g, what, index_of=None):
    """One pass of the last step of `stream` against the oracle's loop and the float64 neighbours, on the GPU's own inputs.
    index_of: what liodom_get_correspondences reports for point i of map_g if not i itself (PCL leaf indices on a filtered map).
    Returns (queries, oracle valid flags, share of the queries the float64 leg left out)."""
    qg = g.knn_queries(it, stream=stream)
    vg, ag, bg = g.correspondences(it, stream=stream)
    vk, ak, bk = orc.match_edges(po, map_g, qg)
    if index_of is not None:
        ak, bk = (np.where(x >= 0, index_of[np.maximum(x, 0)], -1).astype(np.int32) for x in (ak, bk))
    assert np.array_equal(vk, vg) and np.array_equal(ak, ag) and np.array_equal(bk, bg), \
        "%s pass %d: kNN / line gate differ from the oracle on identical inputs at edges %s" % (
            what, it, np.nonzero((vk != vg) | (ak != ag) | (bk != bg))[0][:10])
    if len(map_g) < 2 or len(qg) == 0:
        return qg, vk, 0.0
    i64, d64 = dc.neighbours_f64(map_g, qg, k=6)
    clear = dc.clearly_ordered(d64)
    sel = clear & (vg == 1)
    if index_of is not None:
        i64 = index_of[i64]
    assert np.array_equal(ag[sel], i64[sel, 0]) and np.array_equal(bg[sel], i64[sel, 1]), \
        "%s pass %d: NN0 / NN1 differ from the float64 neighbours on clearly ordered queries %s" % (
            what, it, np.nonzero(sel & ((ag != i64[:, 0]) | (bg != i64[:, 1])))[0][:10])
    return qg, vk, 1.0 - float(clear.mean())


def place(placement, m):
    """(window frames, received map) for one designed map."""
    if placement == "one":
        assert len(m) <= EDGE_CAP
        return [m], None
    if placement == "frames":
        # frame f = the groups (poles, clusters) f, f + P, ... of the map: window index order != generation order.  Groups are
        # more than 1 m apart, so frames 1 .. P-1 find no correspondence in the window, their solves have
        # no residual and the pose stays at the identity: the window is the designed map bit for bit.  (Frames cut ACROSS the
        # poles do match: every solve then slides the new frame along the poles onto the points already there.)
        grp = dc.groups_of(m)
        return [m[grp % P == f] for f in range(P)], None
    n_win = min(4000, len(m) // 4)
    assert len(m) - n_win <= RECV_CAP
    return [m[:n_win]], m[n_win:]


def build_world(name, origin, placement, seed_shift):
    """[(map, queries, label)] of one case; dense / sparse at 10^5 points for the received map, sparse cut to one frame's
    capacity for 'one'."""
    if name in dc.WORLDS:
        return [dc.WORLDS[name](origin, N_Q, seed=11 + seed_shift) + (name,)]
    if name == "dense":
        return [dc.dense(N_Q, seed=5 + seed_shift, pts_per_pole=24000 if placement == "recv" else 2000) + (name,)]
    if name == "sparse":
        n = {"one": 1600, "frames": 3000, "recv": 20000}[placement]
        return [dc.sparse(N_Q, seed=6 + seed_shift, n_clusters=n) + (name,)]
    if name == "gate_edge":
        m, q, _ = dc.gate_edge()
        return [(m, q, name)]
    return [(m, q, "few%d" % len(m)) for m, q in dc.few(seed=8 + seed_shift)]


def run_world(orc, g, po, placement, streams, worlds, name, origin):
    """Steps every stream of `streams` alone (liodom_odometry_step) through its own world: map frames, then the queries."""
    fed = {}
    for s in streams:
        m, q, label = worlds[s]
        frames, recv = place(placement, m)
        for f in frames:
            _, info = g.odometry_step(f, stream=s)
            assert info.status == 0, (label, s, info.status)
        if recv is not None:
            g.set_received_map(recv, stream=s)
        elif placement == "recv":
            g.set_received_map(np.zeros((0, 4), np.float32), stream=s)
        fed[s] = (frames, recv)
    maps = {s: g.local_map(s)[0] for s in streams}
    infos = {}
    for s in streams:
        _, infos[s] = g.odometry_step(worlds[s][1], stream=s)
    for s in streams:
        m, q, label = worlds[s]
        what = "%s %s %s stream %d" % (label, "-" if origin is None else dc.origin_id(origin), placement, s)
        assert infos[s].status == 0, (what, infos[s].status)
        frames, recv = fed[s]
        map_g = maps[s]
        assert len(map_g) == len(m) and infos[s].map_points == len(m), what
        left = [0.0, 0.0]
        q0, v0, left[0] = check_pass(orc, po, g, 0, s, map_g, what)
        # the search ran on the designed points bit for bit; prediction = identity: the first pass's queries are the given edges
        assert same_bits(map_g, np.concatenate(frames + ([recv] if recv is not None else []))), what
        assert same_bits(q0, q[:, :3]), what
        # conditions of the world, on the oracle's output for the first pass's inputs
        if name in dc.MIN_VALID:
            assert float(v0.mean()) >= dc.MIN_VALID[name], (what, float(v0.mean()))
        if name in dc.MIN_TIED:
            assert dc.tie_shares(map_g, q0)[0] >= dc.MIN_TIED[name], what
        if name == "decoys":
            assert dc.fifth_sensitive_share(map_g, q0) >= dc.MIN_FIFTH_SENSITIVE, what
        if name == "few":
            assert (v0.sum() > 0) == (len(m) >= 5), what
        _, _, left[1] = check_pass(orc, po, g, 1, s, map_g, what)
        if name in ("poles", "decoys", "dense", "sparse") and (origin is None or dc.lattice_step(origin) == 1.0 / 64.0):
            assert max(left) <= dc.MAX_LEFT_OUT, (what, left)


def _run(orc, path, placement, case):
    name, origin = case
    g, po, _ = open_handle(orc, path, placement == "recv")
    streams = [0] if PATHS[path][0] < 16 else [0, OTHER_STREAM]
    per_stream = {s: build_world(name, origin, placement, 100 * k) for k, s in enumerate(streams)}
    for i in range(len(per_stream[0])):
        if i:
            g.reset()
        run_world(orc, g, po, placement, streams, {s: per_stream[s][i] for s in streams}, name, origin)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("path", ["s1", "s5", "s16", "s16_knn8off"])
def test_designed_world(orc, path, placement, case):
    """16 streams: stream 0 and stream 7 are stepped alone, each through a world of its own (another seed)."""
    _run(orc, path, placement, case)


@pytest.mark.parametrize("case", TIE_CASES, ids=_case_id)
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("path", ["s1_exact", "s16_exact"])
def test_tie_world_on_the_exact_list_path(orc, path, placement, case):
    """LIODOM_KNN_EXACT_ONLY=1: every query through the sorted (distance, window index) lists."""
    _run(orc, path, placement, case)


# ---------------------------------------------------------------------------------------------
# sequences: appends, evictions, the saved-candidate second pass and the incremental hash on designed data
# ---------------------------------------------------------------------------------------------
SEQ_SHAPE = (16, 8, 10, 6)           # P = 6 > kHbPeriod = 4; edge capacity 1408 >= (72 + 4) * 12 = 912
SEQ_K = 6 + 2 * 4 + 2                # P + 2 * kHbPeriod + 2 frames
SEQ_ORIGINS = dc.ORIGINS[:4]


@pytest.mark.parametrize("origin", SEQ_ORIGINS, ids=dc.origin_id)
@pytest.mark.parametrize("path", ["s1", "s5", "s16", "s16_knn8off"])
def test_designed_sequence(orc, path, origin):
    """SEQ_K frames, each an independent sample of one static pole world (60 % of the poles, 1 cm jitter, four poles of its
    own), true pose identity throughout.  Every scan, both passes: exact comparison as above; the oracle matches at least half
    of the edges.  Near the origin also pose, match counts, LM iterations and terminations against orc.Odometer; far away
    (the rotation has a kilometre lever arm there: no pose bar is derivable) status, correspondences and terminations."""
    close_handles()          # (the overlapped second pass is for a handle that has the GPU to itself: no other live handle)
    g, po, modes = open_handle(orc, path, False, SEQ_SHAPE)
    S = PATHS[path][0]
    near = max(abs(c) for c in origin) < 100.0
    if path == "s16":
        assert modes["hash_incr"] == "1", modes
    if path == "s1":
        assert modes["knn_overlap"] == "1", modes
    streams = [0] if S < 16 else [0, 5]
    frames = {s: dc.sequence_frames(origin, SEQ_K, seed=9 + 50 * k) for k, s in enumerate(streams)}
    pk = orc.make_params(scan_lines=SEQ_SHAPE[0], scan_regions=SEQ_SHAPE[1], edges_per_region=SEQ_SHAPE[2], prev_frames=SEQ_SHAPE[3], knn_mode=1)
    ods = {s: orc.Odometer(pk) for s in streams}
    worst_t = worst_r = 0.0
    for k in range(SEQ_K):
        for s in streams:
            f = frames[s][k]
            what = "%s %s scan %d stream %d" % (path, dc.origin_id(origin), k, s)
            map_g = g.local_map(s)[0]
            pose_g, info = g.odometry_step(f, stream=s)
            pose_o, info_o = ods[s].step(f)
            assert info.status == 0, (what, info.status)
            if k == 0:
                continue
            assert info.map_points == info_o.map_points == len(map_g), what
            for it in (0, 1):
                _, vk, _ = check_pass(orc, po, g, it, s, map_g, what)
                assert int(vk.sum()) >= len(f) // 2 and info.matches[it] == int(vk.sum()), (what, it, int(vk.sum()))
                assert info.lm[it].termination == info_o.lm[it].termination, (what, it)
            dt, dr = float(np.linalg.norm(pose_g[4:] - pose_o[4:])), rot_angle(pose_g[:4], pose_o[:4])
            worst_t, worst_r = max(worst_t, dt), max(worst_r, dr)
            if near:
                assert dt <= POSE_TOL_T and dr <= POSE_TOL_R, (what, dt, dr)
                assert list(info.matches) == list(info_o.matches), what
                assert [info.lm[i].iterations for i in (0, 1)] == [info_o.lm[i].iterations for i in (0, 1)], what
    print("\n  sequence %s %s: GPU - oracle pose difference at most %.3g m, %.3g rad over %d scans" % (
        path, dc.origin_id(origin), worst_t, worst_r, SEQ_K))
    g.sync()
    after = g.modes()
    if path == "s16":
        assert int(after["hash_appends"]) > 0 and int(after["hash_rebuilds"]) > 1, after      # (stream 0's counters)
