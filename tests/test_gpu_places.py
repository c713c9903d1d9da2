"""The place database on the GPU (liodom_places_*; kernels_places.h): descriptors, distances, shifts and ranks are EQUAL to the NumPy
model's (tests/place_model.py), blobs are compared byte for byte with the ones api.build_place_state writes, and a scan is
relocalised without a guess on the project's circle.  The designed clouds and databases are those of place_designed.py."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import place_designed as pd
import place_model as pm

pytestmark = pytest.mark.gpu
U64P = C.POINTER(C.c_uint64)


def _db(geom, max_places=64, max_edges=pd.MAX_EDGES):
    return la.Places(max_places=max_places, max_edges=max_edges, n_rings=geom[0], n_layers=geom[1], r_max=geom[2], z_min=geom[3], z_max=geom[4])


def _model_rows(clouds, geom):
    d = [pm.describe(c, geom) for c in clouds]
    return np.stack([a for a, _ in d]), np.array([b for _, b in d], np.int32)


def _same_matches(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------
# describe
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pd.GEOMETRIES))
def test_describe_single_points_on_every_edge_of_a_comparison(name):
    """One point per row: a tangent, an axis, a ring or layer boundary, or a float beside one; non-finite coordinates."""
    geom = pd.GEOMETRIES[name]
    db = _db(geom)
    pts = pd.single_points(geom)
    clouds = [np.array([p + (1.0,)], np.float32) for _, p in pts]
    assert len(clouds) > 250
    desc, bits = db.describe(clouds)
    want, want_bits = _model_rows(clouds, geom)
    bad = [pts[i][0] for i in range(len(pts)) if not np.array_equal(desc[i], want[i]) or bits[i] != want_bits[i]]
    assert not bad, bad[:10]
    assert 0 < int(want_bits.sum()) < len(pts)          # some points set a bit, some are dropped
    db.close()


@pytest.mark.parametrize("name", list(pd.GEOMETRIES))
def test_describe_clouds_of_every_size_and_shape(name):
    geom = pd.GEOMETRIES[name]
    W = pm.words(geom)
    db = _db(geom)
    # every edge count in one batch, at the stride of the largest row (max_edges)
    clouds = [pd.random_cloud(geom, n, 100 + n) for n in pd.N_EDGES_CASES + (pd.MAX_EDGES,)]
    desc, bits = db.describe(clouds)
    want, want_bits = _model_rows(clouds, geom)
    assert np.array_equal(desc, want) and np.array_equal(bits, want_bits)
    assert not desc[0].any() and bits[0] == 0 and bits[-1] > bits[1]
    # all points in one bit; one point per bit
    desc, bits = db.describe([pd.all_in_one_bit(geom), pd.one_point_per_bit(geom)])
    assert bits[0] == 1 and desc[0][W - 1] == np.uint64(1 << 37) and not desc[0][:W - 1].any()
    assert bits[1] == 64 * W and (desc[1] == pm.ALL).all()
    # batches of 1, 2 and 5 rows, a stride above every n_edges, an empty row between full ones
    for rows in ([300], [257, 64], [255, 0, 256, 0, 1]):
        clouds = [pd.random_cloud(geom, n, 7 * n + len(rows)) for n in rows]
        stride = 301
        packed = np.full((len(rows), stride, 4), np.nan, np.float32)      # what lies beyond n_edges is never read as a point
        for i, c in enumerate(clouds):
            packed[i, :len(c)] = c
        packed[:, -1] = pd.bin_centre(geom, 0, 0, 5)
        counts = np.array(rows, np.int32)
        desc, bits = np.zeros((len(rows), W), np.uint64), np.zeros(len(rows), np.int32)
        db._chk(db._L.liodom_places_describe(db.h, api._fp(packed), stride, api._ip(counts), len(rows), desc.ctypes.data_as(U64P), api._ip(bits)))
        want, want_bits = _model_rows(clouds, geom)
        assert np.array_equal(desc, want) and np.array_equal(bits, want_bits), rows
    db.close()


def test_describe_argument_errors_compute_nothing():
    db = _db(pm.DEFAULT, max_edges=16)
    e = np.zeros((2, 20, 4), np.float32)
    desc = np.full((2, 64), 7, np.uint64)
    for counts, stride, n in (([17, 1], 20, 2), ([1, -1], 20, 2), ([5, 1], 4, 2), ([1, 1], -1, 2), ([1, 1], 20, -1)):
        c = np.array(counts, np.int32)
        assert db._L.liodom_places_describe(db.h, api._fp(e), stride, api._ip(c), n, desc.ctypes.data_as(U64P), None) == api.ERR_INVALID_ARG
    assert db._L.liodom_places_describe(db.h, None, 20, api._ip(np.array([1, 1], np.int32)), 2, desc.ctypes.data_as(U64P), None) == api.ERR_INVALID_ARG
    assert (desc == 7).all()
    out = np.zeros((2, 1), api.PLACE_MATCH_DTYPE)
    c = np.array([1, 1], np.int32)
    for k in (0, 17, -1):
        assert db._L.liodom_places_query(db.h, api._fp(e), 20, api._ip(c), 2, k, out.ctypes.data_as(C.c_void_p), None) == api.ERR_INVALID_ARG
    assert db.describe([])[0].shape == (0, 64)           # n = 0 is no error
    db.close()


# ---------------------------------------------------------------------------------------------
# match (through query_desc; the places are written by import_state)
# ---------------------------------------------------------------------------------------------
def _filled(geom, desc, max_places=None):
    n = len(desc)
    ids, poses = np.arange(1000, 1000 + n), pd.poses_for(n)
    db = _db(geom, max_places=max(n, 1) if max_places is None else max_places)
    blob = api.build_place_state(geom, desc, ids, poses)
    db.import_state(blob)
    return db, ids, poses, np.bitwise_count(desc).sum(axis=1).astype(np.int32), blob


def _check_queries(db, queries, desc, ids, poses, bits, k):
    got = db.query_desc(queries, k)
    for i, q in enumerate(queries):
        want = pm.expected_matches(q, desc, k, ids, poses, bits)
        assert _same_matches(got[i], want), (i, got[i][["index", "distance", "shift"]], want[["index", "distance", "shift"]])


@pytest.mark.parametrize("count", [0, 1, 3, 4, 5, 255, 256, 257, 1025])
def test_match_place_counts(count):
    """Around the four places of a workgroup's round, the 1024 threads of the ranking kernel and a wave's 64 lanes; k = 1, 2, 16
    and k above the number of places."""
    geom = pm.DEFAULT if count <= 257 else pd.GEOMETRIES["7x9"]
    W = pm.words(geom)
    rng = np.random.default_rng(count)
    desc = pd.random_desc(rng, count, W)
    db, ids, poses, bits, _ = _filled(geom, desc)
    assert db.count() == count
    queries = np.concatenate([pd.random_desc(rng, 1, W), desc[-1:] if count else pd.random_desc(rng, 1, W)])
    for k in (1, 2, 16):
        _check_queries(db, queries, desc, ids, poses, bits, k)
    got = db.query_desc(queries, 16)
    assert (got["index"][:, min(count, 16):] == -1).all() and (got["index"][:, :min(count, 16)] >= 0).all()
    if count:
        assert got[1, 0]["distance"] == 0 and got[1, 0]["shift"] == 0 and np.array_equal(got[1, 0]["pose"], pm.match_pose(poses[got[1, 0]["index"]], 0))
    db.close()


@pytest.mark.parametrize("name", ["default", "7x9", "1x1"])
def test_match_every_shift_ties_and_periods(name):
    geom = pd.GEOMETRIES[name]
    W = pm.words(geom)
    rng = np.random.default_rng(3)
    q = pd.random_desc(rng, 1, W, density=0.2)[0]
    # a place that is the query rotated by each s: distance 0 at shift s, and the ranking is by index among the 64 ties
    desc = np.stack([pm.rotl(q, s) for s in range(64)])
    db, ids, poses, bits, _ = _filled(geom, desc)
    got = db.query_desc(q[None, :], 16)[0]
    assert list(got["index"]) == list(range(16)) and list(got["shift"]) == list(range(16)) and not got["distance"].any()
    # ... and the query turned back by each s: place 0 (the query itself) is found at every shift in turn
    queries = np.stack([pm.rotl(q, (64 - s) % 64) for s in range(64)])
    assert list(db.query_desc(queries, 1)[:, 0]["shift"]) == list(range(64))
    _check_queries(db, queries, desc, ids, poses, bits, 16)
    db.close()
    # duplicates (the tie goes to the lowest index), all-zero against all-zero (shift 0), periods 32 and 1 (the lowest shift)
    p32, p1 = pd.periodic_desc(rng, W, 32), pd.periodic_desc(rng, W, 1)
    zero = np.zeros(W, np.uint64)
    desc = np.stack([q, p32, q, zero, p1, pm.rotl(p32, 7), zero, pm.rotl(q, 40)])
    db, ids, poses, bits, _ = _filled(geom, desc)
    queries = np.stack([q, zero, pm.rotl(p32, 5), p1, pm.rotl(p32, 39)])
    _check_queries(db, queries, desc, ids, poses, bits, 8)
    got = db.query_desc(queries, 3)
    assert [tuple(int(v) for v in got[0, r][["index", "distance", "shift"]]) for r in range(3)] == [(0, 0, 0), (2, 0, 0), (7, 0, 40)]
    assert tuple(int(v) for v in got[1, 0][["index", "distance", "shift"]]) == (3, 0, 0) and got[1, 1]["index"] == 6
    assert tuple(int(v) for v in got[2, 0][["index", "distance", "shift"]]) == (1, 0, 27)      # 32 - 5, not 59
    assert tuple(int(v) for v in got[3, 0][["index", "distance", "shift"]]) == (4, 0, 0)
    db.close()


@pytest.mark.parametrize("n", [1, 2, 65])
def test_match_query_batches(n):
    geom = pd.GEOMETRIES["7x9"]
    W = pm.words(geom)
    rng = np.random.default_rng(n)
    desc = pd.random_desc(rng, 37, W)
    db, ids, poses, bits, _ = _filled(geom, desc)
    queries = pd.random_desc(rng, n, W)
    queries[n // 2] = pm.rotl(desc[20], 9)
    _check_queries(db, queries, desc, ids, poses, bits, 3)
    db.close()


# ---------------------------------------------------------------------------------------------
# add / state
# ---------------------------------------------------------------------------------------------
def test_add_fill_export_import_reset():
    geom = pd.GEOMETRIES["7x9"]
    W = pm.words(geom)
    clouds = [pd.random_cloud(geom, 200 + 13 * i, 50 + i) for i in range(6)]
    poses, ids = pd.poses_for(6, seed=5), [7, -3, 2 ** 40, 0, 5, 5]
    want_desc, want_bits = _model_rows(clouds, geom)
    db = _db(geom, max_places=5, max_edges=512)
    empty = api.build_place_state(geom, np.zeros((0, W), np.uint64), [], np.zeros((0, 7)))
    assert db.export_state() == empty and db.count() == 0 and db.state_size() == 720
    # a query against a database without places: index -1 rows, and the query's bits all the same
    got, qbits = db.query(clouds[:2], 2, want_bits=True)
    assert (got["index"] == -1).all() and not got["distance"].any() and list(qbits) == list(want_bits[:2])
    for i in range(3):
        assert db.add(clouds[i], poses[i], ids[i]) == i
    # add after query
    got = db.query(clouds[:1], 3)
    assert list(got[0]["index"]) == [0] + sorted([1, 2], key=lambda j: (pm.match(want_desc[0], want_desc[j:j + 1])[0][0], j))
    for i in (3, 4):
        assert db.add(clouds[i], poses[i], ids[i]) == i
    full = api.build_place_state(geom, want_desc[:5], ids[:5], poses[:5])
    assert db.export_state() == full and db.count() == 5
    # one more: LIODOM_ERR_CAPACITY, untouched; so are a pose that is none and a cloud above max_edges
    with pytest.raises(la.LiodomError) as ei:
        db.add(clouds[5], poses[5], ids[5])
    assert ei.value.code == api.ERR_CAPACITY
    for cloud, pose in ((clouds[5], np.array([0, 0, 0, 1.1, 0, 0, 0.0])), (clouds[5], np.array([0, 0, 0, 1, np.nan, 0, 0])), (np.zeros((513, 4), np.float32), poses[5])):
        with pytest.raises(la.LiodomError) as ei:
            db.add(cloud, pose, 1)
        assert ei.value.code == api.ERR_INVALID_ARG
    assert db.export_state() == full and db.count() == 5
    answers = db.query(clouds, 5)
    for i in range(6):
        assert _same_matches(answers[i], pm.expected_matches(want_desc[i], want_desc[:5], 5, ids[:5], poses[:5], want_bits[:5])), i
    # export -> import into a database of another capacity -> the same answers
    other = _db(geom, max_places=9, max_edges=300)
    other.import_state(full)
    assert other.export_state() == full and other.count() == 5
    assert _same_matches(other.query_desc(want_desc, 5), answers)
    assert other.add(clouds[5][:300], poses[5], ids[5]) == 5                       # ... and it goes on working
    assert other.query_desc(pm.describe(clouds[5][:300], geom)[0][None, :], 1)[0, 0]["index"] == 5
    # import into one too small: LIODOM_ERR_CAPACITY, untouched
    small = _db(geom, max_places=4)
    small.add(clouds[0], poses[0], 9)
    before = small.export_state()
    with pytest.raises(la.LiodomError) as ei:
        small.import_state(full)
    assert ei.value.code == api.ERR_CAPACITY and small.export_state() == before
    # malformed blobs, and a blob of another geometry: untouched
    bad_bits = bytearray(full)
    bad_bits[720] ^= 1
    foreign = api.build_place_state(pm.DEFAULT, np.zeros((1, 64), np.uint64), [1], poses[:1])
    for blob in (full[:-1], b"LIODOMMP" + full[8:], bytes(bad_bits), foreign, b""):
        with pytest.raises(la.LiodomError) as ei:
            db.import_state(blob)
        assert ei.value.code == api.ERR_INVALID_ARG
    assert db.export_state() == full and _same_matches(db.query(clouds, 5), answers)
    # export with a buffer too small: the size, nothing written
    buf, need = (C.c_ubyte * 16)(*([0xAB] * 16)), C.c_int64(-1)
    assert db._L.liodom_places_export_state(db.h, buf, 16, C.byref(need)) == api.ERR_CAPACITY and need.value == len(full) and bytes(buf) == b"\xab" * 16
    # reset
    db.reset()
    assert db.count() == 0 and db.export_state() == empty and (db.query_desc(want_desc[:1], 2)["index"] == -1).all()
    assert db.add(clouds[1], poses[1], 4) == 0 and db.query_desc(want_desc[1:2], 1)[0, 0]["index"] == 0
    for d in (db, other, small):
        d.close()


# ---------------------------------------------------------------------------------------------
# the circle
# ---------------------------------------------------------------------------------------------
def test_the_circle_equals_the_model(orc, synth):
    """47 key frames added from their edge clouds, 111 queries: every field of every match equals the model's."""
    run = pm.circle(orc, synth)
    M = pm.circle_model(orc, synth)
    db = la.Places(max_places=64, max_edges=2048)
    ids = [1000 + k for k, _, _ in run["keys"]]
    poses = np.stack([gt for _, _, gt in run["keys"]])
    for (k, e, gt), i in zip(run["keys"], ids):
        db.add(e, gt, i)
    assert db.export_state() == api.build_place_state(pm.DEFAULT, M["desc"], ids, poses)
    got, qbits = db.query([e for _, _, e, _ in run["queries"]], 3, want_bits=True)
    assert np.array_equal(qbits, M["q_bits"])
    for i in range(len(run["queries"])):
        want = pm.expected_matches(M["q_desc"][i], M["desc"], 3, ids, poses, M["bits"])
        assert [(int(a), int(b), int(c)) for a, b, c in zip(want["index"], want["distance"], want["shift"])] == M["top3"][i]
        assert _same_matches(got[i], want), (i, got[i], want)
    db.close()


# ---------------------------------------------------------------------------------------------
# end to end: a scan is found in the site map without a guess
# ---------------------------------------------------------------------------------------------
SITE_SZ, SITE_CELLS = (12.0, 50.0, 0.4), (3, 1)              # the map of test_gpu_map_paging's run
WINDOW = 4
LEVELS = [dict(step_xy=0.4, step_yaw=0.02, nx=8, ny=8, nyaw=7),      # +-3.2 m, +-0.14 rad: a key-frame spacing and a sector and a half
          dict(step_xy=0.1, step_yaw=0.005, nx=4, ny=4, nyaw=4)]     # the fine level of INTEGRATION.md §7
POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4                          # the project's per-scan pose tolerance [m], [rad]


def _rot_angle(qa, qb):
    return 2.0 * np.arccos(min(1.0, abs(float(np.dot(qa, qb)))))


def _cpu_first_scan(orc, po, edges, recv, seed7):
    """localize_model.seeded_first_scan on explicit inputs: two passes of queries under the pose, the oracle's correspondences on
    the received map and its LM solve (the handle's max_range is the solve's), chained."""
    from designed_solves import blocks_of
    q, t = seed7[:4].copy(), seed7[4:].copy()
    for _ in range(2):
        T, _ = orc.pose_ops(q, t)
        v, ia, ib = orc.match_edges(po, recv, orc.transform(T, edges)[:, :3])
        q, t, _ = orc.lm_solve(blocks_of(edges, recv, v, ia, ib), q, t, min_d=3.0, max_d=pm.MAX_RANGE)
    return np.concatenate([q, t])


def test_relocalize_global_on_the_circle(orc, synth):
    from mapper_lag_common import T_of
    run = pm.circle(orc, synth)
    H, W = pm.H, pm.W_SCAN
    m = la.Map(*SITE_SZ, max_cells=512, cell_capacity=4096, max_modified_cells=256)
    for k in range(pm.N_SITE_SCANS):
        m.update(run["edges"][k], T_of(run["gt"][k]))
    assert m.status() == 0
    site = m.export_state()
    g = la.Liodom(la.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, prev_frames=WINDOW, mapping=1, max_range=pm.MAX_RANGE),
                  la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))
    g.attach_map_reader(m, *SITE_CELLS)
    po = orc.make_params(scan_lines=H, scan_regions=pm.REGIONS, edges_per_region=pm.EPR, prev_frames=WINDOW, knn_mode=1, mapping=2, max_range=pm.MAX_RANGE)
    db = la.Places(max_places=64, max_edges=2048)
    state = g.export_stream_state(0)
    # an empty database: None, the stream untouched
    assert g.relocalize_global(m, db, run["scans"][190], H, W, 3, LEVELS, min_fraction=0.3) is None
    assert g.export_stream_state(0) == state
    for k, e, gt in run["keys"]:
        db.add(e, gt, k)
    places = db.export_state()
    # no score reaches a fraction of 1.1: None, the stream untouched
    assert g.relocalize_global(m, db, pm.rot_z(run["scans"][190], 1.0), H, W, 3, LEVELS, min_fraction=1.1) is None
    assert g.export_stream_state(0) == state
    for k, a in ((190, 1.0), (205, 2.5), (222, 1.0)):
        scan = pm.rot_z(run["scans"][k], a)
        true = next(t for kk, aa, _, t in run["queries"] if (kk, aa) == (k, a))
        r = g.relocalize_global(m, db, scan, H, W, 3, LEVELS, min_fraction=0.3)
        assert r is not None and r["n_edges"] > 200
        # by hand: the same query, the same levels around each match's pose
        edges = g.extract_edges(scan, H, W)["edges"]
        matches = db.query([edges], 3)[0]
        assert _same_matches(matches, r["matches"]) and (matches["index"] >= 0).all()
        by_hand = []
        for mt in matches:
            pose = mt["pose"]
            for grid in LEVELS:
                lv = m.search_pose(edges, pose, **grid)
                pose = lv["pose"]
            by_hand.append((lv["hits_r"] + lv["hits_0"], pose, lv))
        best = max(range(3), key=lambda i: (by_hand[i][0], -i))
        assert r["rank"] == best and r["match"]["index"] == matches[best]["index"]
        assert np.array_equal(r["pose"], by_hand[best][1]) and (r["hits_r"], r["hits_0"]) == (by_hand[best][2]["hits_r"], by_hand[best][2]["hits_0"])
        assert [lv["n_candidates"] for lv in r["levels"]] == [17 * 17 * 15, 729]
        d_place = np.linalg.norm(r["match"]["place_pose"][4:] - true[4:])
        print("scan %d turned %.1f: place %d (rank %d, %.2f m off), fraction %.3f, searched pose %.3f m / %.4f rad off the truth"
              % (k, a, r["match"]["id"], r["rank"], d_place, r["fraction"], np.linalg.norm(r["pose"][4:] - true[4:]), _rot_angle(r["pose"][:4], true[:4])))
        assert d_place <= 4.0
        assert np.array_equal(api.parse_stream_state(g.export_stream_state(0))["param_t"], r["pose"][4:])      # seeded
        recv = g.received_map()
        got, info = g.process_scan(scan, H, W)
        assert info.scan_index == 0 and info.status == 0
        own = g.get_edges()["edges"]
        want = _cpu_first_scan(orc, po, own, recv, r["pose"])
        dt, dr = np.linalg.norm(got[4:] - want[4:]), _rot_angle(got[:4], want[:4])
        print("   the scan after the seed: dt %.3e dr %.3e of the CPU chain, %.3f m off the truth" % (dt, dr, np.linalg.norm(got[4:] - true[4:])))
        assert dt <= POSE_TOL_T and dr <= POSE_TOL_R
        assert np.linalg.norm(got[4:] - true[4:]) <= 1.0
        g.reset_stream(0)
    assert m.status() == 0 and m.export_state() == site and db.export_state() == places      # both are only read
    g.attach_mapper(None)
    g.close(); m.close(); db.close()
