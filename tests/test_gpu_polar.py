"""Polar scans on the device (include/liodom_hip.h, "polar scans"): k_polar_project against the NumPy restatement of its arithmetic
(tests/polarref.py) on designed blobs, and every entry point that takes a blob against the packed entry point fed polarref's
projected cloud on a second handle.  All comparisons are on bits.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import liodom_amd as la
import polarref

pytestmark = pytest.mark.gpu

SCENES = {
    # name: lidar_type, H, W, R, epr, P
    "t0_16x900": (0, 16, 900, 6, 10, 5),
    "t1_16x512": (1, 16, 512, 6, 10, 5),
}


def geom_of(s):
    return la.polar_geometry(s.height, s.width, s.range_bits, s.intensity_bits, s.range_unit, s.beam_origin, s.cos_alt, s.sin_alt,
                             s.cos_baz, s.sin_baz, s.cos_enc, s.sin_enc)


_opened = []


def handle(lt, H, R=6, epr=10, P=5, max_points=None, W=None, S=1, keep=False, **cfg):
    """A handle that the test's end closes, passed or failed (keep: its fixture closes it).  A handle left open by a failed test
    would keep every later handle of the process out of chain mode."""
    g = la.Liodom(la.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P),
                  la.make_config(n_streams=S, max_points=max_points, max_width=W or max(1, max_points // H), **cfg))
    if not keep:
        _opened.append(g)
    return g


@pytest.fixture(autouse=True)
def close_handles():
    yield
    while _opened:
        _opened.pop().close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def info_tuple(i):
    return (i.n_edges, i.map_points, tuple(i.matches), i.status, i.scan_index) + tuple(
        (t.iterations, t.accepted, t.termination, t.initial_cost, t.final_cost) for t in i.lm)


def edges_equal(a, b):
    return (np.array_equal(u32(a["edges"]), u32(b["edges"])) and np.array_equal(a["ring"], b["ring"])
            and np.array_equal(a["idx_in_ring"], b["idx_in_ring"]) and np.array_equal(a["src"], b["src"]))


_scene_cache = {}


def scene(synth, name, K, stream=0):
    """K quantised generator scans of a SCENES row: (polarref.Scan list, projected clouds, blobs).  The tables come from scan 0 of
    data stream 0 — one geometry serves every stream of the sensor model, as one geometry serves a handle."""
    key = (name, K, stream)
    if key not in _scene_cache:
        lt, H, W = SCENES[name][:3]
        cfg = synth.make_cfg(H, W, lt)
        first = polarref.quantise(synth.scan(cfg, 0, 0)[0], H, W, lt)
        tabs = (first.cos_alt, first.sin_alt, first.cos_enc, first.sin_enc)
        qs = [polarref.quantise(synth.scan(cfg, stream, k)[0], H, W, lt, tables=tabs) for k in range(K)]
        clouds = [polarref.project(q) for q in qs]
        for c in clouds:
            c.setflags(write=False)
        _scene_cache[key] = (qs, clouds, [q.blob() for q in qs])
    return _scene_cache[key]


# ---- projection -------------------------------------------------------------------------------------------------------------------
class TestDesignedBlobs:
    """The two handles are the class's, not the module's: they are closed before the tests below run, which need the process's only
    live handle to see chain mode (overlap_modes in liodom_hip.hip)."""

    @pytest.fixture(scope="class")
    def projectors(self):
        """One handle per lidar_type.  Type 0: max_points = 16 x 70 exactly (16 x 33 is below it); type 1: 128 x 33 exactly."""
        hs = {0: handle(0, 16, max_points=16 * 70, keep=True), 1: handle(1, 128, max_points=128 * 33, keep=True)}
        yield hs
        for g in hs.values():
            g.close()

    @pytest.mark.parametrize("name", [r[0] for r in polarref.DESIGNED])
    def test_projection_equals_reference_bitwise(self, projectors, name):
        s = polarref.designed(name)
        g = projectors[s.order]
        g.set_polar_geometry(geom_of(s))
        got = g.project_polar(s.blob())
        ref = polarref.project(s)
        assert got.shape == ref.shape
        bad = np.flatnonzero((u32(got) != u32(ref)).any(axis=1))
        assert bad.size == 0, (name, bad[:8], got[bad[:4]], ref[bad[:4]])
        # a second blob on the same geometry (the staging slots are taken in turn), then the first again
        s2 = polarref.Scan(s.order, s.height, s.width, s.range_bits, s.intensity_bits, s.range_unit, s.beam_origin, s.cos_alt, s.sin_alt,
                           s.cos_baz, s.sin_baz, s.cos_enc, s.sin_enc, s.ticks[::-1], s.counts[::-1], None if s.intensities is None else s.intensities[::-1])
        assert np.array_equal(u32(g.project_polar(s2.blob())), u32(polarref.project(s2)))
        assert np.array_equal(u32(g.project_polar(s.blob())), u32(ref))


def test_projection_of_more_than_one_tile_with_a_ragged_tail(synth):
    """16 x 900 = 14 tiles of 1024 points and a tail of 64; 16 x 512 type 1: whole tiles only."""
    for name in SCENES:
        lt, H, W = SCENES[name][:3]
        qs, clouds, blobs = scene(synth, name, 2)
        g = handle(lt, H, max_points=H * W + 77, W=W)
        g.set_polar_geometry(geom_of(qs[0]))
        for k in range(2):
            assert np.array_equal(u32(g.project_polar(blobs[k])), u32(clouds[k])), (name, k)
        g.close()


# ---- per-scan path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_process_scan_polar_equals_process_scan_on_the_projected_cloud(synth, orc, name):
    lt, H, W, R, epr, P = SCENES[name]
    K = 8
    qs, clouds, blobs = scene(synth, name, K)
    po = orc.make_params(lidar_type=lt, scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, knn_mode=1)
    gp, gx = handle(lt, H, R, epr, P, H * W, W), handle(lt, H, R, epr, P, H * W, W)
    gp.set_polar_geometry(geom_of(qs[0]))
    for k in range(K):
        pose_p, info_p = gp.process_scan_polar(blobs[k], stamp=0.1 * k)
        pose_x, info_x = gx.process_scan(clouds[k], H, W, stamp=0.1 * k)
        ep, ex = gp.get_edges(), gx.get_edges()
        assert edges_equal(ep, ex), k
        assert info_tuple(info_p) == info_tuple(info_x), k
        assert np.array_equal(pose_p, pose_x), k
        o = orc.extract(po, clouds[k], H, W)
        assert np.array_equal(u32(ep["edges"]), u32(o["edges"])) and np.array_equal(ep["ring"], o["ring"]) and np.array_equal(ep["idx_in_ring"], o["idx_in_ring"]), k
        assert info_p.status == 0 and info_p.n_edges > 100
    gp.close(); gx.close()


# ---- ticket path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["scan_buffer", "registered", "pageable"])
def test_ticket_path_equals_per_scan_path(synth, source):
    name = "t0_16x900"
    lt, H, W, R, epr, P = SCENES[name]
    K = 12
    qs, clouds, blobs = scene(synth, name, K)
    g = handle(lt, H, R, epr, P, H * W, W)
    g.set_polar_geometry(geom_of(qs[0]))
    ref = []
    for k in range(K):
        pose, info = g.process_scan_polar(blobs[k])
        ref.append((pose, info_tuple(info), g.get_edges()))
    g.reset()
    assert g.modes()["chain"] == "1"
    L = la.load()
    reg = np.stack(blobs).copy()
    if source == "registered":
        assert L.liodom_pin_host_buffer(reg.ctypes.data_as(C.c_void_p), reg.nbytes) == 0
    try:
        for k in range(K):
            if source == "scan_buffer":
                buf = g.scan_buffer_polar()
                assert buf.shape == (blobs[k].size,)
                buf[:] = blobs[k]
                src = buf
            else:
                src = reg[k]
            t = g.extract_edges_device_polar(src)
            assert t is not None and t.seq != 0
            e = g.wait_edges(t)
            pose, info = g.odometry_step_device(t)
            assert edges_equal(e, ref[k][2]), k
            assert np.array_equal(pose, ref[k][0]), k
            assert info_tuple(info) == ref[k][1], k
        assert g.modes()["chain"] == "1"
    finally:
        if source == "registered":
            L.liodom_unpin_host_buffer(reg.ctypes.data_as(C.c_void_p))
    g.close()


def test_ticket_path_back_pressure(synth):
    name = "t0_16x900"
    lt, H, W, R, epr, P = SCENES[name]
    qs, clouds, blobs = scene(synth, name, 12)
    g = handle(lt, H, R, epr, P, H * W, W)
    g.set_polar_geometry(geom_of(qs[0]))
    tickets = [g.extract_edges_device_polar(blobs[k]) for k in range(3)]
    assert all(t is not None for t in tickets)
    t4 = la.api.EdgeTicket()
    assert g.L.liodom_extract_edges_device_polar(g.h, 0, blobs[3].ctypes.data_as(C.c_void_p), C.byref(t4)) == la.api.ERR_BUSY
    assert g.extract_edges_device_polar(blobs[3]) is None
    # tickets outstanding: no new geometry, no fused scan
    assert g.L.liodom_set_polar_geometry(g.h, C.byref(geom_of(qs[0]))) == la.api.ERR_BUSY
    pose = np.zeros(7)
    assert g.L.liodom_process_scan_polar(g.h, 0, blobs[3].ctypes.data_as(C.c_void_p), 0.0, pose.ctypes.data_as(C.POINTER(C.c_double)), None) == la.api.ERR_BUSY
    p0, _ = g.odometry_step_device(tickets[0])
    t = g.extract_edges_device_polar(blobs[3])          # a consumed ticket frees its slot
    assert t is not None
    poses = [p0] + [g.odometry_step_device(x)[0] for x in tickets[1:] + [t]]
    gx = handle(lt, H, R, epr, P, H * W, W)
    for k in range(4):
        assert np.array_equal(poses[k], gx.process_scan(clouds[k], H, W)[0]), k
    g.close(); gx.close()


# ---- C++ driver ---------------------------------------------------------------------------------------------------------------------
def test_cxx_two_thread_replay_polar_equals_packed_driver(synth):
    name = "t0_16x900"
    lt, H, W, R, epr, P = SCENES[name]
    K = 12
    qs, clouds, blobs = scene(synth, name, K)
    g = handle(lt, H, R, epr, P, H * W, W)
    ref, _, tot_ref = g.two_thread_replay(np.stack(clouds), H * W, H, W, timed_from=2)
    g.reset()
    g.set_polar_geometry(geom_of(qs[0]))
    for depth, fetch, pin in ((1, True, True), (0, False, False)):
        got, secs, tot = g.two_thread_replay_polar(np.stack(blobs), timed_from=2, fetch_edges=fetch, depth=depth, pin=pin)
        assert np.array_equal(got, ref), (depth, fetch, pin)
        assert secs > 0 and tot == (tot_ref if fetch else 0)
        g.reset()
    g.close()


# ---- lock-step --------------------------------------------------------------------------------------------------------------------
def test_lockstep_upload_scan_polar_equals_upload_scan(synth):
    """16 streams, 4 distinct data streams, P + 6 scans: polar uploads, packed uploads of the projected clouds, and a mix of the
    two on one handle give the same pose logs."""
    name = "t0_16x900"
    lt, H, W, R, epr, P = SCENES[name]
    S, D, K = 16, 4, P + 6
    data = [scene(synth, name, K, stream=d) for d in range(D)]
    g = handle(lt, H, R, epr, P, H * W, W, S=S, pose_log_capacity=K + 4)
    g.alloc_resident(2)
    logs = {}
    for mode in ("packed", "polar", "mixed"):
        g.reset()
        for k in range(K):
            slot = k & 1
            for s in range(S):
                qs, clouds, blobs = data[s % D]
                if mode == "polar" or (mode == "mixed" and (s + k) % 2 == 0):
                    g.upload_scan_polar(s, slot, blobs[k])
                else:
                    g.upload_scan(s, slot, clouds[k])
            g.process_resident(slot, H * W, H, W, readback=False)
        g.sync()
        logs[mode] = np.stack([g.pose_log(s, 0, K)[0] for s in range(S)])
        if mode == "packed":
            g.set_polar_geometry(geom_of(data[0][0][0]))
    assert np.array_equal(logs["polar"], logs["packed"])
    assert np.array_equal(logs["mixed"], logs["packed"])
    assert not np.array_equal(logs["packed"][0], logs["packed"][1])      # distinct data streams
    g.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_error_table_and_the_handle_goes_on(synth):
    name = "t0_16x900"
    lt, H, W, R, epr, P = SCENES[name]
    K = 4
    qs, clouds, blobs = scene(synth, name, K)
    g = handle(lt, H, R, epr, P, H * W, W)
    L, h = g.L, g.h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((H * W, 4), np.float32)
    pose = np.zeros(7)
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    p, n, t = C.c_void_p(), C.c_int64(), la.api.EdgeTicket()
    g.alloc_resident(1)
    UNS, INV, CAP = la.api.ERR_UNSUPPORTED, la.api.ERR_INVALID_ARG, la.api.ERR_CAPACITY
    # every polar call before a geometry is set
    assert L.liodom_project_polar(h, vp(blobs[0]), out.ctypes.data_as(C.POINTER(C.c_float))) == UNS
    assert L.liodom_upload_scan_polar(h, 0, 0, vp(blobs[0])) == UNS
    assert L.liodom_process_scan_polar(h, 0, vp(blobs[0]), 0.0, dp, None) == UNS
    assert L.liodom_scan_buffer_polar(h, 0, C.byref(p), C.byref(n)) == UNS
    assert L.liodom_extract_edges_device_polar(h, 0, vp(blobs[0]), C.byref(t)) == UNS
    good = geom_of(qs[0])

    def variant(**kw):
        v = geom_of(qs[0])
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    null = C.POINTER(C.c_float)()
    bad = [variant(height=H + 1)]                                                    # H W > max_points
    assert L.liodom_set_polar_geometry(h, C.byref(bad[0])) == CAP
    for kw in ([dict(**{tab: null}) for tab in ("cos_alt", "sin_alt", "cos_baz", "sin_baz", "cos_enc", "sin_enc")]
               + [dict(range_bits=8), dict(range_bits=24), dict(intensity_bits=4), dict(intensity_bits=32), dict(ticks=0), dict(ticks=-3),
                  dict(height=0), dict(width=0), dict(height=-1), dict(width=-5)]):
        assert L.liodom_set_polar_geometry(h, C.byref(variant(**kw))) == INV, kw
    assert L.liodom_set_polar_geometry(h, None) == INV
    # still no geometry after the refused ones
    assert L.liodom_process_scan_polar(h, 0, vp(blobs[0]), 0.0, dp, None) == UNS
    g.set_polar_geometry(good)
    assert L.liodom_process_scan_polar(h, 0, None, 0.0, dp, None) == INV
    # a refused replacement leaves the geometry that was set
    assert L.liodom_set_polar_geometry(h, C.byref(variant(range_bits=8))) == INV
    assert L.liodom_set_polar_geometry(h, C.byref(bad[0])) == CAP
    # a handle with more than one stream has no ticket path
    g2 = handle(lt, H, R, epr, P, H * W, W, S=2)
    g2.set_polar_geometry(good)
    assert g2.L.liodom_extract_edges_device_polar(g2.h, 0, vp(blobs[0]), C.byref(t)) == UNS
    g2.close()
    gx = handle(lt, H, R, epr, P, H * W, W)
    for k in range(K):
        pp, ip = g.process_scan_polar(blobs[k])
        px, ix = gx.process_scan(clouds[k], H, W)
        assert np.array_equal(pp, px) and info_tuple(ip) == info_tuple(ix), k
    # replacing the geometry (another width of the numbers) keeps the handle going
    q32 = polarref.quantise(clouds[0], H, W, lt, range_bits=32, intensity_bits=16, tables=(qs[0].cos_alt, qs[0].sin_alt, qs[0].cos_enc, qs[0].sin_enc))
    g.set_polar_geometry(geom_of(q32))
    assert np.array_equal(u32(g.project_polar(q32.blob())), u32(polarref.project(q32)))
    g.close(); gx.close()
