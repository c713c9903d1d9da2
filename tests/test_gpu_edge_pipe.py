"""The designed scripts of tests/edge_pipe_cases.py through the public API, on one handle at cfg1_16x900: after every call the return
code and the text of liodom_last_error() are the ones the restatement's verdict stands for, and every collected pose has the bits
liodom_process_scan gives on a second handle.  A polar handle of the same shape plays the scripts that need no resident scans through
the _polar entry points.  (The codes and texts below were taken from, and first checked against, the library before edge_pipe.h.)"""
import ctypes as C

import numpy as np
import pytest

import edge_pipe_cases as ec

pytestmark = pytest.mark.gpu

LT, H, W, R, EPR, P = 0, 16, 900, 6, 10, 5      # cfg1_16x900
K = 8                                           # scans a script may feed between two resets
SLOTS = 4                                       # resident slots the replay steps walk round
OK, INVALID, BUSY, NEEDS_SYNC = 0, -1, -6, -7
TEXT = {
    ("x", "ahead"): (NEEDS_SYNC, "edge extraction by ticket: a pipelined replay of this handle has an extraction issued ahead: call liodom_sync() first"),
    ("x", "replay_live"): (NEEDS_SYNC, "edge extraction by ticket: scans of a pipelined replay (liodom_process_resident / liodom_replay_*) are still in the edge buffers: call liodom_sync() first"),
    ("x", "full"): (BUSY, "edge extraction by ticket: all hand-off slots hold edge clouds no liodom_odometry_step_device has taken yet"),
    ("s", "stale"): (INVALID, "liodom_odometry_submit_device: stale or unknown ticket (already consumed, or voided by liodom_reset)"),
    ("s", "submitted"): (INVALID, "liodom_odometry_submit_device: ticket already submitted"),
    ("s", "two_in_flight"): (BUSY, "liodom_odometry_submit_device: two scans are in flight: collect a pose first (liodom_odometry_collect)"),
    ("c", "none"): (INVALID, "liodom_odometry_collect: no scan has been submitted"),
    ("*", "tickets_out"): (BUSY, "edge tickets of liodom_extract_edges_device are outstanding: consume them with liodom_odometry_step_device first"),
}


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def data(synth):
    """Blobs, their projected clouds, the geometry, and the poses of liodom_process_scan over the clouds on a handle of its own."""
    import liodom_amd as la
    from test_gpu_polar import geom_of, scene
    assert (la.api.ERR_INVALID_ARG, la.api.ERR_BUSY, la.api.ERR_NEEDS_SYNC) == (INVALID, BUSY, NEEDS_SYNC)
    qs, clouds, blobs = scene(synth, "t0_16x900", K)
    g = _handle()
    want = [g.process_scan(clouds[k], H, W)[0] for k in range(K)]
    g.close()
    return dict(clouds=[np.ascontiguousarray(c, np.float32) for c in clouds], blobs=blobs, geom=geom_of(qs[0]), want=want)


def _handle():
    import liodom_amd as la
    return la.Liodom(la.make_params(lidar_type=LT, scan_lines=H, scan_regions=R, edges_per_region=EPR, prev_frames=P),
                     la.make_config(max_points=H * W, max_width=W))


def play(g, data, polar, scripts):
    """Every script from a reset handle.  Returns the number of API calls and of poses compared."""
    import liodom_amd as la
    L, calls, compared = g.L, 0, 0
    for name, text, ticket_only in scripts:
        g.reset()
        m = ec.Model()
        tickets, scan_of = [], []      # tickets given, and the scan each holds
        n_odo, flying = 0, []          # scans that have entered odometry since the reset; tickets submitted and not collected
        waiting = []                   # tickets given since the reset and not submitted
        use_ring = False
        for step, (o, expect) in enumerate(ec.script_ops(text)):
            o = o.replace("s_", "s ")
            where = (name, step, o)
            cur, pf = m.cur, m.pf
            verdict = m.op(o)
            assert verdict.split()[0] == expect, where
            pose, got_pose = np.zeros(7), None
            info = la.api.StepInfo()
            if o == "x":
                k = n_odo + len(waiting)      # the scan behind those that entered odometry and those waiting by ticket
                t = la.api.EdgeTicket()
                if polar:
                    src = data["blobs"][k]
                    if use_ring:      # every second extraction from the handle's page-locked ring, the others from pageable memory
                        src = g.scan_buffer_polar()
                        src[:] = data["blobs"][k]
                    rc = L.liodom_extract_edges_device_polar(g.h, 0, src.ctypes.data_as(C.c_void_p), C.byref(t))
                else:
                    src = data["clouds"][k]
                    if use_ring:
                        src = g.scan_buffer()[:H * W]
                        src[:] = data["clouds"][k]
                    rc = L.liodom_extract_edges_device(g.h, 0, _fp(src), H * W, H, W, C.byref(t))
                use_ring = not use_ring
                if rc == OK:
                    assert verdict == "ok %d %d" % (t.slot, t.seq) and t.stream == 0, (where, verdict, t.slot, t.seq)
                    waiting.append(len(tickets))
                    tickets.append(t)
                    scan_of.append(k)
            elif o[0] == "s":
                j = int(o.split()[1])
                t = tickets[j] if j < len(tickets) else la.api.EdgeTicket()
                rc = L.liodom_odometry_submit_device(g.h, C.byref(t), 0.0)
                if rc == OK:
                    assert scan_of[j] == n_odo, where      # (the scripts submit in the order of extraction)
                    waiting.remove(j)
                    flying.append(j)
                    n_odo += 1
            elif o == "c":
                rc = L.liodom_odometry_collect(g.h, 0, _dp(pose), C.byref(info))
                if rc == OK:
                    got_pose = scan_of[flying.pop(0)]
            elif o in ("r", "ra"):
                slot, nxt = cur % SLOTS, (cur + 1) % SLOTS
                if pf != cur:
                    g.upload_scan(0, slot, data["clouds"][n_odo])
                if o == "ra":
                    g.upload_scan(0, nxt, data["clouds"][n_odo + 1])
                rc = L.liodom_process_resident_pipelined(g.h, slot, nxt if o == "ra" else -1, H * W, H, W, _dp(pose), C.byref(info))
                if rc == OK:
                    got_pose, n_odo = n_odo, n_odo + 1
            elif o == "p":
                if polar:
                    rc = L.liodom_process_scan_polar(g.h, 0, data["blobs"][n_odo].ctypes.data_as(C.c_void_p), 0.0, _dp(pose), C.byref(info))
                else:
                    rc = L.liodom_process_scan(g.h, 0, _fp(data["clouds"][n_odo]), H * W, H, W, 0.0, _dp(pose), C.byref(info))
                if rc == OK:
                    got_pose, n_odo = n_odo, n_odo + 1
            elif o == "y":
                rc = L.liodom_sync(g.h)
            else:
                assert o == "z", o
                rc = L.liodom_reset(g.h)
                n_odo, flying, waiting = 0, [], []
            calls += 1
            err = L.liodom_last_error().decode()
            print(where, verdict, rc, err if rc else "")
            if verdict.startswith("ok"):
                assert rc == OK, (where, rc, err)
            else:
                want_rc, want_text = TEXT.get((o[0], verdict)) or TEXT[("*", verdict)]
                assert (rc, err) == (want_rc, want_text), (where, verdict, rc, err)
            if got_pose is not None:
                assert info.status == 0 and info.scan_index == got_pose, (where, info.status, info.scan_index)
                assert np.array_equal(pose.view(np.uint64), data["want"][got_pose].view(np.uint64)), (where, got_pose)
                compared += 1
    return calls, compared


def _expected(scripts):
    """Calls a list of scripts makes, and the poses it collects: every c, r, ra and p that is to succeed."""
    ops = [op for s in scripts for op in ec.script_ops(s[1])]
    return len(ops), sum(1 for o, v in ops if o in ("c", "r", "ra", "p") and v == "ok")


def test_designed_scripts_through_the_public_api(data):
    g = _handle()
    g.alloc_resident(SLOTS)
    try:
        calls, compared = play(g, data, False, ec.SCRIPTS)
    finally:
        g.close()
    assert (calls, compared) == _expected(ec.SCRIPTS), (calls, compared)


def test_ticket_scripts_through_the_polar_entry_points(data):
    g = _handle()
    try:
        g.set_polar_geometry(data["geom"])
        calls, compared = play(g, data, True, [s for s in ec.SCRIPTS if s[2]])
    finally:
        g.close()
    assert (calls, compared) == _expected([s for s in ec.SCRIPTS if s[2]]), (calls, compared)
