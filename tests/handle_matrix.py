"""The handles whose creation-time decisions are recorded in tests/handle_modes_mi355x.json (tools/record_handle_modes.py) and
replayed by tests/test_handle_plan.py (the plan alone, no GPU) and tests/test_gpu_handle_plan.py (liodom_create on the device).

An entry is (group, name, params, config, switches): keyword arguments of la.make_params / la.make_config and the LIODOM_*
environment switches set while the handle is created.  Clouds are small so that a create takes milliseconds: max_points is
scan_lines x 256 and the window 5 frames unless the entry says otherwise."""
import ctypes as C

# liodom_get_modes keys that only scans change (all zero right after creation) and the probe's own result
RUNTIME_KEYS = ("hash_rebuilds", "hash_appends", "hash_appends_spilled", "hash_points_spilled", "spec_early", "spec_unconfirmed",
                "chain_done", "replay_enqueue_us", "replay_wait_us", "subset_steps")
PROBE_KEY = "streams_concurrent"


def _shape(H, R=8, epr=10, max_points=None, P=5, **params):
    mp = H * 256 if max_points is None else max_points
    return dict(scan_lines=H, scan_regions=R, edges_per_region=epr, prev_frames=P, **params), dict(max_points=mp, max_width=mp // H)


def _entry(group, name, shape, config=None, switches=None):
    p, c = shape
    return (group, name, dict(p), dict(c, **(config or {})), dict(switches or {}))


HDL64 = dict(H=64, max_points=64 * 1800)
S16 = dict(n_streams=16)

MATRIX = [
    # one stream
    _entry("shape", "hdl64", _shape(**HDL64)),
    _entry("shape", "ouster128", _shape(128, max_points=128 * 1024)),                   # overlapped pass off, chain mode on
    _entry("shape", "h128-epr12", _shape(128, epr=12)),                                 # edge capacity 13 312: flag_gate, no chain, no overlap
    _entry("shape", "vlp16", _shape(16)),
    _entry("shape", "h4-r4-epr3", _shape(4, R=4, epr=3)),                               # edge capacity 64, lm_groups 1
    # stream-count switches, H 16
    _entry("shape", "s4", _shape(16), dict(n_streams=4)),
    _entry("shape", "s5", _shape(16), dict(n_streams=5)),
    _entry("shape", "s15", _shape(16), dict(n_streams=15)),
    _entry("shape", "s16", _shape(16), S16),
    _entry("shape", "s256", _shape(16), dict(n_streams=256)),
    _entry("shape", "s16-window4", _shape(16, P=4), S16),                               # hash_incr off
    _entry("shape", "s16-lidar1", _shape(16, lidar_type=1), S16),                       # ring_split_lb off
    # parameter variants, HDL-64
    _entry("params", "mapping", _shape(mapping=1, **HDL64)),
    _entry("params", "mapping-recv1000", _shape(mapping=1, **HDL64), dict(recv_capacity=1000)),
    _entry("params", "filter", _shape(filter_local_map=1, **HDL64)),
    _entry("params", "mapping-filter", _shape(mapping=1, filter_local_map=1, **HDL64)),
    _entry("params", "imu", _shape(use_imu=1, **HDL64)),
    _entry("params", "pose-cov", _shape(**HDL64), dict(pose_covariance=1)),
    _entry("params", "lm3", _shape(**HDL64), dict(lm_workgroups=3)),
    _entry("params", "lm100", _shape(**HDL64), dict(lm_workgroups=100)),
    _entry("params", "lm-1", _shape(**HDL64), dict(lm_workgroups=-1)),
    _entry("params", "debug-buffers", _shape(**HDL64), dict(debug_buffers=1)),
] + [
    # switches, one at a time, on the HDL-64 handle
    _entry("switches", "hdl64 %s=%s" % kv, _shape(**HDL64), None, dict([kv])) for kv in [
        ("LIODOM_SAFE_MODE", "1"), ("LIODOM_PIPE_FLAGS", "0"), ("LIODOM_EARLY_REBUILD", "0"), ("LIODOM_RING_SPLIT", "0"),
        ("LIODOM_KNN_OVERLAP", "0"), ("LIODOM_KNN_OVERLAP", "2"), ("LIODOM_CHAIN", "0"), ("LIODOM_SPECULATE", "0"),
        ("LIODOM_SPECULATE", "2"), ("LIODOM_KNN_SAVE", "0"), ("LIODOM_KNN_SAVE", "1"), ("LIODOM_REBUILD_DELTA", "0.4"),
        ("LIODOM_REBUILD_DELTA", "0.5"), ("LIODOM_HASH_BUILD", "lds")]
] + [
    # ... and on the 16-stream handle
    _entry("switches", "s16 %s=%s" % kv, _shape(16), S16, dict([kv])) for kv in [
        ("LIODOM_SAFE_MODE", "1"), ("LIODOM_HASH_BUILD", "global"), ("LIODOM_KNN8", "0"), ("LIODOM_HASH_INCR", "0"),
        ("LIODOM_RING_SPLIT_LB", "0"), ("LIODOM_LDS_CELLS_MAX", "100"), ("LIODOM_RING_PITCH", "8"), ("LIODOM_HB_SLACK", "0"),
        ("LIODOM_HB_NEW_ROOM", "1")]
]

NAMES = [e[1] for e in MATRIX]
assert len(set(NAMES)) == len(NAMES)


def create(la, entry):
    """The entry's handle; the caller has set the entry's switches (and no other LIODOM_* variable) in the environment."""
    _, _, p, c, _ = entry
    return la.Liodom(la.make_params(**p), la.make_config(**c))


def modes_string(g):
    """liodom_get_modes as the library wrote it."""
    buf = C.create_string_buffer(2048)
    g.L.liodom_get_modes.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    g._check(g.L.liodom_get_modes(g.h, buf, 2048))
    return buf.value.decode()


def parse_modes(s):
    return dict(kv.split("=", 1) for kv in s.split())
