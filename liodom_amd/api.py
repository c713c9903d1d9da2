import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "lib", "libliodom_hip.so")
_HASH = _LIB + ".srchash"
_BUILD_INFO = {"rebuilt": None, "source_hash": None}
_SRC = [os.path.join(_HERE, "csrc", f) for f in ("liodom_hip.hip", "liodom_kernels.h", "kernels_extract.h", "kernels_sync.h",
                                                  "kernels_compact.h", "kernels_knn.h", "kernels_knn8.h", "kernels_lm.h", "kernels_rebuild.h",
                                                  "kernels_filter.h", "kernels_cov.h", "kernels_state.h", "stream_state_format.h", "pose7.h", "kernels_polar.h", "kernels_mapper.h", "liodom_math.h", "wave_ops.h",
                                                  "liodom_map.h", "liodom_map_host.h", "map_state_format.h", "kernels_reloc.h", "reloc_candidates.h",
                                                  "kernels_reloc_bnb.h", "reloc_bnb.h", "kernels_map_hits.h", "kernels_register.h", "map_register.h",
                                                  "kernels_places.h", "liodom_places_host.h", "place_state_format.h",
                                                  "kernels_graph.h", "liodom_graph_host.h", "graph_csr.h", "graph_marginals.h", "graph_lm.h",
                                                  "liodom_sizes.h", "handle_plan.h", "step_plan.h", "edge_pipe.h", "map_attach.h", "liodom_step_host.h",
                                                  "odom_edges.h", "kernels_odom_edges.h")] + [
    os.path.join(_ROOT, "include", "liodom_hip.h")]

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-Wno-unused-value"]


class LiodomError(RuntimeError):
    pass


def lib_path():
    return _LIB


def source_hash():
    """SHA-256 over the compile flags and every source the library is built from."""
    h = hashlib.sha256()
    h.update(" ".join(HIPCC_FLAGS).encode())
    for p in _SRC:
        with open(p, "rb") as f:
            h.update(b"\0" + os.path.basename(p).encode() + b"\0" + f.read())
    return h.hexdigest()


def built_hash():
    """Source hash recorded beside the library when it was built ('' if none)."""
    try:
        with open(_HASH) as f:
            return f.read().strip()
    except OSError:
        return ""


def is_stale():
    return not os.path.exists(_LIB) or built_hash() != source_hash()


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU).  The library is
    rebuilt whenever the hash of its sources + flags differs from the one recorded at its last build
    (mtimes do not survive a copy to another box), so a stale binary is never tested against newer
    sources.  Returns the library path; build_info() tells whether this call compiled anything."""
    import fcntl
    os.makedirs(os.path.dirname(_LIB), exist_ok=True)
    with open(_LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)           # several ranks may arrive here at once
        want = source_hash()
        if not force and os.path.exists(_LIB) and built_hash() == want:
            _BUILD_INFO.update(rebuilt=False, source_hash=want)
            return _LIB
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        tmp = _LIB + ".tmp.%d" % os.getpid()
        cmd = [hipcc] + HIPCC_FLAGS + ["-o", tmp, _SRC[0]]
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, _LIB)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        with open(_HASH, "w") as f:
            f.write(want + "\n")
        _BUILD_INFO.update(rebuilt=True, source_hash=want)
    return _LIB


def build_info():
    return dict(_BUILD_INFO)


class Params(C.Structure):
    """liodom_params_t — mirror of liodom::Params (include/liodom/params.h:33-49)."""
    _fields_ = [
        ("min_range", C.c_double), ("max_range", C.c_double),
        ("lidar_type", C.c_int32), ("scan_lines", C.c_int32), ("scan_regions", C.c_int32),
        ("edges_per_region", C.c_int32),
        ("min_points_per_scan", C.c_uint64), ("local_map_size", C.c_uint64),
        ("save_results", C.c_int32),
        ("results_dir", C.c_char * 256), ("fixed_frame", C.c_char * 64), ("base_frame", C.c_char * 64),
        ("laser_frame", C.c_char * 64),
        ("use_imu", C.c_int32), ("filter_local_map", C.c_int32), ("mapping", C.c_int32), ("publish_tf", C.c_int32),
    ]


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("n_streams", C.c_int32), ("max_points", C.c_int32), ("max_width", C.c_int32),
        ("reserved1", C.c_int32), ("lm_apply_step_on_ftol", C.c_int32), ("pose_log_capacity", C.c_int32),
        ("debug_buffers", C.c_int32), ("lm_workgroups", C.c_int32), ("recv_capacity", C.c_int32),
        ("pose_rotation_mode", C.c_int32), ("pose_covariance", C.c_int32),
    ]


class LmTrace(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32), ("pad", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


class StepInfo(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("map_points", C.c_int32), ("matches", C.c_int32 * 2), ("lm", LmTrace * 2),
                ("status", C.c_uint32), ("scan_index", C.c_int32)]


NUM_KERNELS = 12


class PoseCov(C.Structure):
    """liodom_pose_cov_t: the pose covariance record of one scan (include/liodom_hip.h)."""
    _fields_ = [("scan_index", C.c_int32), ("flags", C.c_uint32), ("n_residuals", C.c_int32), ("termination", C.c_int32),
                ("final_cost", C.c_double), ("sigma2", C.c_double), ("information", C.c_double * 36), ("covariance", C.c_double * 36),
                ("eigenvalues", C.c_double * 6), ("eigenvectors", C.c_double * 36)]


COV_VALID, COV_SINGULAR, COV_NO_SOLVE, COV_EVAL_FAILURE, COV_FEW_RESIDUALS = 1, 2, 4, 8, 16


def pose_cov_dict(r):
    """A PoseCov record as NumPy arrays: information / covariance / eigenvectors 6 x 6, eigenvalues (6,), plus the scalars."""
    return dict(scan_index=r.scan_index, flags=r.flags, n_residuals=r.n_residuals, termination=r.termination,
                final_cost=r.final_cost, sigma2=r.sigma2,
                information=np.ctypeslib.as_array(r.information).reshape(6, 6).copy(),
                covariance=np.ctypeslib.as_array(r.covariance).reshape(6, 6).copy(),
                eigenvalues=np.ctypeslib.as_array(r.eigenvalues).copy(),
                eigenvectors=np.ctypeslib.as_array(r.eigenvectors).reshape(6, 6).copy())


class MapConfig(C.Structure):
    """liodom_map_config_t — the mapping node's parameters (liodom_mapping_node.cc:115-125) + capacities."""
    _fields_ = [("device", C.c_int32), ("max_cells", C.c_int32),
                ("voxel_xysize", C.c_double), ("voxel_zsize", C.c_double), ("resolution", C.c_double),
                ("cell_capacity", C.c_int32), ("max_update_points", C.c_int32), ("max_modified_cells", C.c_int32),
                ("reserved", C.c_int32)]


class MapperOptions(C.Structure):
    """liodom_mapper_options_t: how liodom_attach_mapper_ex wires a map to a stream (include/liodom_hip.h)."""
    _fields_ = [("cells_xy", C.c_int32), ("cells_z", C.c_int32), ("lag", C.c_int32), ("prune_period", C.c_int32),
                ("keep_cells_xy", C.c_int32), ("keep_cells_z", C.c_int32), ("reserved", C.c_int32 * 2)]


class PoseSearch(C.Structure):
    """liodom_pose_search_t: the candidate grid of liodom_map_search_pose (include/liodom_hip.h)."""
    _fields_ = [("centre", C.c_double * 7), ("step_xy", C.c_double), ("step_z", C.c_double), ("step_yaw", C.c_double),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("nyaw", C.c_int32), ("radius", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class PoseSearchResult(C.Structure):
    """liodom_pose_search_result_t: the best candidate of liodom_map_search_pose."""
    _fields_ = [("best_index", C.c_int32), ("hits_r", C.c_int32), ("hits_0", C.c_int32), ("n_candidates", C.c_int32),
                ("pose", C.c_double * 7), ("T", C.c_double * 12)]


class PoseSearchBnb(C.Structure):
    """liodom_pose_search_bnb_t: the options of liodom_map_search_pose_bnb."""
    _fields_ = [("batch", C.c_int32), ("reserved", C.c_int32 * 7)]


class PoseSearchStats(C.Structure):
    """liodom_pose_search_stats_t: what a liodom_map_search_pose_bnb call did."""
    _fields_ = [("n_candidates", C.c_int64), ("nodes_bounded", C.c_int64), ("candidates_scored", C.c_int64),
                ("rounds", C.c_int32), ("levels_built", C.c_int32), ("reserved", C.c_int32 * 2)]


class RegisterOptions(C.Structure):
    """liodom_map_register_t: the options of liodom_map_register_poses (include/liodom_hip.h)."""
    _fields_ = [("cells_xy", C.c_int32), ("cells_z", C.c_int32), ("max_passes", C.c_int32), ("min_matches", C.c_int32),
                ("local_capacity", C.c_int32), ("reserved", C.c_int32), ("stop_translation", C.c_double), ("stop_rotation", C.c_double),
                ("min_range", C.c_double), ("max_range", C.c_double)]


class Registration(C.Structure):
    """liodom_map_registration_t: how one start pose of liodom_map_register_poses ended."""
    _fields_ = [("pose", C.c_double * 7), ("information", C.c_double * 36), ("final_cost", C.c_double), ("sigma2", C.c_double),
                ("last_move_t", C.c_double), ("last_move_r", C.c_double), ("termination", C.c_int32), ("passes", C.c_int32),
                ("matches", C.c_int32), ("n_residuals", C.c_int32), ("local_points", C.c_int32), ("cov_flags", C.c_uint32),
                ("last_lm", LmTrace)]


REG_CONVERGED, REG_MAX_PASSES, REG_FEW_MATCHES, REG_NO_MAP, REG_EVAL_FAILURE = 0, 1, 2, 3, 4
REGISTER_ROWS_MAX = 64


def registration_dict(r):
    """A Registration record as NumPy arrays and plain numbers: pose (7,), information 6 x 6, the scalars, last_lm as a dict."""
    return dict(pose=np.array(r.pose[:]), information=np.ctypeslib.as_array(r.information).reshape(6, 6).copy(),
                final_cost=r.final_cost, sigma2=r.sigma2, last_move_t=r.last_move_t, last_move_r=r.last_move_r,
                termination=int(r.termination), passes=int(r.passes), matches=int(r.matches), n_residuals=int(r.n_residuals),
                local_points=int(r.local_points), cov_flags=int(r.cov_flags),
                last_lm=dict(iterations=int(r.last_lm.iterations), accepted=int(r.last_lm.accepted), termination=int(r.last_lm.termination),
                             initial_cost=r.last_lm.initial_cost, final_cost=r.last_lm.final_cost))


class MapHit(C.Structure):
    """liodom_map_hit_t: one scan's map-hit record (liodom_set_map_hits)."""
    _fields_ = [("scan_index", C.c_int32), ("flags", C.c_uint32), ("n_edges", C.c_int32), ("hits_r", C.c_int32), ("hits_0", C.c_int32),
                ("radius", C.c_int32), ("reserved", C.c_int32 * 2), ("T", C.c_double * 12)]


MAP_HIT_DTYPE = np.dtype([("scan_index", "<i4"), ("flags", "<u4"), ("n_edges", "<i4"), ("hits_r", "<i4"), ("hits_0", "<i4"), ("radius", "<i4"),
                          ("reserved", "<i4", (2,)), ("T", "<f8", (3, 4))])
HIT_VALID, HIT_NO_READER, HIT_NO_SOLVE = 1, 2, 4
TRACKING, LOST = "TRACKING", "LOST"


class TrackPolicy:
    """When a map reader counts as lost: the rules of liodom_amd/csrc/track_policy.h, restated (tests/test_track_policy.py holds the
    two equal).  feed() takes one hit record and answers TRACKING or LOST: LOST at the lost_after-th consecutive valid scan whose
    fraction (hits_r + hits_0) / (2 n_edges) is below min_fraction (n_edges = 0 counts as below; a record without HIT_VALID changes
    nothing); the streak starts over with LOST."""

    def __init__(self, min_fraction, lost_after=3):
        self.min_fraction, self.lost_after, self.below = float(min_fraction), int(lost_after), 0

    @staticmethod
    def fraction(hits_r, hits_0, n_edges):
        return (float(hits_r) + float(hits_0)) / (2.0 * float(n_edges)) if n_edges > 0 else 0.0

    def feed(self, hits_r, hits_0, n_edges, flags):
        if not (int(flags) & HIT_VALID):
            return TRACKING
        if n_edges > 0 and self.fraction(hits_r, hits_0, n_edges) >= self.min_fraction:
            self.below = 0
            return TRACKING
        self.below += 1
        if self.below < max(1, self.lost_after):
            return TRACKING
        self.below = 0
        return LOST


class PlaceGeometry(C.Structure):
    """liodom_place_geometry_t: the five numbers of a place descriptor (include/liodom_hip.h)."""
    _fields_ = [("n_rings", C.c_int32), ("n_layers", C.c_int32), ("r_max", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("reserved", C.c_int64)]


class PlaceMatch(C.Structure):
    """liodom_place_match_t: one of the K best places of a query."""
    _fields_ = [("index", C.c_int32), ("distance", C.c_int32), ("shift", C.c_int32), ("bits_place", C.c_int32), ("id", C.c_int64),
                ("pose", C.c_double * 7), ("place_pose", C.c_double * 7)]


PLACE_MATCH_DTYPE = np.dtype([("index", "<i4"), ("distance", "<i4"), ("shift", "<i4"), ("bits_place", "<i4"), ("id", "<i8"),
                              ("pose", "<f8", (7,)), ("place_pose", "<f8", (7,))])


class GraphEdge(C.Structure):
    """liodom_graph_edge_t: "X_i^-1 o X_j was measured as z, with information info" (include/liodom_hip.h "closing loops")."""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32), ("z", C.c_double * 7), ("info", C.c_double * 36)]


GRAPH_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<i4"), ("reserved", "<i4"), ("z", "<f8", (7,)), ("info", "<f8", (6, 6))])
GRAPH_TERMINATIONS = ("gradient", "cost", "max_iterations", "lambda", "breakdown")      # LIODOM_GRAPH_TERM_*


class GraphOptions(C.Structure):
    """liodom_graph_options_t."""
    _fields_ = [("max_iterations", C.c_int32), ("max_pcg_iterations", C.c_int32), ("pcg_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("cost_tolerance", C.c_double)]


class GraphReport(C.Structure):
    """liodom_graph_report_t."""
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("max_gradient", C.c_double), ("final_lambda", C.c_double),
                ("iterations", C.c_int32), ("accepted_steps", C.c_int32), ("pcg_iterations", C.c_int32), ("termination", C.c_int32)]


class GraphCovOptions(C.Structure):
    """liodom_graph_cov_options_t."""
    _fields_ = [("max_pcg_iterations", C.c_int32), ("batch_columns", C.c_int32), ("pcg_tolerance", C.c_double)]


GRAPH_COV_STATUSES = ("ok", "not_converged", "breakdown", "unanchored", "not_pd")      # LIODOM_GRAPH_COV_*
GRAPH_COV_OK, GRAPH_COV_NOT_CONVERGED, GRAPH_COV_BREAKDOWN, GRAPH_COV_UNANCHORED, GRAPH_COV_NOT_PD = range(5)
# liodom_odom_edge_t / liodom_odom_edge_options_t: odometry edges chained from the scans' covariances
ODOM_EDGE_DTYPE = np.dtype([("scan_from", "<i4"), ("scan_to", "<i4"), ("flags", "<u4"), ("n_used", "<i4"), ("n_missing", "<i4"), ("reserved", "<i4"),
                            ("z", "<f8", (7,)), ("covariance", "<f8", (6, 6)), ("information", "<f8", (6, 6))])
ODOM_EDGE_VALID, ODOM_EDGE_GAPS, ODOM_EDGE_NOT_PD, ODOM_EDGE_NO_POSE = 1, 2, 4, 8
ODOM_EDGES_MAX = 1 << 20
POSE_COV_DTYPE = np.dtype([("scan_index", "<i4"), ("flags", "<u4"), ("n_residuals", "<i4"), ("termination", "<i4"), ("final_cost", "<f8"),
                           ("sigma2", "<f8"), ("information", "<f8", (6, 6)), ("covariance", "<f8", (6, 6)), ("eigenvalues", "<f8", (6,)),
                           ("eigenvectors", "<f8", (6, 6))])      # liodom_pose_cov_t as a structured array (944 bytes)


class OdomEdgeOptions(C.Structure):
    _fields_ = [("inflation", C.c_double), ("floor_rotation", C.c_double), ("floor_translation", C.c_double), ("reserved", C.c_int32 * 4)]


GRAPH_COV_STATUS_DTYPE = np.dtype([("iterations", "<i4"), ("status", "<i4"), ("residual", "<f8")])      # liodom_graph_cov_status_t


class PlacePolicy:
    """When a scan becomes a key frame of a place database: the rules of liodom_amd/csrc/place_policy.h, restated
    (tests/test_place_policy.py holds the two equal).  feed(pose7) answers True — and remembers the pose — for the first finite pose
    and for one that has moved from the last key frame's by >= min_dist metres or by a rotation >= min_yaw radians."""

    def __init__(self, min_dist, min_yaw=float("inf")):
        self.min_dist, self.min_yaw, self.last = float(min_dist), float(min_yaw), None

    @staticmethod
    def dist(a, b):
        import math
        dx, dy, dz = a[4] - b[4], a[5] - b[5], a[6] - b[6]
        return math.sqrt(dx * dx + dy * dy + dz * dz)

    @staticmethod
    def angle(a, b):
        import math
        na = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3])
        nb = math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3])
        dot = abs(a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]) / (na * nb)
        return 2.0 * math.acos(dot if dot < 1.0 else 1.0)

    def feed(self, pose7):
        import math
        p = [float(v) for v in np.asarray(pose7, np.float64).reshape(7)]
        if not all(math.isfinite(v) for v in p) or not (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3] > 0.0):
            return False
        if self.last is not None and not (self.dist(p, self.last) >= self.min_dist) and not (self.angle(p, self.last) >= self.min_yaw):
            return False
        self.last = p
        return True


# ---- place-state blob (liodom_places_export_state; layout in csrc/place_state_format.h and DESIGN.md §3) ----
PLACE_STATE_MAGIC = b"LIODOMPL"
PLACE_STATE_VERSION = 1
PLACE_STATE_HEADER_BYTES = 64
PLACE_TABLES_BYTES = 656
PLACE_RECORD_BYTES = 72
PLACE_RECORD_DTYPE = np.dtype([("id", "<i8"), ("bits", "<i4"), ("reserved", "<i4"), ("pose", "<f8", (7,))])


def place_geometry(n_rings=16, n_layers=4, r_max=80.0, z_min=-4.0, z_max=12.0):
    """The five numbers as a tuple (the defaults are liodom_place_geometry_default's)."""
    return (int(n_rings), int(n_layers), float(r_max), float(z_min), float(z_max))


def place_tables(geom):
    """The descriptor's tables as place_state_format.h makes them (double, rounded to float once): dict(C, S (15,), R2 (n_rings,),
    Z (n_layers + 1,)) of float32."""
    import math
    n_rings, n_layers, r_max, z_min, z_max = place_geometry(*geom)
    if not (1 <= n_rings and 1 <= n_layers and n_rings * n_layers <= 64 and math.isfinite(r_max) and math.isfinite(z_min) and
            math.isfinite(z_max) and r_max > 0.0 and z_min < z_max):
        raise ValueError("not a place geometry: 1 <= n_rings * n_layers <= 64, r_max > 0, z_min < z_max, all finite")
    return dict(C=np.array([math.cos(i * math.pi / 32.0) for i in range(1, 16)], np.float64).astype(np.float32),
                S=np.array([math.sin(i * math.pi / 32.0) for i in range(1, 16)], np.float64).astype(np.float32),
                R2=np.array([(i * r_max / n_rings) * (i * r_max / n_rings) for i in range(1, n_rings + 1)], np.float64).astype(np.float32),
                Z=np.array([z_min + i * (z_max - z_min) / n_layers for i in range(n_layers + 1)], np.float64).astype(np.float32))


def _place_tables_bytes(geom):
    t = place_tables(geom)
    raw = np.zeros(PLACE_TABLES_BYTES // 4, "<f4")
    raw[0:15], raw[16:31] = t["C"], t["S"]
    raw[32:32 + len(t["R2"])] = t["R2"]
    raw[96:96 + len(t["Z"])] = t["Z"]
    return raw.tobytes()


def build_place_state(geom, desc, ids, poses, bits=None):
    """Writes a place-state blob: geom = the five numbers, desc [n, W] uint64, ids (n,), poses [n, 7]; bits (n,) defaults to the
    descriptors' popcounts.  The writer the tests fill a database with that needs no describe kernel."""
    g = place_geometry(*geom)
    W = g[0] * g[1]
    tables = _place_tables_bytes(g)
    desc = np.ascontiguousarray(desc, dtype="<u8").reshape(-1, W)
    n = desc.shape[0]
    rec = np.zeros(n, PLACE_RECORD_DTYPE)
    rec["id"] = np.asarray(ids, np.int64).reshape(n)
    rec["pose"] = np.asarray(poses, np.float64).reshape(n, 7)
    rec["bits"] = np.bitwise_count(desc).sum(axis=1) if bits is None else np.asarray(bits, np.int32).reshape(n)
    total = PLACE_STATE_HEADER_BYTES + PLACE_TABLES_BYTES + (8 * W + PLACE_RECORD_BYTES) * n
    blob = b"".join([PLACE_STATE_MAGIC, np.array([PLACE_STATE_VERSION, PLACE_STATE_HEADER_BYTES], "<u4").tobytes(),
                     np.array([total], "<u8").tobytes(), np.array(g[:2], "<i4").tobytes(), np.array(g[2:], "<f8").tobytes(),
                     np.array([n, 0], "<i4").tobytes(), tables, desc.tobytes(), rec.tobytes()])
    assert len(blob) == total
    return blob


def parse_place_state(blob, geom=None):
    """A place-state blob as a dict (pure Python: no library, no GPU).  Keys: version, total_bytes, geometry (the five numbers),
    tables (as place_tables), count, desc [n, W] uint64, bits, ids, poses [n, 7].  Raises ValueError on everything the library's
    place_state_validate rejects as malformed, and — with geom — on a geometry that differs in any bit."""
    b = bytes(blob)
    if len(b) < PLACE_STATE_HEADER_BYTES:
        raise ValueError("place-state blob truncated (%d bytes)" % len(b))
    if b[:8] != PLACE_STATE_MAGIC:
        raise ValueError("not a place-state blob (bad magic)")
    version, header_bytes = (int(x) for x in np.frombuffer(b, "<u4", 2, 8))
    total = int(np.frombuffer(b, "<u8", 1, 16)[0])
    if version != PLACE_STATE_VERSION or header_bytes != PLACE_STATE_HEADER_BYTES:
        raise ValueError("place-state blob of version %d (this code reads %d)" % (version, PLACE_STATE_VERSION))
    if total != len(b):
        raise ValueError("place-state blob says %d bytes, has %d" % (total, len(b)))
    if len(b) < PLACE_STATE_HEADER_BYTES + PLACE_TABLES_BYTES:
        raise ValueError("place-state blob truncated (%d bytes)" % len(b))
    n_rings, n_layers = (int(x) for x in np.frombuffer(b, "<i4", 2, 24))
    r_max, z_min, z_max = (float(x) for x in np.frombuffer(b, "<f8", 3, 32))
    count, reserved = (int(x) for x in np.frombuffer(b, "<i4", 2, 56))
    g = (n_rings, n_layers, r_max, z_min, z_max)
    if n_rings > 64 or n_layers > 64:
        raise ValueError("place-state blob: not a geometry")
    try:
        tables = _place_tables_bytes(g)
    except ValueError:
        raise ValueError("place-state blob: not a geometry")
    if reserved != 0:
        raise ValueError("place-state blob: reserved header word is not 0")
    W = n_rings * n_layers
    rest = len(b) - PLACE_STATE_HEADER_BYTES - PLACE_TABLES_BYTES
    if count < 0 or rest != (8 * W + PLACE_RECORD_BYTES) * count:
        raise ValueError("place-state blob: sizes do not add up")
    if b[PLACE_STATE_HEADER_BYTES:PLACE_STATE_HEADER_BYTES + PLACE_TABLES_BYTES] != tables:
        raise ValueError("place-state blob: the tables are not the ones its geometry gives")
    if geom is not None and (np.array(place_geometry(*geom)[:2], "<i4").tobytes() + np.array(place_geometry(*geom)[2:], "<f8").tobytes()) != b[24:56]:
        raise ValueError("place-state blob comes from a database with another geometry")
    off = PLACE_STATE_HEADER_BYTES + PLACE_TABLES_BYTES
    desc = np.frombuffer(b, "<u8", W * count, off).reshape(count, W).copy()
    rec = np.frombuffer(b, PLACE_RECORD_DTYPE, count, off + 8 * W * count).copy()
    if not np.array_equal(rec["bits"], np.bitwise_count(desc).sum(axis=1).astype(np.int32)):
        raise ValueError("place-state blob: a bit count is not the popcount of its descriptor")
    if (rec["reserved"] != 0).any():
        raise ValueError("place-state blob: reserved record word is not 0")
    with np.errstate(all="ignore"):
        norm = np.sqrt((rec["pose"][:, :4] ** 2).sum(axis=1))
        if not (np.isfinite(rec["pose"]).all() and (np.abs(norm - 1.0) <= 1e-6).all()):
            raise ValueError("place-state blob: a pose is non-finite or its quaternion is not normalised")
    return dict(version=version, total_bytes=total, geometry=g, tables=place_tables(g), count=count, desc=desc, bits=rec["bits"].copy(),
                ids=rec["id"].copy(), poses=rec["pose"].copy())


class EdgeTicket(C.Structure):
    """liodom_edge_ticket_t: an edge cloud left on the device by liodom_extract_edges_device."""
    _fields_ = [("seq", C.c_uint32), ("slot", C.c_int32), ("stream", C.c_int32), ("reserved", C.c_int32)]


ERR_INVALID_ARG = -1
ERR_UNSUPPORTED = -2
ERR_CAPACITY = -3
ERR_BUSY = -6
ERR_NEEDS_SYNC = -7


# ---- stream-state blob (liodom_export_stream_state; layout in csrc/stream_state_format.h and DESIGN.md §3) ----
STATE_MAGIC = b"LIODOMST"
STATE_VERSION = 1
STATE_HEADER_BYTES = 64
STATE_RECORD_BYTES = 416
_STATE_FINGERPRINT = ("local_map_size", "mapping", "filter_local_map", "use_imu", "pose_rotation_mode", "lm_apply_step_on_ftol")


def parse_stream_state(blob):
    """A stream-state blob as a dict of NumPy arrays and scalars (pure Python: no library, no GPU).  Keys: version, total_bytes,
    the six fingerprint parameters, odom / prev_odom / final_odom (3 x 4), param_q, param_t, initialized, append_raw, frame_count,
    n_frames, scan_counter, status, has_imu, imu_q, frame_counts (n_frames,), frames (list of [count, 4] float32 arrays, oldest
    first), window (the frames back to back: what liodom_get_window returns), received_map ([n_recv, 4]).  Raises ValueError on a
    bad magic, version or size."""
    b = bytes(blob)
    if len(b) < STATE_HEADER_BYTES + STATE_RECORD_BYTES:
        raise ValueError("stream-state blob truncated (%d bytes)" % len(b))
    if b[:8] != STATE_MAGIC:
        raise ValueError("not a stream-state blob (bad magic)")
    version, header_bytes = np.frombuffer(b, "<u4", 2, 8)
    total = int(np.frombuffer(b, "<u8", 1, 16)[0])
    if version != STATE_VERSION or header_bytes != STATE_HEADER_BYTES:
        raise ValueError("stream-state blob of version %d (this code reads %d)" % (version, STATE_VERSION))
    if total != len(b):
        raise ValueError("stream-state blob says %d bytes, has %d" % (total, len(b)))
    out = dict(version=int(version), total_bytes=total)
    out.update(zip(_STATE_FINGERPRINT, (int(x) for x in np.frombuffer(b, "<u4", 6, 24))))
    d = np.frombuffer(b, "<f8", 43, STATE_HEADER_BYTES)
    out.update(odom=d[0:12].reshape(3, 4).copy(), prev_odom=d[12:24].reshape(3, 4).copy(), final_odom=d[24:36].reshape(3, 4).copy(),
               param_q=d[36:40].copy(), param_t=d[40:43].copy())
    i = np.frombuffer(b, "<i4", 10, STATE_HEADER_BYTES + 344)
    out.update(initialized=int(i[0]), append_raw=int(i[1]), frame_count=int(i[2]), n_frames=int(i[3]), scan_counter=int(i[4]),
               status=int(np.uint32(i[5])), has_imu=int(i[8]))
    n_points, n_recv = int(i[6]), int(i[7])
    out["imu_q"] = np.frombuffer(b, "<f8", 4, STATE_HEADER_BYTES + 384).copy()
    P = out["local_map_size"]
    off = STATE_HEADER_BYTES + STATE_RECORD_BYTES
    n_counts = (P + 3) // 4 * 4
    pts_off = off + 4 * n_counts
    if out["n_frames"] < 0 or out["n_frames"] > P or n_points < 0 or n_recv < 0 or total != pts_off + 16 * (n_points + n_recv):
        raise ValueError("stream-state blob: sizes do not add up")
    counts = np.frombuffer(b, "<i4", n_counts, off)[:out["n_frames"]].copy()
    if (counts < 0).any() or int(counts.sum()) != n_points:
        raise ValueError("stream-state blob: frame counts do not add up")
    pts = np.frombuffer(b, "<f4", 4 * (n_points + n_recv), pts_off).reshape(-1, 4)
    out["frame_counts"] = counts
    out["window"] = pts[:n_points].copy()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    out["frames"] = [out["window"][starts[j]:starts[j + 1]] for j in range(out["n_frames"])]
    out["received_map"] = pts[n_points:].copy()
    return out


def patch_stream_state(blob, **fields):
    """A copy of a stream-state blob with poses of its record replaced (pure Python): odom, prev_odom, final_odom (3 x 4 or 12),
    param_q (4), param_t (3), imu_q (4; sets has_imu).  Counters, window and fingerprint stay, so liodom_import_stream_state takes
    the result on the handle the blob came from.  For tests and tools that start a stream from a chosen pose state."""
    b = bytearray(bytes(blob))
    parse_stream_state(b)          # (raises on anything that is not a blob)
    where = dict(odom=(0, 12), prev_odom=(96, 12), final_odom=(192, 12), param_q=(288, 4), param_t=(320, 3), imu_q=(384, 4))
    for name, value in fields.items():
        off, n = where[name]       # KeyError: not a patchable field
        a = np.ascontiguousarray(value, dtype="<f8").reshape(-1)
        if a.shape[0] != n:
            raise ValueError("%s takes %d doubles" % (name, n))
        b[STATE_HEADER_BYTES + off:STATE_HEADER_BYTES + off + 8 * n] = a.tobytes()
        if name == "imu_q":
            b[STATE_HEADER_BYTES + 376:STATE_HEADER_BYTES + 380] = np.array([1], "<i4").tobytes()
    return bytes(b)


# ---- map-state blob (liodom_map_export_state; layout in csrc/map_state_format.h and DESIGN.md §3) ----
MAP_STATE_MAGIC = b"LIODOMMP"
MAP_STATE_VERSION = 1
MAP_STATE_HEADER_BYTES = 64
MAP_STATE_RECORD_BYTES = 32
MAP_KEY_LIMIT = 1 << 20


def parse_map_state(blob, sizes=None):
    """A map-state blob as a dict of NumPy arrays and scalars (pure Python: no library, no GPU).  Keys: version, total_bytes,
    voxel_xysize, voxel_zsize, resolution, status, keys [n, 3], corner_leaf [n, 3], counts (n,), points [n_points, 4] (what
    liodom_map_get_all returns) and cells (a list of [count, 4] float32 arrays in creation order).  Raises ValueError on everything
    the library's map_state_validate rejects as malformed, and — with sizes = (voxel_xysize, voxel_zsize, resolution) of the map
    that is to take the blob — on a fingerprint that differs in any bit.  (Capacities are the importing map's to check.)"""
    b = bytes(blob)
    if len(b) < MAP_STATE_HEADER_BYTES:
        raise ValueError("map-state blob truncated (%d bytes)" % len(b))
    if b[:8] != MAP_STATE_MAGIC:
        raise ValueError("not a map-state blob (bad magic)")
    version, header_bytes = (int(x) for x in np.frombuffer(b, "<u4", 2, 8))
    total = int(np.frombuffer(b, "<u8", 1, 16)[0])
    if version != MAP_STATE_VERSION or header_bytes != MAP_STATE_HEADER_BYTES:
        raise ValueError("map-state blob of version %d (this code reads %d)" % (version, MAP_STATE_VERSION))
    if total != len(b):
        raise ValueError("map-state blob says %d bytes, has %d" % (total, len(b)))
    xy, z, res = (float(x) for x in np.frombuffer(b, "<f8", 3, 24))
    if sizes is not None and np.array(sizes, "<f8").tobytes() != b[24:48]:
        raise ValueError("map-state blob comes from a map with other sizes (%r, %r, %r)" % (xy, z, res))
    n_cells = int(np.frombuffer(b, "<i4", 1, 48)[0])
    status = int(np.frombuffer(b, "<u4", 1, 52)[0])
    n_points = int(np.frombuffer(b, "<i8", 1, 56)[0])
    if n_cells < 0 or n_points < 0 or total != MAP_STATE_HEADER_BYTES + MAP_STATE_RECORD_BYTES * n_cells + 16 * n_points:
        raise ValueError("map-state blob: sizes do not add up")
    rec = np.frombuffer(b, "<i4", 8 * n_cells, MAP_STATE_HEADER_BYTES).reshape(n_cells, 8)
    keys, corner, counts, first = rec[:, 0:3].copy(), rec[:, 3:6].copy(), rec[:, 6].copy(), rec[:, 7].copy()
    if (counts < 0).any():
        raise ValueError("map-state blob: negative cell count")
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    if not np.array_equal(first.astype(np.int64), starts[:-1]):
        raise ValueError("map-state blob: first is not the prefix sum of the counts")
    if int(starts[-1]) != n_points:
        raise ValueError("map-state blob: cell counts do not add up to n_points")
    if ((keys < -MAP_KEY_LIMIT) | (keys >= MAP_KEY_LIMIT)).any():
        raise ValueError("map-state blob: cell key beyond +-2^20")
    if n_cells and len(np.unique(keys, axis=0)) != n_cells:
        raise ValueError("map-state blob: duplicate cell key")
    pts = np.frombuffer(b, "<f4", 4 * n_points, MAP_STATE_HEADER_BYTES + MAP_STATE_RECORD_BYTES * n_cells).reshape(n_points, 4).copy()
    return dict(version=version, total_bytes=total, voxel_xysize=xy, voxel_zsize=z, resolution=res, status=status, keys=keys,
                corner_leaf=corner, counts=counts, points=pts,
                cells=[pts[int(starts[c]):int(starts[c + 1])] for c in range(n_cells)])


def map_cell_key(xyz, xy, z):
    """The reference's coarse-cell key of a float32 point (map.cc:103-105): int(floor(x * inv) * size + size / 2) in FP64."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    out = []
    for a, size in enumerate((xy, xy, z)):
        size = float(size)
        out.append(int(np.floor(p[a] * (1.0 / size)) * size + size / 2.0))      # int(): truncation, as the C cast
    return out


def map_cell_corner_leaf(xyz, xy, z, res):
    """Leaf coordinates of the lower corner of the coarse cell of a float32 point, with the float arithmetic of k_map_assign:
    floorf(float(floor(x * inv) * size) * leaf_inv), leaf_inv = 1.0f / float(resolution)."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    leaf_inv = np.float32(1.0) / np.float32(res)
    out = []
    for a, size in enumerate((xy, xy, z)):
        size = float(size)
        out.append(int(np.floor(np.float32(np.floor(p[a] * (1.0 / size)) * size) * leaf_inv)))
    return out


def build_map_state(xy, z, res, cells, status=0):
    """Writes a map-state blob from `cells`, a list of [count, 4] float32 arrays in creation order (count >= 1): the key of a
    cell comes from its first point with the reference's formula, corner_leaf with the float arithmetic of k_map_assign.  The
    writer the tests design maps with that no sequence of updates is needed for; it does not check that the points of a cell
    share its key or hold one point per leaf."""
    cells = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in cells]
    counts = [c.shape[0] for c in cells]
    if any(n < 1 for n in counts):
        raise ValueError("build_map_state: a cell needs at least one point (its key comes from the first)")
    n_points = int(sum(counts))
    total = MAP_STATE_HEADER_BYTES + MAP_STATE_RECORD_BYTES * len(cells) + 16 * n_points
    out = [MAP_STATE_MAGIC, np.array([MAP_STATE_VERSION, MAP_STATE_HEADER_BYTES], "<u4").tobytes(), np.array([total], "<u8").tobytes(),
           np.array([xy, z, res], "<f8").tobytes(), np.array([len(cells)], "<i4").tobytes(), np.array([status], "<u4").tobytes(),
           np.array([n_points], "<i8").tobytes()]
    first = 0
    for c in cells:
        out.append(np.array(map_cell_key(c[0, :3], xy, z) + map_cell_corner_leaf(c[0, :3], xy, z, res) + [c.shape[0], first], "<i4").tobytes())
        first += c.shape[0]
    out.extend(c.astype("<f4").tobytes() for c in cells)
    blob = b"".join(out)
    assert len(blob) == total
    return blob


def join_map_state(xy, z, res, keys, corner_leaf, cells, status=0):
    """Writes a map-state blob from records as parse_map_state returns them: keys [n, 3], corner_leaf [n, 3] and cells, a list of
    [count, 4] float32 arrays, in the order given.  Unlike build_map_state nothing is derived from the points: corner_leaf cannot
    be (map_state_format.h), so a store of cells has to keep it.  Cells may be empty."""
    cells = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in cells]
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    corner = np.asarray(corner_leaf, np.int64).reshape(-1, 3)
    if not (len(keys) == len(corner) == len(cells)):
        raise ValueError("join_map_state: keys, corner_leaf and cells differ in length")
    counts = np.array([c.shape[0] for c in cells], np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])
    n_points = int(first[-1])
    total = MAP_STATE_HEADER_BYTES + MAP_STATE_RECORD_BYTES * len(cells) + 16 * n_points
    rec = np.zeros((len(cells), 8), "<i4")
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7] = keys, corner, counts, first[:-1]
    out = [MAP_STATE_MAGIC, np.array([MAP_STATE_VERSION, MAP_STATE_HEADER_BYTES], "<u4").tobytes(), np.array([total], "<u8").tobytes(),
           np.array([xy, z, res], "<f8").tobytes(), np.array([len(cells)], "<i4").tobytes(), np.array([status], "<u4").tobytes(),
           np.array([n_points], "<i8").tobytes(), rec.tobytes()]
    out.extend(c.astype("<f4").tobytes() for c in cells)
    blob = b"".join(out)
    assert len(blob) == total
    return blob


class PolarGeometry(C.Structure):
    """liodom_polar_geometry_t: a polar scan's shape, number widths and tables (include/liodom_hip.h)."""
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("range_bits", C.c_int32), ("intensity_bits", C.c_int32),
                ("range_unit", C.c_float), ("beam_origin", C.c_float),
                ("cos_alt", C.POINTER(C.c_float)), ("sin_alt", C.POINTER(C.c_float)),
                ("cos_baz", C.POINTER(C.c_float)), ("sin_baz", C.POINTER(C.c_float)),
                ("ticks", C.c_int32), ("reserved", C.c_int32),
                ("cos_enc", C.POINTER(C.c_float)), ("sin_enc", C.POINTER(C.c_float))]


class PolarLayout(C.Structure):
    _fields_ = [("tick_offset", C.c_int64), ("range_offset", C.c_int64), ("intensity_offset", C.c_int64), ("total_bytes", C.c_int64)]


_POLAR_TABLES = ("cos_alt", "sin_alt", "cos_baz", "sin_baz", "cos_enc", "sin_enc")


def polar_geometry(height, width, range_bits, intensity_bits, range_unit, beam_origin, cos_alt, sin_alt, cos_baz, sin_baz,
                   cos_enc, sin_enc):
    """A PolarGeometry from float32 tables ([height] x 4, [ticks] x 2).  The arrays are kept alive by the returned object (.tables)."""
    g = PolarGeometry()
    g.height, g.width, g.range_bits, g.intensity_bits = int(height), int(width), int(range_bits), int(intensity_bits)
    g.range_unit, g.beam_origin = float(np.float32(range_unit)), float(np.float32(beam_origin))
    g.tables = {}
    for name, a in zip(_POLAR_TABLES, (cos_alt, sin_alt, cos_baz, sin_baz, cos_enc, sin_enc)):
        g.tables[name] = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        setattr(g, name, _fp(g.tables[name]))
    g.ticks = int(g.tables["cos_enc"].shape[0])
    return g


def polar_geometry_from_angles(height, width, altitude_rad, beam_azimuth_rad, encoder_rad, range_bits=16, intensity_bits=8,
                               range_unit=0.002, beam_origin=0.0):
    """The tables from angles in radians: altitude_rad and beam_azimuth_rad per row, encoder_rad per tick (the azimuth of the
    column that carries that tick, counter-clockwise positive).  Sines and cosines are taken in float64 and rounded to float32
    once; from there on everything is the library's table arithmetic."""
    alt = np.asarray(altitude_rad, np.float64).reshape(-1)
    baz = np.broadcast_to(np.asarray(beam_azimuth_rad, np.float64), alt.shape)
    enc = np.asarray(encoder_rad, np.float64).reshape(-1)
    return polar_geometry(height, width, range_bits, intensity_bits, range_unit, beam_origin, np.cos(alt), np.sin(alt),
                          np.cos(baz), np.sin(baz), np.cos(enc), np.sin(enc))


def polar_layout(geom):
    """Section offsets and size of a blob of this geometry (liodom_polar_layout; no handle, no device)."""
    lay = PolarLayout()
    rc = load().liodom_polar_layout(C.byref(geom), C.byref(lay))
    if rc != 0:
        raise LiodomError("liodom_polar_layout error %d: %s" % (rc, load().liodom_last_error().decode()))
    return lay


def pack_polar(geom, ticks, ranges, intensities=None, out=None):
    """One scan as a blob (uint8 array of liodom_polar_layout's total size): ticks [width], range counts and intensities
    [height * width] in the point order of the handle's lidar_type.  out: a uint8 buffer to fill instead (scan_buffer_polar)."""
    lay = polar_layout(geom)
    n = geom.height * geom.width
    blob = np.zeros(lay.total_bytes, np.uint8) if out is None else out
    blob[lay.tick_offset:lay.tick_offset + 4 * geom.width] = np.ascontiguousarray(ticks, dtype="<u4").reshape(geom.width).view(np.uint8)
    rt = "<u2" if geom.range_bits == 16 else "<u4"
    blob[lay.range_offset:lay.range_offset + n * geom.range_bits // 8] = np.ascontiguousarray(ranges, dtype=rt).reshape(n).view(np.uint8)
    if geom.intensity_bits:
        it = "u1" if geom.intensity_bits == 8 else "<u2"
        blob[lay.intensity_offset:lay.intensity_offset + n * geom.intensity_bits // 8] = np.ascontiguousarray(intensities, dtype=it).reshape(n).view(np.uint8)
    return blob


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int64), ("total_ms", C.c_double)]


_lib = None


def load():
    """Load libliodom_hip.so.  Raises LiodomError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if is_stale():
        # missing, or built from other sources than the ones present: rebuild (hipcc is part of the
        # image on the build box and on the GPU box); never load a binary that does not match the tree
        try:
            build()
        except Exception as ex:
            raise LiodomError("%s is missing or stale and could not be rebuilt (%s): run `python -c 'import "
                              "__graft_entry__ as g; g.build()'` (the HIP extension is required; there is no "
                              "CPU fallback)" % (_LIB, ex))
    L = C.CDLL(_LIB, mode=C.RTLD_GLOBAL)
    fp, dp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.liodom_last_error.restype = C.c_char_p
    L.liodom_params_default.argtypes = [C.POINTER(Params)]
    L.liodom_config_default.argtypes = [C.POINTER(Config)]
    L.liodom_create.restype = C.c_int
    L.liodom_create.argtypes = [C.POINTER(Params), C.POINTER(Config), C.POINTER(vp)]
    L.liodom_destroy.argtypes = [vp]
    L.liodom_extract_edges.restype = C.c_int
    L.liodom_extract_edges.argtypes = [vp, C.c_int, fp, C.c_int64, C.c_int, C.c_int, fp, ip, ip, ip, C.c_int, ip]
    L.liodom_odometry_step.restype = C.c_int
    L.liodom_odometry_step.argtypes = [vp, C.c_int, fp, C.c_int, C.c_double, dp, C.POINTER(StepInfo)]
    L.liodom_process_scan.restype = C.c_int
    L.liodom_process_scan.argtypes = [vp, C.c_int, fp, C.c_int64, C.c_int, C.c_int, C.c_double, dp, C.POINTER(StepInfo)]
    L.liodom_set_received_map.restype = C.c_int
    L.liodom_set_received_map.argtypes = [vp, C.c_int, fp, C.c_int64]
    L.liodom_alloc_resident.restype = C.c_int
    L.liodom_alloc_resident.argtypes = [vp, C.c_int]
    L.liodom_upload_scan.restype = C.c_int
    L.liodom_upload_scan.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int64]
    L.liodom_process_resident.restype = C.c_int
    L.liodom_process_resident.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_process_resident_pipelined.restype = C.c_int
    L.liodom_replay_resident.restype = C.c_int
    L.liodom_replay_resident.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_process_resident_pipelined.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_process_resident_subset.restype = C.c_int
    L.liodom_process_resident_subset.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int, ip, C.c_int, C.c_int64, C.c_int, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_sync.restype = C.c_int
    L.liodom_sync.argtypes = [vp]
    L.liodom_get_pose_log.restype = C.c_int
    L.liodom_get_pose_log.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_get_pose_covariance_log.restype = C.c_int
    L.liodom_get_pose_covariance_log.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(PoseCov)]
    L.liodom_wait_pose_covariance.restype = C.c_int
    L.liodom_wait_pose_covariance.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PoseCov)]
    L.liodom_reset.restype = C.c_int
    L.liodom_reset.argtypes = [vp]
    L.liodom_reset_stream.restype = C.c_int
    L.liodom_reset_stream.argtypes = [vp, C.c_int]
    L.liodom_stream_state_size.restype = C.c_int
    L.liodom_stream_state_size.argtypes = [vp, C.POINTER(C.c_int64)]
    L.liodom_export_stream_state.restype = C.c_int
    L.liodom_export_stream_state.argtypes = [vp, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.liodom_import_stream_state.restype = C.c_int
    L.liodom_import_stream_state.argtypes = [vp, C.c_int, C.c_void_p, C.c_int64]
    L.liodom_get_edges.restype = C.c_int
    L.liodom_get_edges.argtypes = [vp, C.c_int, fp, ip, ip, ip, C.c_int, ip]
    L.liodom_get_window.restype = C.c_int
    L.liodom_get_window.argtypes = [vp, C.c_int, fp, C.c_int64, C.POINTER(C.c_int64), ip]
    L.liodom_get_local_map.restype = C.c_int
    L.liodom_get_local_map.argtypes = [vp, C.c_int, fp, C.c_int64, C.POINTER(C.c_int64), ip]
    L.liodom_get_correspondences.restype = C.c_int
    L.liodom_get_correspondences.argtypes = [vp, C.c_int, C.c_int, ip, ip, ip, C.c_int, ip]
    L.liodom_get_knn_queries.restype = C.c_int
    L.liodom_get_knn_queries.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int, ip]
    L.liodom_get_curvature.restype = C.c_int
    L.liodom_get_curvature.argtypes = [vp, C.c_int, dp, C.c_int64, ip]
    L.liodom_set_profiling.restype = C.c_int
    L.liodom_set_profiling.argtypes = [vp, C.c_int]
    L.liodom_get_kernel_stats.restype = C.c_int
    L.liodom_get_kernel_stats.argtypes = [vp, C.POINTER(KernelStat)]
    L.liodom_reset_kernel_stats.restype = C.c_int
    L.liodom_reset_kernel_stats.argtypes = [vp]
    L.liodom_device_count.restype = C.c_int
    L.liodom_device_count.argtypes = [ip]
    L.liodom_device_pci_bus_id.restype = C.c_int
    L.liodom_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
    L.liodom_device_info.restype = C.c_int
    L.liodom_device_info.argtypes = [vp, C.c_char_p, C.c_int, ip]
    i64p = C.POINTER(C.c_int64)
    L.liodom_get_received_map.restype = C.c_int
    L.liodom_get_received_map.argtypes = [vp, C.c_int, fp, C.c_int64, i64p]
    L.liodom_set_imu_orientation.restype = C.c_int
    L.liodom_set_imu_orientation.argtypes = [vp, C.c_int, dp]
    L.liodom_set_laser_to_base.restype = C.c_int
    L.liodom_set_laser_to_base.argtypes = [vp, dp]
    L.liodom_attach_mapper.restype = C.c_int
    L.liodom_attach_mapper.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
    L.liodom_mapper_options_default.restype = None
    L.liodom_mapper_options_default.argtypes = [C.POINTER(MapperOptions)]
    L.liodom_attach_mapper_ex.restype = C.c_int
    L.liodom_attach_mapper_ex.argtypes = [vp, C.c_int, vp, C.POINTER(MapperOptions)]
    L.liodom_attach_map_reader.restype = C.c_int
    L.liodom_attach_map_reader.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
    L.liodom_seed_stream.restype = C.c_int
    L.liodom_seed_stream.argtypes = [vp, C.c_int, dp]
    L.liodom_map_get_local_batch.restype = C.c_int
    L.liodom_map_get_local_batch.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int, fp, C.c_int64, C.POINTER(C.c_int64)]
    L.liodom_map_prune.restype = C.c_int
    L.liodom_map_prune.argtypes = [vp, dp, C.c_int, C.c_int, ip]
    L.liodom_map_evict.restype = C.c_int
    L.liodom_map_evict.argtypes = [vp, dp, C.c_int, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64), ip]
    L.liodom_map_merge_state.restype = C.c_int
    L.liodom_map_merge_state.argtypes = [vp, vp, C.c_int64, ip, ip]
    L.liodom_map_score_poses.restype = C.c_int
    L.liodom_map_score_poses.argtypes = [vp, fp, C.c_int, dp, C.c_int, C.c_int, ip]
    L.liodom_pose_search_default.argtypes = [C.POINTER(PoseSearch)]
    L.liodom_set_map_hits.restype = C.c_int
    L.liodom_set_map_hits.argtypes = [vp, C.c_int, C.c_int]
    L.liodom_get_map_hit_log.restype = C.c_int
    L.liodom_get_map_hit_log.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.liodom_map_hit_rows.restype = C.c_int
    L.liodom_map_hit_rows.argtypes = [vp, fp, C.c_int64, ip, dp, C.c_int, C.c_int, ip]
    L.liodom_map_search_pose.restype = C.c_int
    L.liodom_map_search_pose.argtypes = [vp, fp, C.c_int, C.POINTER(PoseSearch), C.POINTER(PoseSearchResult), dp, ip]
    L.liodom_pose_search_bnb_default.argtypes = [C.POINTER(PoseSearchBnb)]
    L.liodom_map_bound_nodes.restype = C.c_int
    L.liodom_map_bound_nodes.argtypes = [vp, fp, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, ip]
    L.liodom_map_search_pose_bnb.restype = C.c_int
    L.liodom_map_search_pose_bnb.argtypes = [vp, fp, C.c_int, C.POINTER(PoseSearch), C.POINTER(PoseSearchBnb), C.POINTER(PoseSearchResult),
                                             C.POINTER(PoseSearchStats)]
    L.liodom_map_config_default.argtypes = [C.POINTER(MapConfig)]
    L.liodom_map_create.restype = C.c_int
    L.liodom_map_create.argtypes = [C.POINTER(MapConfig), C.POINTER(vp)]
    L.liodom_map_destroy.argtypes = [vp]
    L.liodom_map_update.restype = C.c_int
    L.liodom_map_update.argtypes = [vp, fp, C.c_int64, dp]
    L.liodom_map_get_local.restype = C.c_int
    L.liodom_map_get_local.argtypes = [vp, dp, C.c_int, C.c_int, fp, C.c_int64, i64p]
    L.liodom_map_get_all.restype = C.c_int
    L.liodom_map_get_all.argtypes = [vp, fp, C.c_int64, i64p]
    L.liodom_map_num_cells.restype = C.c_int
    L.liodom_map_num_cells.argtypes = [vp, ip]
    L.liodom_map_status.restype = C.c_int
    L.liodom_map_status.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.liodom_map_state_size.restype = C.c_int
    L.liodom_map_state_size.argtypes = [vp, i64p]
    L.liodom_map_export_state.restype = C.c_int
    L.liodom_map_export_state.argtypes = [vp, vp, C.c_int64, i64p]
    L.liodom_map_import_state.restype = C.c_int
    L.liodom_map_import_state.argtypes = [vp, vp, C.c_int64]
    L.liodom_map_reset.restype = C.c_int
    L.liodom_map_reset.argtypes = [vp]
    tp = C.POINTER(EdgeTicket)
    L.liodom_scan_buffer.restype = C.c_int
    L.liodom_scan_buffer.argtypes = [vp, C.c_int, C.POINTER(fp), i64p]
    L.liodom_extract_edges_device.restype = C.c_int
    L.liodom_extract_edges_device.argtypes = [vp, C.c_int, fp, C.c_int64, C.c_int, C.c_int, tp]
    L.liodom_wait_edges.restype = C.c_int
    L.liodom_wait_edges.argtypes = [vp, tp, fp, ip, ip, ip, C.c_int, ip]
    L.liodom_odometry_step_device.restype = C.c_int
    L.liodom_odometry_step_device.argtypes = [vp, tp, C.c_double, dp, C.POINTER(StepInfo)]
    L.liodom_odometry_submit_device.restype = C.c_int
    L.liodom_odometry_submit_device.argtypes = [vp, tp, C.c_double]
    L.liodom_odometry_collect.restype = C.c_int
    L.liodom_odometry_collect.argtypes = [vp, C.c_int, dp, C.POINTER(StepInfo)]
    L.liodom_pin_host_buffer.restype = C.c_int
    L.liodom_pin_host_buffer.argtypes = [C.c_void_p, C.c_int64]
    L.liodom_unpin_host_buffer.restype = C.c_int
    L.liodom_unpin_host_buffer.argtypes = [C.c_void_p]
    L.liodom_polar_layout.restype = C.c_int
    L.liodom_polar_layout.argtypes = [C.POINTER(PolarGeometry), C.POINTER(PolarLayout)]
    L.liodom_set_polar_geometry.restype = C.c_int
    L.liodom_set_polar_geometry.argtypes = [vp, C.POINTER(PolarGeometry)]
    L.liodom_project_polar.restype = C.c_int
    L.liodom_project_polar.argtypes = [vp, vp, fp]
    L.liodom_upload_scan_polar.restype = C.c_int
    L.liodom_upload_scan_polar.argtypes = [vp, C.c_int, C.c_int, vp]
    L.liodom_process_scan_polar.restype = C.c_int
    L.liodom_process_scan_polar.argtypes = [vp, C.c_int, vp, C.c_double, dp, C.POINTER(StepInfo)]
    L.liodom_scan_buffer_polar.restype = C.c_int
    L.liodom_scan_buffer_polar.argtypes = [vp, C.c_int, C.POINTER(vp), i64p]
    L.liodom_extract_edges_device_polar.restype = C.c_int
    L.liodom_extract_edges_device_polar.argtypes = [vp, C.c_int, vp, tp]
    u64p = C.POINTER(C.c_uint64)
    L.liodom_place_geometry_default.restype = None
    L.liodom_place_geometry_default.argtypes = [C.POINTER(PlaceGeometry)]
    L.liodom_places_create.restype = C.c_int
    L.liodom_places_create.argtypes = [C.POINTER(PlaceGeometry), C.c_int, C.c_int, C.POINTER(vp)]
    L.liodom_places_destroy.restype = None
    L.liodom_places_destroy.argtypes = [vp]
    L.liodom_places_count.restype = C.c_int
    L.liodom_places_count.argtypes = [vp, ip]
    L.liodom_places_reset.restype = C.c_int
    L.liodom_places_reset.argtypes = [vp]
    L.liodom_places_describe.restype = C.c_int
    L.liodom_places_describe.argtypes = [vp, fp, C.c_int64, ip, C.c_int, u64p, ip]
    L.liodom_places_add.restype = C.c_int
    L.liodom_places_add.argtypes = [vp, fp, C.c_int, dp, C.c_int64, ip]
    L.liodom_places_query.restype = C.c_int
    L.liodom_places_query.argtypes = [vp, fp, C.c_int64, ip, C.c_int, C.c_int, vp, ip]
    L.liodom_places_query_desc.restype = C.c_int
    L.liodom_places_query_desc.argtypes = [vp, u64p, C.c_int, C.c_int, vp]
    L.liodom_map_register_default.restype = None
    L.liodom_map_register_default.argtypes = [C.POINTER(RegisterOptions)]
    L.liodom_map_register_poses.restype = C.c_int
    L.liodom_map_register_poses.argtypes = [vp, C.POINTER(C.c_float), C.c_int, dp, C.c_int, C.POINTER(RegisterOptions), vp, ip]
    L.liodom_places_state_size.restype = C.c_int
    L.liodom_places_state_size.argtypes = [vp, i64p]
    L.liodom_places_export_state.restype = C.c_int
    L.liodom_places_export_state.argtypes = [vp, vp, C.c_int64, i64p]
    L.liodom_places_import_state.restype = C.c_int
    L.liodom_places_import_state.argtypes = [vp, vp, C.c_int64]
    L.liodom_graph_create.restype = C.c_int
    L.liodom_graph_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.liodom_graph_destroy.restype = None
    L.liodom_graph_destroy.argtypes = [vp]
    L.liodom_graph_reset.restype = C.c_int
    L.liodom_graph_reset.argtypes = [vp]
    L.liodom_graph_count.restype = C.c_int
    L.liodom_graph_count.argtypes = [vp, ip, ip]
    L.liodom_graph_add_nodes.restype = C.c_int
    L.liodom_graph_add_nodes.argtypes = [vp, dp, ip, C.c_int, ip]
    L.liodom_graph_add_edges.restype = C.c_int
    L.liodom_graph_add_edges.argtypes = [vp, vp, C.c_int]
    L.liodom_graph_set_fixed.restype = C.c_int
    L.liodom_graph_set_fixed.argtypes = [vp, C.c_int, C.c_int, ip]
    L.liodom_graph_get_poses.restype = C.c_int
    L.liodom_graph_get_poses.argtypes = [vp, C.c_int, C.c_int, dp]
    L.liodom_graph_set_poses.restype = C.c_int
    L.liodom_graph_set_poses.argtypes = [vp, C.c_int, C.c_int, dp]
    L.liodom_graph_get_edges.restype = C.c_int
    L.liodom_graph_get_edges.argtypes = [vp, C.c_int, C.c_int, vp]
    L.liodom_graph_linearize.restype = C.c_int
    L.liodom_graph_linearize.argtypes = [vp, dp, dp, dp]
    L.liodom_graph_multiply.restype = C.c_int
    L.liodom_graph_multiply.argtypes = [vp, C.c_double, dp, dp]
    L.liodom_graph_options_default.restype = None
    L.liodom_graph_options_default.argtypes = [C.POINTER(GraphOptions)]
    L.liodom_graph_optimize.restype = C.c_int
    L.liodom_graph_optimize.argtypes = [vp, C.POINTER(GraphOptions), C.POINTER(GraphReport)]
    L.liodom_graph_set_loss.restype = C.c_int
    L.liodom_graph_set_loss.argtypes = [vp, C.c_int, C.c_int, C.c_double]
    L.liodom_graph_get_loss.restype = C.c_int
    L.liodom_graph_get_loss.argtypes = [vp, C.c_int, ip, dp]
    L.liodom_graph_set_edge_active.restype = C.c_int
    L.liodom_graph_set_edge_active.argtypes = [vp, C.c_int, C.c_int, ip]
    L.liodom_graph_get_edge_active.restype = C.c_int
    L.liodom_graph_get_edge_active.argtypes = [vp, C.c_int, C.c_int, ip]
    L.liodom_graph_edge_weights.restype = C.c_int
    L.liodom_graph_edge_weights.argtypes = [vp, dp, dp]
    L.liodom_graph_cov_options_default.restype = None
    L.liodom_graph_cov_options_default.argtypes = [C.POINTER(GraphCovOptions)]
    L.liodom_graph_solve_columns.restype = C.c_int
    L.liodom_graph_solve_columns.argtypes = [vp, ip, C.c_int, C.POINTER(GraphCovOptions), dp, vp]
    L.liodom_graph_covariance.restype = C.c_int
    L.liodom_graph_covariance.argtypes = [vp, ip, ip, C.c_int, C.POINTER(GraphCovOptions), dp, ip]
    L.liodom_graph_gate_edges.restype = C.c_int
    L.liodom_graph_gate_edges.argtypes = [vp, vp, C.c_int, C.POINTER(GraphCovOptions), dp, ip]
    L.liodom_graph_cov_counters.restype = C.c_int
    L.liodom_graph_cov_counters.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.liodom_odom_edge_options_default.restype = None
    L.liodom_odom_edge_options_default.argtypes = [C.POINTER(OdomEdgeOptions)]
    L.liodom_chain_odometry_edges.restype = C.c_int
    L.liodom_chain_odometry_edges.argtypes = [dp, vp, C.c_int, ip, ip, C.c_int, C.POINTER(OdomEdgeOptions), vp]
    L.liodom_get_odometry_edges.restype = C.c_int
    L.liodom_get_odometry_edges.argtypes = [vp, C.c_int, ip, ip, C.c_int, C.POINTER(OdomEdgeOptions), vp]
    _lib = L
    return L


_host_lib = None


def host_lib():
    """libliodom_host.so: the C++ mirror of the reference's classes over the C-ABI (liodom_amd/host), built by make."""
    global _host_lib
    if _host_lib is None:
        load()
        hd = os.path.join(_HERE, "host")
        subprocess.check_call(["make", "-C", hd, "-s"])
        HL = C.CDLL(os.path.join(hd, "libliodom_host.so"), mode=C.RTLD_GLOBAL)
        HL.liodom_host_two_thread_replay.restype = C.c_int
        HL.liodom_host_two_thread_replay.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                     C.POINTER(C.c_int64)]
        HL.liodom_host_two_thread_replay_polar.restype = C.c_int
        HL.liodom_host_two_thread_replay_polar.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        _host_lib = HL
    return _host_lib


EXPORTED_SYMBOLS = [
    "liodom_params_default", "liodom_config_default", "liodom_create", "liodom_destroy", "liodom_last_error",
    "liodom_extract_edges", "liodom_odometry_step", "liodom_process_scan", "liodom_set_received_map",
    "liodom_alloc_resident", "liodom_upload_scan", "liodom_process_resident", "liodom_process_resident_pipelined", "liodom_process_resident_subset", "liodom_replay_resident", "liodom_sync", "liodom_get_pose_log",
    "liodom_reset", "liodom_get_edges", "liodom_get_window", "liodom_get_local_map", "liodom_get_correspondences", "liodom_get_curvature", "liodom_get_knn_queries",
    "liodom_set_profiling", "liodom_get_kernel_stats", "liodom_reset_kernel_stats", "liodom_device_info",
    "liodom_device_count", "liodom_device_pci_bus_id", "liodom_get_modes", "liodom_replay_host", "liodom_pin_host_buffer", "liodom_unpin_host_buffer",
    "liodom_map_config_default", "liodom_map_create", "liodom_map_destroy", "liodom_map_update", "liodom_map_get_local",
    "liodom_map_get_all", "liodom_map_num_cells", "liodom_map_status", "liodom_get_received_map", "liodom_attach_mapper",
    "liodom_set_imu_orientation", "liodom_set_laser_to_base",
    "liodom_scan_buffer", "liodom_extract_edges_device", "liodom_wait_edges", "liodom_odometry_step_device",
    "liodom_odometry_submit_device", "liodom_odometry_collect",
    "liodom_get_pose_covariance_log", "liodom_wait_pose_covariance",
    "liodom_reset_stream", "liodom_stream_state_size", "liodom_export_stream_state", "liodom_import_stream_state",
    "liodom_polar_layout", "liodom_set_polar_geometry", "liodom_project_polar", "liodom_upload_scan_polar", "liodom_process_scan_polar",
    "liodom_scan_buffer_polar", "liodom_extract_edges_device_polar",
    "liodom_map_state_size", "liodom_map_export_state", "liodom_map_import_state", "liodom_map_reset",
    "liodom_mapper_options_default", "liodom_attach_mapper_ex", "liodom_map_prune",
    "liodom_map_evict", "liodom_map_merge_state",
    "liodom_attach_map_reader", "liodom_seed_stream", "liodom_map_get_local_batch",
    "liodom_map_score_poses", "liodom_pose_search_default", "liodom_map_search_pose",
    "liodom_pose_search_bnb_default", "liodom_map_bound_nodes", "liodom_map_search_pose_bnb",
    "liodom_set_map_hits", "liodom_get_map_hit_log", "liodom_map_hit_rows",
    "liodom_map_register_default", "liodom_map_register_poses",
    "liodom_place_geometry_default", "liodom_places_create", "liodom_places_destroy", "liodom_places_count", "liodom_places_reset",
    "liodom_places_describe", "liodom_places_add", "liodom_places_query", "liodom_places_query_desc",
    "liodom_places_state_size", "liodom_places_export_state", "liodom_places_import_state",
    "liodom_graph_create", "liodom_graph_destroy", "liodom_graph_reset", "liodom_graph_count", "liodom_graph_add_nodes",
    "liodom_graph_add_edges", "liodom_graph_set_fixed", "liodom_graph_get_poses", "liodom_graph_set_poses", "liodom_graph_get_edges",
    "liodom_graph_linearize", "liodom_graph_multiply", "liodom_graph_options_default", "liodom_graph_optimize",
    "liodom_graph_set_loss", "liodom_graph_get_loss", "liodom_graph_set_edge_active", "liodom_graph_get_edge_active",
    "liodom_graph_edge_weights",
    "liodom_graph_cov_options_default", "liodom_graph_solve_columns", "liodom_graph_covariance", "liodom_graph_gate_edges",
    "liodom_graph_cov_counters",
    "liodom_odom_edge_options_default", "liodom_chain_odometry_edges", "liodom_get_odometry_edges",
]


def device_count():
    n = C.c_int32()
    load().liodom_device_count(C.byref(n))
    return n.value


def device_pci_bus_id(device):
    buf = C.create_string_buffer(64)
    if load().liodom_device_pci_bus_id(int(device), buf, 64) != 0:
        return None
    return buf.value.decode()


def make_params(**kw):
    """Params with the defaults of Params::readParams (src/params.cc:40-109); `prev_frames`
    is the ROS parameter behind local_map_size."""
    p = Params()
    load().liodom_params_default(C.byref(p))
    if "prev_frames" in kw:
        kw["local_map_size"] = kw.pop("prev_frames")
    for k, v in kw.items():
        setattr(p, k, v)
    if "min_points_per_scan" not in kw:
        p.min_points_per_scan = p.scan_regions * p.edges_per_region + 10  # params.cc:63
    return p


def make_config(**kw):
    c = Config()
    load().liodom_config_default(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def make_mapper_options(**kw):
    """MapperOptions with the defaults of liodom_mapper_options_default (cells 2 / 1, lag 0, no pruning)."""
    o = MapperOptions()
    load().liodom_mapper_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, int(v))
    return o


def make_pose_search(centre, **kw):
    """PoseSearch with the defaults of liodom_pose_search_default (steps 0.4 m / 0.4 m / 0.02 rad, half counts 0, radius 1) around
    centre = [qx qy qz qw tx ty tz]; keywords set step_xy, step_z, step_yaw, nx, ny, nz, nyaw, radius."""
    s = PoseSearch()
    load().liodom_pose_search_default(C.byref(s))
    s.centre[:] = [float(v) for v in np.asarray(centre, np.float64).reshape(7)]
    for k, v in kw.items():
        if k not in ("step_xy", "step_z", "step_yaw", "nx", "ny", "nz", "nyaw", "radius"):
            raise KeyError(k)
        setattr(s, k, v)
    return s


def make_register_options(**kw):
    """RegisterOptions with the defaults of liodom_map_register_default (cells 2 / 1, 10 passes, 6 matches, stops 1e-4 m / 1e-5,
    ranges 3 / 75); keywords set cells_xy, cells_z, max_passes, min_matches, local_capacity, reserved, stop_translation,
    stop_rotation, min_range, max_range."""
    o = RegisterOptions()
    load().liodom_map_register_default(C.byref(o))
    names = {f[0]: f[1] for f in RegisterOptions._fields_}
    for k, v in kw.items():
        if k not in names:
            raise KeyError(k)
        setattr(o, k, float(v) if names[k] is C.c_double else int(v))
    return o


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class Liodom:
    """One handle = one GPU, `n_streams` lock-step LiDAR streams."""

    def __init__(self, params, config):
        self.L = load()
        self.params, self.config = params, config
        h = C.c_void_p()
        rc = self.L.liodom_create(C.byref(params), C.byref(config), C.byref(h))
        if rc != 0:
            raise LiodomError("liodom_create failed (%d): %s" % (rc, self.L.liodom_last_error().decode()))
        self.h = h
        self.edge_cap = params.scan_lines * params.scan_regions * (params.edges_per_region + 1) + 64
        self.polar, self.polar_bytes = None, 0

    def _check(self, rc):
        if rc != 0:
            raise LiodomError("libliodom_hip error %d: %s" % (rc, self.L.liodom_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.liodom_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- FeatureExtractor ---
    def extract_edges(self, xyzi, height, width, stream=0):
        x = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        cap = self.edge_cap
        e = np.zeros((cap, 4), np.float32)
        ring, idx, src = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int32()
        self._check(self.L.liodom_extract_edges(self.h, stream, _fp(x), x.shape[0], height, width, _fp(e), _ip(ring),
                                                _ip(idx), _ip(src), cap, C.byref(n)))
        k = n.value
        return dict(edges=e[:k].copy(), ring=ring[:k].copy(), idx_in_ring=idx[:k].copy(), src=src[:k].copy())

    def get_edges(self, stream=0):
        cap = self.edge_cap
        e = np.zeros((cap, 4), np.float32)
        ring, idx, src = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int32()
        self._check(self.L.liodom_get_edges(self.h, stream, _fp(e), _ip(ring), _ip(idx), _ip(src), cap, C.byref(n)))
        k = n.value
        return dict(edges=e[:k].copy(), ring=ring[:k].copy(), idx_in_ring=idx[:k].copy(), src=src[:k].copy())

    # --- LaserOdometer ---
    def odometry_step(self, edges, stamp=0.0, stream=0):
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        pose = np.zeros(7)
        info = StepInfo()
        self._check(self.L.liodom_odometry_step(self.h, stream, _fp(e), e.shape[0], stamp, _dp(pose), C.byref(info)))
        return pose, info

    # --- the same two sides with the edge cloud staying on the device (tickets) ---
    def scan_buffer(self, stream=0):
        """Page-locked buffer [max_points, 4] to assemble the next cloud in (liodom_scan_buffer)."""
        p = C.POINTER(C.c_float)()
        cap = C.c_int64()
        self._check(self.L.liodom_scan_buffer(self.h, stream, C.byref(p), C.byref(cap)))
        return np.ctypeslib.as_array(p, shape=(cap.value, 4))

    def extract_edges_device(self, xyzi, height, width, stream=0):
        """Enqueues upload + extraction; returns the ticket, or None when every hand-off slot is taken (LIODOM_ERR_BUSY).
        A page-locked `xyzi` (scan_buffer / pin) must stay untouched until wait_edges or the ticket's odometry returned."""
        x = xyzi if (isinstance(xyzi, np.ndarray) and xyzi.dtype == np.float32 and xyzi.flags["C_CONTIGUOUS"]) else np.ascontiguousarray(xyzi, dtype=np.float32)
        n = x.size // 4
        t = EdgeTicket()
        rc = self.L.liodom_extract_edges_device(self.h, stream, _fp(x), n, height, width, C.byref(t))
        if rc == ERR_BUSY:
            return None
        self._check(rc)
        t._keep = x          # the upload may still be reading it
        return t

    def wait_edges(self, ticket):
        cap = self.edge_cap
        e = np.zeros((cap, 4), np.float32)
        ring, idx, src = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int32()
        self._check(self.L.liodom_wait_edges(self.h, C.byref(ticket), _fp(e), _ip(ring), _ip(idx), _ip(src), cap, C.byref(n)))
        k = n.value
        return dict(edges=e[:k].copy(), ring=ring[:k].copy(), idx_in_ring=idx[:k].copy(), src=src[:k].copy())

    def odometry_step_device(self, ticket, stamp=0.0):
        pose = np.zeros(7)
        info = StepInfo()
        self._check(self.L.liodom_odometry_step_device(self.h, C.byref(ticket), stamp, _dp(pose), C.byref(info)))
        return pose, info

    def odometry_submit_device(self, ticket, stamp=0.0):
        """False when two scans are already in flight (LIODOM_ERR_BUSY)."""
        rc = self.L.liodom_odometry_submit_device(self.h, C.byref(ticket), stamp)
        if rc == ERR_BUSY:
            return False
        self._check(rc)
        return True

    def odometry_collect(self, stream=0):
        pose = np.zeros(7)
        info = StepInfo()
        self._check(self.L.liodom_odometry_collect(self.h, stream, _dp(pose), C.byref(info)))
        return pose, info

    def two_thread_replay(self, scans, n, height, width, timed_from=0, fetch_edges=True, depth=1, pin=True):
        """The two-thread binding driven by two C++ threads (liodom_host_two_thread_replay in libliodom_host.so: an extractor
        thread with liodom_extract_edges_device + liodom_wait_edges, an odometer thread with liodom_odometry_submit_device /
        liodom_odometry_collect, a ticket queue between them).  scans: float32 [count, max_points, 4] in host memory (page-locked
        for the call if pin).  Returns (poses [count, 7], seconds from the submission of scan timed_from to the last pose,
        total number of edges fetched)."""
        HL = host_lib()
        a = np.ascontiguousarray(scans, dtype=np.float32)
        count = a.shape[0]
        stride = int(a.size // max(1, count))
        poses = np.zeros((count, 7))
        secs = C.c_double()
        tot = C.c_int64()
        pinned = pin and self.L.liodom_pin_host_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        try:
            self._check(HL.liodom_host_two_thread_replay(self.h, _fp(a), stride, count, n, height, width, int(timed_from),
                                                         1 if fetch_edges else 0, int(depth), self.edge_cap, _dp(poses),
                                                         C.byref(secs), C.byref(tot)))
        finally:
            if pinned:
                self.L.liodom_unpin_host_buffer(a.ctypes.data_as(C.c_void_p))
        return poses, secs.value, tot.value

    def process_scan(self, xyzi, height, width, stamp=0.0, stream=0):
        x = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        pose = np.zeros(7)
        info = StepInfo()
        self._check(self.L.liodom_process_scan(self.h, stream, _fp(x), x.shape[0], height, width, stamp, _dp(pose),
                                               C.byref(info)))
        return pose, info

    # --- polar scans: range counts go up, the projection to XYZI runs on the device ---
    def set_polar_geometry(self, geom):
        """liodom_set_polar_geometry: from here on the *_polar calls take blobs of this geometry (pack_polar)."""
        self._check(self.L.liodom_set_polar_geometry(self.h, C.byref(geom)))
        self.polar = geom
        self.polar_bytes = int(polar_layout(geom).total_bytes)

    def _blob(self, blob):
        if self.polar is None:
            raise LiodomError("error %d: no polar geometry has been set (set_polar_geometry)" % ERR_UNSUPPORTED)
        b = blob if (isinstance(blob, np.ndarray) and blob.dtype == np.uint8 and blob.flags["C_CONTIGUOUS"]) else np.ascontiguousarray(blob, dtype=np.uint8)
        if b.size < self.polar_bytes:
            raise ValueError("polar blob of %d bytes, the geometry needs %d" % (b.size, self.polar_bytes))
        return b

    def project_polar(self, blob):
        """The packed cloud [height * width, 4] of one blob (liodom_project_polar)."""
        b = self._blob(blob)
        out = np.zeros((self.polar.height * self.polar.width, 4), np.float32)
        self._check(self.L.liodom_project_polar(self.h, b.ctypes.data_as(C.c_void_p), _fp(out)))
        return out

    def upload_scan_polar(self, stream, slot, blob):
        b = self._blob(blob)
        self._check(self.L.liodom_upload_scan_polar(self.h, stream, slot, b.ctypes.data_as(C.c_void_p)))

    def process_scan_polar(self, blob, stamp=0.0, stream=0):
        b = self._blob(blob)
        pose = np.zeros(7)
        info = StepInfo()
        self._check(self.L.liodom_process_scan_polar(self.h, stream, b.ctypes.data_as(C.c_void_p), stamp, _dp(pose), C.byref(info)))
        return pose, info

    def scan_buffer_polar(self, stream=0):
        """Page-locked uint8 buffer of one blob to assemble the next scan in (liodom_scan_buffer_polar; pack_polar(..., out=))."""
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.L.liodom_scan_buffer_polar(self.h, stream, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,))

    def extract_edges_device_polar(self, blob, stream=0):
        """extract_edges_device for a blob: the ticket, or None when every hand-off slot is taken (LIODOM_ERR_BUSY)."""
        b = self._blob(blob)
        t = EdgeTicket()
        rc = self.L.liodom_extract_edges_device_polar(self.h, stream, b.ctypes.data_as(C.c_void_p), C.byref(t))
        if rc == ERR_BUSY:
            return None
        self._check(rc)
        t._keep = b          # the upload may still be reading it
        return t

    def two_thread_replay_polar(self, blobs, timed_from=0, fetch_edges=True, depth=1, pin=True):
        """two_thread_replay fed polar blobs (liodom_host_two_thread_replay_polar): blobs = uint8 [count, total_bytes].  Returns
        (poses [count, 7], seconds from the submission of scan timed_from to the last pose, total number of edges fetched)."""
        HL = host_lib()
        a = np.ascontiguousarray(blobs, dtype=np.uint8)
        count = a.shape[0]
        if self.polar is None:
            raise LiodomError("error %d: no polar geometry has been set (set_polar_geometry)" % ERR_UNSUPPORTED)
        if a.shape[1] < self.polar_bytes:
            raise ValueError("polar blobs of %d bytes, the geometry needs %d" % (a.shape[1], self.polar_bytes))
        poses = np.zeros((count, 7))
        secs = C.c_double()
        tot = C.c_int64()
        pinned = pin and self.L.liodom_pin_host_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        try:
            self._check(HL.liodom_host_two_thread_replay_polar(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], count, int(timed_from),
                                                               1 if fetch_edges else 0, int(depth), self.edge_cap, _dp(poses),
                                                               C.byref(secs), C.byref(tot)))
        finally:
            if pinned:
                self.L.liodom_unpin_host_buffer(a.ctypes.data_as(C.c_void_p))
        return poses, secs.value, tot.value

    # --- resident replay ---
    def alloc_resident(self, n_slots):
        self._check(self.L.liodom_alloc_resident(self.h, n_slots))

    def upload_scan(self, stream, slot, xyzi):
        x = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        self._check(self.L.liodom_upload_scan(self.h, stream, slot, _fp(x), x.shape[0]))

    def process_resident(self, slot, n, height, width, readback=True, next_slot=-1):
        """next_slot >= 0: also issue that slot's extraction on the second stream (pipelined replay)."""
        S = self.config.n_streams
        if readback:
            poses = np.zeros((S, 7))
            infos = (StepInfo * S)()
            self._check(self.L.liodom_process_resident_pipelined(self.h, slot, next_slot, n, height, width, _dp(poses), infos))
            return poses, infos
        self._check(self.L.liodom_process_resident_pipelined(self.h, slot, next_slot, n, height, width, None, None))
        return None, None

    def process_resident_subset(self, slot, streams, n, height, width, readback=True, next_slot=-1, next_streams=None):
        """One lock-step step for the streams in `streams` only (strictly ascending stream indices; liodom_process_resident_subset):
        every other stream sits the step out, untouched.  Stream s reads resident slot `slot` at its own place (upload_scan(s, slot, ...)).
        Returns (poses[len(streams), 7], infos) in list order, or (None, None) without readback or for an empty list.
        next_slot >= 0: also issue that slot's extraction ahead for next_streams (None: the same list)."""
        ls = np.ascontiguousarray(streams, dtype=np.int32).reshape(-1)
        m = int(ls.shape[0])
        nx = None if next_streams is None else np.ascontiguousarray(next_streams, dtype=np.int32).reshape(-1)
        nxp, nxn = (None, 0) if nx is None else (_ip(nx), int(nx.shape[0]))
        if readback and m > 0:
            poses = np.zeros((m, 7))
            infos = (StepInfo * m)()
            self._check(self.L.liodom_process_resident_subset(self.h, slot, _ip(ls), m, next_slot, nxp, nxn, n, height, width, _dp(poses), infos))
            return poses, infos
        self._check(self.L.liodom_process_resident_subset(self.h, slot, _ip(ls), m, next_slot, nxp, nxn, n, height, width, None, None))
        return None, None

    def replay_resident(self, first_slot, count, n, height, width, ahead=False, depth=0):
        """The pipelined consumer loop over resident slots first_slot .. first_slot + count - 1, in C
        (liodom_replay_resident): every pose read back in order; depth 0 = strictly synchronous, 1 = the odometry of
        scan k+1 is submitted before pose k is waited for.  Returns poses [count, n_streams, 7] and the step infos."""
        S = self.config.n_streams
        poses = np.zeros((count, S, 7))
        infos = (StepInfo * (count * S))()
        self._check(self.L.liodom_replay_resident(self.h, first_slot, count, 1 if ahead else 0, int(depth), n, height, width, _dp(poses), infos))
        return poses, infos

    def replay_host(self, scans, n, height, width, depth=1, pin=True):
        """Host-fed replay (liodom_replay_host): scans = float32 array [count, n_streams, max_points, 4] in host memory
        (page-locked for the duration of the call if pin).  Returns poses [count, n_streams, 7] and the step infos."""
        S = self.config.n_streams
        a = np.ascontiguousarray(scans, dtype=np.float32)
        count = a.shape[0]
        stride = int(a.size // max(1, count * S))
        poses = np.zeros((count, S, 7))
        infos = (StepInfo * (count * S))()
        self.L.liodom_replay_host.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(StepInfo)]
        self.L.liodom_pin_host_buffer.argtypes = [C.c_void_p, C.c_int64]
        self.L.liodom_unpin_host_buffer.argtypes = [C.c_void_p]
        pinned = pin and self.L.liodom_pin_host_buffer(a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        try:
            self._check(self.L.liodom_replay_host(self.h, _fp(a), stride, count, int(depth), n, height, width, _dp(poses), infos))
        finally:
            if pinned:
                self.L.liodom_unpin_host_buffer(a.ctypes.data_as(C.c_void_p))
        return poses, infos

    def modes(self):
        """The code paths this handle runs ("key=value ..." from liodom_get_modes) as a dict of strings."""
        buf = C.create_string_buffer(2048)
        self.L.liodom_get_modes.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        self._check(self.L.liodom_get_modes(self.h, buf, 2048))
        return dict(kv.split("=", 1) for kv in buf.value.decode().split())

    def sync(self):
        self._check(self.L.liodom_sync(self.h))

    def reset(self):
        self._check(self.L.liodom_reset(self.h))

    # --- streams with a life of their own ---
    def reset_stream(self, stream):
        """liodom_reset for one stream: its next scan is its first; the other streams and the pipeline keep what they have."""
        self._check(self.L.liodom_reset_stream(self.h, int(stream)))

    def stream_state_size(self):
        n = C.c_int64()
        self._check(self.L.liodom_stream_state_size(self.h, C.byref(n)))
        return n.value

    def export_stream_state(self, stream):
        """The stream's odometry state as bytes (liodom_export_stream_state); parse_stream_state reads it."""
        cap = self.stream_state_size()
        buf = (C.c_ubyte * cap)()
        n = C.c_int64()
        self._check(self.L.liodom_export_stream_state(self.h, int(stream), buf, cap, C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def import_stream_state(self, stream, blob):
        """Puts an exported state into `stream` (liodom_import_stream_state): any handle with the same local_map_size, mapping,
        filter_local_map, use_imu, pose_rotation_mode and lm_apply_step_on_ftol will do, whatever its n_streams."""
        b = bytes(blob)
        self._check(self.L.liodom_import_stream_state(self.h, int(stream), b, len(b)))

    def pose_log(self, stream, first, count):
        poses = np.zeros((count, 7))
        infos = (StepInfo * count)()
        self._check(self.L.liodom_get_pose_log(self.h, stream, first, count, _dp(poses), infos))
        return poses, infos

    def pose_covariance_log(self, stream, first, count):
        """Covariance records of scans first .. first + count - 1 (handles created with pose_covariance = 1): a list of dicts of
        NumPy arrays (pose_cov_dict); the flags are in each dict."""
        recs = (PoseCov * max(count, 1))()
        self._check(self.L.liodom_get_pose_covariance_log(self.h, stream, first, count, recs))
        return [pose_cov_dict(recs[i]) for i in range(count)]

    def odometry_edges(self, stream, scan_from, scan_to, **options):
        """The odometry edges of the intervals (scan_from[i], scan_to[i]) of `stream`, chained on the device from the stream's own
        pose log and covariance log (liodom_get_odometry_edges; handles created with pose_covariance = 1): a structured array
        (ODOM_EDGE_DTYPE) with z, covariance (Sigma_e), information (Omega) and flags (ODOM_EDGE_*) per interval.  **options:
        inflation, floor_rotation, floor_translation (make_odom_edge_options).  A refused call raises LiodomError with .code."""
        f, t = _intervals(scan_from, scan_to)
        out = np.zeros(f.shape[0], ODOM_EDGE_DTYPE)
        rc = self.L.liodom_get_odometry_edges(self.h, int(stream), _ip(f), _ip(t), f.shape[0], C.byref(make_odom_edge_options(**options)),
                                              out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            e = LiodomError("liodom_get_odometry_edges failed (%d): %s" % (rc, (self.L.liodom_last_error() or b"").decode()))
            e.code = rc
            raise e
        return out

    def wait_pose_covariance(self, stream, scan_index):
        """The covariance record of scan `scan_index` (one of the two latest of the stream), as a dict of NumPy arrays."""
        r = PoseCov()
        self._check(self.L.liodom_wait_pose_covariance(self.h, stream, scan_index, C.byref(r)))
        return pose_cov_dict(r)

    # --- inspection ---
    def window(self, stream=0):
        cap = self.edge_cap * int(self.params.local_map_size)
        w = np.zeros((cap, 4), np.float32)
        n = C.c_int64()
        nf = C.c_int32()
        self._check(self.L.liodom_get_window(self.h, stream, _fp(w), cap, C.byref(n), C.byref(nf)))
        return w[:n.value].copy(), nf.value

    def set_imu(self, q_xyzw, stream=0):
        """imuClb (liodom_node.cc:66-70): latest IMU orientation, used when params.use_imu."""
        q = np.ascontiguousarray(q_xyzw, dtype=np.float64)
        self._check(self.L.liodom_set_imu_orientation(self.h, stream, _dp(q)))

    def set_laser_to_base(self, T34):
        T = np.ascontiguousarray(T34, dtype=np.float64).reshape(12)
        self._check(self.L.liodom_set_laser_to_base(self.h, _dp(T)))

    def set_received_map(self, xyzi, stream=0):
        """mapClb (liodom_node.cc:57-64): the cloud the mapper published on ~map."""
        x = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        self._check(self.L.liodom_set_received_map(self.h, stream, _fp(x), x.shape[0]))

    def received_map(self, stream=0):
        cap = max(int(self.config.recv_capacity), 262144)
        w = np.zeros((cap, 4), np.float32)
        n = C.c_int64()
        self._check(self.L.liodom_get_received_map(self.h, stream, _fp(w), cap, C.byref(n)))
        return w[:n.value].copy()

    def attach_mapper(self, mapper, cells_xy=2, cells_z=1, stream=0, lag=0, prune_period=0, keep_cells_xy=0, keep_cells_z=0):
        """On-device mapper for this stream (liodom_attach_mapper_ex in include/liodom_hip.h).  lag = 0: the synchronous replay
        of the liodom_mapping node (faithful, and degenerate: every pose is the prediction); lag = 1: the map takes a frame when
        it leaves the sliding window (scan-to-map odometry that solves).  prune_period = n > 0: the map is pruned to the keep box
        around the pose every n-th scan.  mapper = None detaches."""
        o = make_mapper_options(cells_xy=cells_xy, cells_z=cells_z, lag=lag, prune_period=prune_period, keep_cells_xy=keep_cells_xy,
                                keep_cells_z=keep_cells_z)
        self._check(self.L.liodom_attach_mapper_ex(self.h, stream, mapper.h if mapper is not None else None, C.byref(o)))
        self._mappers = getattr(self, "_mappers", {})
        self._mappers[stream] = mapper      # keep it alive while attached

    def attach_map_reader(self, map, cells_xy=2, cells_z=1, stream=0):
        """Read-only attachment (liodom_attach_map_reader): after every scan the stream receives getLocalMap(pose) of `map`, and
        the map is never written.  Any number of streams of this handle may read one map.  map = None detaches (as
        attach_mapper(None) does, for either kind)."""
        self._check(self.L.liodom_attach_map_reader(self.h, stream, map.h if map is not None else None, int(cells_xy), int(cells_z)))
        self._mappers = getattr(self, "_mappers", {})
        self._mappers[stream] = map      # keep it alive while attached

    def seed_stream(self, pose7, stream=0):
        """The stream's next scan is its first and solves from pose7 = [qx qy qz qw tx ty tz] (liodom_seed_stream); with a mapper
        or reader attached the stream receives that map's local map at the seed."""
        p = np.ascontiguousarray(pose7, dtype=np.float64).reshape(7)
        self._check(self.L.liodom_seed_stream(self.h, int(stream), _dp(p)))

    def relocalize(self, map, scan, height, width, centre, levels, min_fraction=0.5, stream=0, refine=None):
        """Finds the stream's pose in a saved map from a rough guess and seeds the stream with it.  The scan's edges
        (extract_edges) are scored against `map` on one candidate grid per level (Map.search_pose; `levels` is a list of dicts of its
        grid keywords; a level with bnb=True goes to Map.search_pose_bnb instead, with its batch= if given), the first around `centre` = [qx qy qz qw tx ty tz], each later one around the level before's best.  If the last
        level's score / (2 * n_edges) >= min_fraction the stream is seeded with the best pose (seed_stream) and
        dict(pose, hits_r, hits_0, n_edges, fraction, levels=[each level's result]) comes back: process the SAME scan next.  Otherwise
        None, and the stream is as it was but for the edges extract_edges left in it.
        refine = dict(options of Map.register_poses) (opt-in): the verified pose is registered to the map in 6-DoF
        (Map.register_poses) and, if that row ended CONVERGED or MAX_PASSES, the stream is seeded with the registered pose instead;
        the result gains searched_pose and registration (the row's dict).  refine = None: exactly as above."""
        edges = self.extract_edges(scan, height, width, stream=stream)["edges"]
        pose, found = self._search_levels(map, edges, centre, levels)
        if not found or edges.shape[0] == 0:
            return None
        last = found[-1]
        fraction = (last["hits_r"] + last["hits_0"]) / (2.0 * edges.shape[0])
        if not fraction >= min_fraction:
            return None
        extra = {}
        if refine is not None:
            best, rows = self._refine_poses(map, edges, [pose], refine)
            extra = dict(searched_pose=np.array(pose, np.float64), registration=rows[0])
            if best is not None:
                pose = rows[best]["pose"].copy()
        self.seed_stream(pose, stream=stream)
        return dict(pose=pose, hits_r=last["hits_r"], hits_0=last["hits_0"], n_edges=int(edges.shape[0]), fraction=fraction, levels=found, **extra)

    @staticmethod
    def _refine_poses(map, edges, poses, refine):
        """Map.register_poses of `poses` in one call -> (index of the best row, rows): the best row is the one with the most valid
        correspondences among those that ended CONVERGED — failing that, MAX_PASSES —; None if no row ended either way."""
        rows = map.register_poses(edges, np.asarray(poses, np.float64).reshape(-1, 7), **dict(refine))
        for end in (REG_CONVERGED, REG_MAX_PASSES):
            ok = [i for i, r in enumerate(rows) if r["termination"] == end]
            if ok:
                return max(ok, key=lambda i: (rows[i]["matches"], -i)), rows
        return None, rows

    @staticmethod
    def _search_levels(map, edges, centre, levels):
        """The levels of relocalize: each a grid (Map.search_pose, or Map.search_pose_bnb with bnb=True) around the one before's
        best, the first around `centre` -> (the last level's pose, [each level's result])."""
        pose, found = np.array(centre, dtype=np.float64).reshape(7), []
        for grid in levels:
            grid = dict(grid)
            bnb, batch = grid.pop("bnb", False), grid.pop("batch", 0)
            found.append(map.search_pose_bnb(edges, pose, batch=batch, **grid) if bnb else map.search_pose(edges, pose, **grid))
            pose = found[-1]["pose"]
        return pose, found

    def add_place(self, places, pose, id=0, stream=0):
        """Makes the scan just processed a place: its edge cloud (get_edges: the sensor frame) goes to places.add with `pose` =
        [qx qy qz qw tx ty tz] — the pose that scan ended with — and the tag `id`.  Returns the place's index."""
        return places.add(self.get_edges(stream=stream)["edges"], pose, id)

    def relocalize_global(self, map, places, scan, height, width, k, levels, min_fraction=0.5, pager=None, stream=0, refine=None):
        """relocalize without a guess: the scan's edges (extract_edges, once) are looked up in `places` (Places.query, the k best),
        and `levels` (as relocalize's) run around the pose of every match in turn; with a `pager` (MapPager of `map`), pager.step at
        the match's pose comes first, so that the map holds the cells around it.  The match whose last level scores highest wins
        (ties go to the better rank).  If its score / (2 * n_edges) >= min_fraction the stream is seeded with the searched pose
        (with a pager: after a pager.step there) and dict(pose, hits_r, hits_0, n_edges, fraction, levels, match, rank, matches)
        comes back: process the SAME scan next.  Otherwise — also for an empty database — None, and the stream is as it was but for
        the edges extract_edges left in it.  A host loop over existing calls: nothing is scored here.
        refine = dict(options of Map.register_poses) (opt-in): every match whose last level reaches min_fraction is registered to
        the map in 6-DoF, all in ONE Map.register_poses call (with a pager: the winning match alone, after the pager.step at its
        pose), and the stream is seeded with the registered pose of the best row — most valid correspondences among the rows that
        ended CONVERGED, failing that MAX_PASSES; the result then describes that match and gains searched_pose, registration (its
        row) and registrations (all rows).  If no row ends either way the searched pose is seeded, as without refine."""
        edges = self.extract_edges(scan, height, width, stream=stream)["edges"]
        if edges.shape[0] == 0 or not levels:
            return None
        matches = places.query([edges], k)[0]
        best, verified = None, []
        for rank, m in enumerate(matches):
            if m["index"] < 0:
                break
            if pager is not None:
                pager.step(pose_T34(m["pose"]))
            pose, found = self._search_levels(map, edges, m["pose"], levels)
            score = found[-1]["hits_r"] + found[-1]["hits_0"]
            if best is None or score > best[0]:
                best = (score, rank, m, pose, found)
            if score / (2.0 * edges.shape[0]) >= min_fraction:
                verified.append((score, rank, m, pose, found))
        if best is None:
            return None
        score, rank, m, pose, found = best
        fraction = score / (2.0 * edges.shape[0])
        if not fraction >= min_fraction:
            return None
        if pager is not None:
            pager.step(pose_T34(pose))
        extra = {}
        if refine is not None:
            cands = [best] if pager is not None else verified
            pick, rows = self._refine_poses(map, edges, [c[3] for c in cands], refine)
            if pick is not None:
                score, rank, m, searched, found = cands[pick]
                fraction = score / (2.0 * edges.shape[0])
                pose = rows[pick]["pose"].copy()
                extra = dict(searched_pose=np.array(searched, np.float64), registration=rows[pick], registrations=rows)
            else:
                extra = dict(searched_pose=np.array(pose, np.float64), registration=None, registrations=rows)
        self.seed_stream(pose, stream=stream)
        return dict(pose=pose, hits_r=found[-1]["hits_r"], hits_0=found[-1]["hits_0"], n_edges=int(edges.shape[0]), fraction=fraction,
                    levels=found, match=m, rank=rank, matches=matches, **extra)

    def set_map_hits(self, radius, stream=0):
        """Per-scan map-hit records for `stream` (liodom_set_map_hits): radius 0 or 1 switches them on, -1 off."""
        self._check(self.L.liodom_set_map_hits(self.h, int(stream), int(radius)))

    def map_hits(self, first, count, stream=0):
        """Hit records of scans first .. first + count - 1 of `stream` (liodom_get_map_hit_log) as a structured array
        (MAP_HIT_DTYPE: scan_index, flags, n_edges, hits_r, hits_0, radius, reserved, T [3, 4])."""
        out = np.zeros(max(int(count), 1), MAP_HIT_DTYPE)
        self._check(self.L.liodom_get_map_hit_log(self.h, int(stream), int(first), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:max(int(count), 0)]

    def localize_scan(self, map, scan, height, width, stamp, policy, levels, stream=0):
        """process_scan with the "lost" policy and the recovery on top: the scan's hit record (set_map_hits must be on for the
        stream) is fed to `policy` (a TrackPolicy, kept by the caller from scan to scan); on LOST the stream is relocalised
        (relocalize with policy.min_fraction, `levels` as there) around the pose of the last scan whose fraction was
        >= policy.min_fraction — this scan's pose if there has been none — and, if that seeds the stream, the SAME scan is
        processed again.  Returns dict(pose, info, hit, state, relocalized): pose / info / hit (a MAP_HIT_DTYPE record) of the scan
        as it was last processed, state = what the policy answered for its first processing, relocalized = the result of
        relocalize (None: not lost, or nothing good enough was found and the stream goes on as it was)."""
        pose, info = self.process_scan(scan, height, width, stamp=stamp, stream=stream)
        hit = self.map_hits(info.scan_index, 1, stream=stream)[0].copy()
        state = policy.feed(hit["hits_r"], hit["hits_0"], hit["n_edges"], hit["flags"])
        good = getattr(policy, "last_good_pose", None)
        found = None
        if state == LOST:
            found = self.relocalize(map, scan, height, width, pose if good is None else good, levels, min_fraction=policy.min_fraction, stream=stream)
            if found is not None:
                pose, info = self.process_scan(scan, height, width, stamp=stamp, stream=stream)
                hit = self.map_hits(info.scan_index, 1, stream=stream)[0].copy()
        if (int(hit["flags"]) & HIT_VALID) and hit["n_edges"] > 0 and policy.fraction(hit["hits_r"], hit["hits_0"], hit["n_edges"]) >= policy.min_fraction:
            policy.last_good_pose = np.array(pose, dtype=np.float64)
        return dict(pose=pose, info=info, hit=hit, state=state, relocalized=found)

    def local_map(self, stream=0):
        cap = self.edge_cap * int(self.params.local_map_size) + (max(int(self.config.recv_capacity), 262144) if self.params.mapping else 0)
        w = np.zeros((cap, 4), np.float32)
        n = C.c_int64()
        filt = C.c_int32()
        self._check(self.L.liodom_get_local_map(self.h, stream, _fp(w), cap, C.byref(n), C.byref(filt)))
        return w[:n.value].copy(), bool(filt.value)

    def correspondences(self, it, stream=0):
        cap = self.edge_cap
        v, a, b = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int32()
        self._check(self.L.liodom_get_correspondences(self.h, stream, it, _ip(v), _ip(a), _ip(b), cap, C.byref(n)))
        k = n.value
        return v[:k].copy(), a[:k].copy(), b[:k].copy()

    def knn_queries(self, it, stream=0):
        """World-frame float queries of outer iteration `it` of the last step (debug_buffers = 1)."""
        cap = self.edge_cap
        q = np.zeros((cap, 4), np.float32)
        n = C.c_int32()
        self._check(self.L.liodom_get_knn_queries(self.h, stream, it, _fp(q), cap, C.byref(n)))
        return q[:n.value, :3].copy()

    def curvature(self, stream=0):
        cap = int(self.config.max_points) + 16
        c = np.zeros(cap)
        offs = np.zeros(self.params.scan_lines + 1, np.int32)
        self._check(self.L.liodom_get_curvature(self.h, stream, _dp(c), cap, _ip(offs)))
        return c[:offs[-1]].copy(), offs

    # --- measurement ---
    def set_profiling(self, on):
        self._check(self.L.liodom_set_profiling(self.h, int(on)))

    def kernel_stats(self):
        st = (KernelStat * NUM_KERNELS)()
        self._check(self.L.liodom_get_kernel_stats(self.h, st))
        return {s.name.decode(): (int(s.launches), float(s.total_ms)) for s in st}

    def reset_kernel_stats(self):
        self._check(self.L.liodom_reset_kernel_stats(self.h))

    def device_info(self):
        buf = C.create_string_buffer(256)
        cu = C.c_int32()
        self._check(self.L.liodom_device_info(self.h, buf, 256, C.byref(cu)))
        return buf.value.decode(), cu.value


class Map:
    """liodom::Map on the device (src/map.cc): updateMap / getLocalMap / getMap of the mapping node."""

    def __init__(self, xy=40.0, z=50.0, res=0.4, **caps):
        L = load()
        c = MapConfig()
        L.liodom_map_config_default(C.byref(c))
        c.voxel_xysize, c.voxel_zsize, c.resolution = xy, z, res
        for k, v in caps.items():
            if not hasattr(c, k):
                raise KeyError(k)
            setattr(c, k, v)
        self.h = C.c_void_p()
        self._L = L
        self._chk(L.liodom_map_create(C.byref(c), C.byref(self.h)))
        self.result_capacity = 1 << 18
        self.sizes = (float(xy), float(z), float(res))
        self.max_update_points = int(c.max_update_points)

    def _chk(self, rc):
        if rc != 0:
            e = LiodomError("liodom_map error %d: %s" % (rc, (self._L.liodom_last_error() or b"").decode()))
            e.code = rc      # LIODOM_ERR_* (ERR_INVALID_ARG, ERR_CAPACITY, ERR_BUSY, ...)
            raise e

    def close(self):
        if self.h:
            self._L.liodom_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _T(T34):
        return np.ascontiguousarray(np.eye(4)[:3] if T34 is None else T34, dtype=np.float64).reshape(12)

    def update(self, xyzi, T34=None):
        x = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        T = self._T(T34)
        self._chk(self._L.liodom_map_update(self.h, _fp(x), x.shape[0], _dp(T)))

    def local(self, T34=None, cells_xy=2, cells_z=1):
        T = self._T(T34)
        out = np.zeros((self.result_capacity, 4), dtype=np.float32)
        n = C.c_int64(0)
        self._chk(self._L.liodom_map_get_local(self.h, _dp(T), cells_xy, cells_z, _fp(out), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    get_local = local

    def get_local_batch(self, T, cells_xy=2, cells_z=1, cap_per_row=None):
        """local() for n poses in one launch (liodom_map_get_local_batch): T = [n, 3, 4] (or [n, 12]) -> a list of n [count, 4]
        arrays.  cap_per_row = None sizes the buffer by the library's ERR_CAPACITY reply; with a number, a larger row raises
        LiodomError with .code ERR_CAPACITY and .sizes = the rows' sizes."""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 12)
        n = T.shape[0]
        sizes = np.zeros(max(n, 1), np.int64)
        sp = sizes.ctypes.data_as(C.POINTER(C.c_int64))
        if cap_per_row is None:
            rc = self._L.liodom_map_get_local_batch(self.h, _dp(T), n, int(cells_xy), int(cells_z), None, 0, sp)
            if rc != ERR_CAPACITY:
                self._chk(rc)
            cap_per_row = int(sizes[:n].max()) if n else 0
        cap = int(cap_per_row)
        out = np.zeros((max(n, 1), max(cap, 1), 4), dtype=np.float32)
        try:
            self._chk(self._L.liodom_map_get_local_batch(self.h, _dp(T), n, int(cells_xy), int(cells_z), _fp(out), cap, sp))
        except LiodomError as e:
            e.sizes = sizes[:n].copy()
            raise
        return [out[i, :int(sizes[i])].copy() for i in range(n)]

    def score_poses(self, edges, T, radius=1):
        """hits_r, hits_0 of every candidate pose T = [n, 3, 4] (or [n, 12]) for the edge cloud `edges` [E, 4] against the map's leaf
        occupancy (liodom_map_score_poses) -> int32 [n, 2].  Read-only on the map; works on an attached map between steps."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 12)
        hits = np.zeros((T.shape[0], 2), np.int32)
        self._chk(self._L.liodom_map_score_poses(self.h, _fp(e), e.shape[0], _dp(T), T.shape[0], int(radius), _ip(hits)))
        return hits

    def hit_rows(self, edges_list, T, radius=1):
        """hits_r, hits_0 of n rows, each its own edge cloud under its own pose (liodom_map_hit_rows): edges_list = n arrays [E_i, 4],
        T = [n, 3, 4] (or [n, 12]) -> int32 [n, 2].  Row i equals score_poses(edges_list[i], T[i], radius)[0].  Read-only on the map."""
        T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 12)
        clouds = [np.ascontiguousarray(e, dtype=np.float32).reshape(-1, 4) for e in edges_list]
        n = T.shape[0]
        if len(clouds) != n:
            raise ValueError("hit_rows: one edge cloud per pose")
        counts = np.array([c.shape[0] for c in clouds], np.int32).reshape(-1)
        stride = int(counts.max()) if n else 0
        packed = np.zeros((max(n, 1), max(stride, 1), 4), np.float32)
        for i, c in enumerate(clouds):
            packed[i, :c.shape[0]] = c
        hits = np.zeros((max(n, 1), 2), np.int32)
        self._chk(self._L.liodom_map_hit_rows(self.h, _fp(packed), max(stride, 1) if n else 0, _ip(np.ascontiguousarray(counts) if n else np.zeros(1, np.int32)),
                                              _dp(T if n else np.zeros(12)), n, int(radius), _ip(hits)))
        return hits[:n]

    def search_pose(self, edges, centre, want_T=False, want_hits=False, **grid):
        """Scores the candidate grid around centre = [qx qy qz qw tx ty tz] (liodom_map_search_pose; grid keywords as
        make_pose_search: step_xy, step_z, step_yaw, nx, ny, nz, nyaw, radius) -> dict(best_index, hits_r, hits_0, n_candidates,
        pose [7] — what Liodom.seed_stream takes —, T [3, 4]) plus, when asked for, T_all [n, 3, 4] and hits [n, 2]."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        s = make_pose_search(centre, **grid)
        n = max(1, (2 * int(s.nx) + 1) * (2 * int(s.ny) + 1) * (2 * int(s.nz) + 1) * (2 * int(s.nyaw) + 1))
        if n > (1 << 20):
            n = 1          # (the library refuses the grid before it writes anything)
        T_all = np.zeros((n, 12)) if want_T else None
        hits = np.zeros((n, 2), np.int32) if want_hits else None
        r = PoseSearchResult()
        self._chk(self._L.liodom_map_search_pose(self.h, _fp(e), e.shape[0], C.byref(s), C.byref(r), _dp(T_all) if want_T else None,
                                                 _ip(hits) if want_hits else None))
        out = dict(best_index=int(r.best_index), hits_r=int(r.hits_r), hits_0=int(r.hits_0), n_candidates=int(r.n_candidates),
                   pose=np.array(r.pose[:]), T=np.array(r.T[:]).reshape(3, 4))
        if want_T:
            out["T_all"] = T_all.reshape(-1, 3, 4)
        if want_hits:
            out["hits"] = hits
        return out

    def bound_nodes(self, edges, T_lo, t_hi, level, radius=1):
        """Upper bounds of nodes of a candidate grid (liodom_map_bound_nodes): T_lo [n, 3, 4] (or [n, 12]) the matrices of the nodes'
        lowest children, t_hi [n, 2] = T[3], T[7] of their highest, all at block level `level` (1 .. 21) -> int32 [n, 2] (ub_r, ub_0).
        Read-only on the map."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        T_lo = np.ascontiguousarray(T_lo, dtype=np.float64).reshape(-1, 12)
        t_hi = np.ascontiguousarray(t_hi, dtype=np.float64).reshape(-1, 2)
        if t_hi.shape[0] != T_lo.shape[0]:
            raise ValueError("T_lo and t_hi differ in length")
        ub = np.zeros((T_lo.shape[0], 2), np.int32)
        self._chk(self._L.liodom_map_bound_nodes(self.h, _fp(e), e.shape[0], _dp(T_lo), _dp(t_hi), T_lo.shape[0], int(level), int(radius), _ip(ub)))
        return ub

    def search_pose_bnb(self, edges, centre, batch=0, **grid):
        """Map.search_pose's result for the same grid by branch-and-bound (liodom_map_search_pose_bnb): up to 2^31 - 1 candidates,
        few of them scored.  batch: nodes taken per round, 0 = the library's default.  -> search_pose's dict plus
        stats = dict(n_candidates, nodes_bounded, candidates_scored, rounds, levels_built)."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        s = make_pose_search(centre, **grid)
        opt = PoseSearchBnb()
        self._L.liodom_pose_search_bnb_default(C.byref(opt))
        if batch:
            opt.batch = int(batch)
        r, st = PoseSearchResult(), PoseSearchStats()
        self._chk(self._L.liodom_map_search_pose_bnb(self.h, _fp(e), e.shape[0], C.byref(s), C.byref(opt), C.byref(r), C.byref(st)))
        return dict(best_index=int(r.best_index), hits_r=int(r.hits_r), hits_0=int(r.hits_0), n_candidates=int(r.n_candidates),
                    pose=np.array(r.pose[:]), T=np.array(r.T[:]).reshape(3, 4),
                    stats=dict(n_candidates=int(st.n_candidates), nodes_bounded=int(st.nodes_bounded), candidates_scored=int(st.candidates_scored),
                               rounds=int(st.rounds), levels_built=int(st.levels_built)))

    def register_poses(self, edges, poses, want_corr=False, **options):
        """Registers the edge cloud `edges` [E, 4] to the map in 6-DoF from every start pose of poses = [n, 7] ([qx qy qz qw tx ty tz])
        in one call (liodom_map_register_poses; options as make_register_options) -> a list of n dicts (registration_dict), each
        with corr [E, 2] (int32, -1: no correspondence) when want_corr.  Read-only on the map; works on an attached map between
        steps.  LiodomError with .code ERR_INVALID_ARG / ERR_CAPACITY; on ERR_CAPACITY .sizes holds the rows' local-map sizes."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        n = p.shape[0]
        opt = make_register_options(**options)
        out = (Registration * max(n, 1))()
        corr = np.full((max(n, 1), max(e.shape[0], 1), 2), -1, np.int32) if want_corr else None
        try:
            self._chk(self._L.liodom_map_register_poses(self.h, _fp(e), e.shape[0], _dp(p if n else np.zeros(7)), n, C.byref(opt), out,
                                                        _ip(corr) if want_corr else None))
        except LiodomError as err:
            if err.code == ERR_CAPACITY:
                err.sizes = np.array([out[i].local_points for i in range(n)], np.int64)
            raise
        res = [registration_dict(out[i]) for i in range(n)]
        if want_corr:
            for i in range(n):
                res[i]["corr"] = corr[i, :e.shape[0]].copy()
        return res

    def prune(self, T34=None, keep_xy=2, keep_z=1):
        """Drops every cell outside the box of keep_xy / keep_z cells around the pose's cell (liodom_map_prune); returns the
        number of cells removed.  Works on an attached map too.  LiodomError with .code ERR_INVALID_ARG for a negative keep."""
        T = self._T(T34)
        n = C.c_int32(0)
        self._chk(self._L.liodom_map_prune(self.h, _dp(T), int(keep_xy), int(keep_z), C.byref(n)))
        return n.value

    def evict(self, T34=None, keep_xy=2, keep_z=1):
        """liodom_map_prune whose dropped cells come out (liodom_map_evict): -> (blob of the dropped cells, their number).  The
        buffer is sized by the library's ERR_CAPACITY reply, which leaves the map untouched.  Works on an attached map too."""
        T = self._T(T34)
        need, n = C.c_int64(0), C.c_int32(0)
        rc = self._L.liodom_map_evict(self.h, _dp(T), int(keep_xy), int(keep_z), None, 0, C.byref(need), C.byref(n))
        if rc != ERR_CAPACITY:           # (a blob is never smaller than its 64-byte header: success cannot happen here)
            self._chk(rc)
        buf = (C.c_ubyte * need.value)()
        self._chk(self._L.liodom_map_evict(self.h, _dp(T), int(keep_xy), int(keep_z), buf, need.value, C.byref(need), C.byref(n)))
        return bytes(memoryview(buf)[:need.value]), n.value

    def merge_state(self, blob):
        """Appends the cells of `blob` whose keys are not cells of the map yet (liodom_map_merge_state); -> taken, an int32 array
        with one flag per blob cell.  Allowed on an attached map.  LiodomError with .code ERR_INVALID_ARG / ERR_CAPACITY: map
        untouched."""
        b = bytes(blob)
        n_cells = int(np.frombuffer(b, "<i4", 1, 48)[0]) if len(b) >= MAP_STATE_HEADER_BYTES else 0
        taken = np.zeros(max(0, min(n_cells, (len(b) - MAP_STATE_HEADER_BYTES) // MAP_STATE_RECORD_BYTES)), np.int32)
        n = C.c_int32(0)
        self._chk(self._L.liodom_map_merge_state(self.h, b, len(b), _ip(taken) if taken.size else None, C.byref(n)))
        assert int(taken.sum()) == n.value
        return taken

    def all(self):
        out = np.zeros((self.result_capacity, 4), dtype=np.float32)
        n = C.c_int64(0)
        self._chk(self._L.liodom_map_get_all(self.h, _fp(out), out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def num_cells(self):
        n = C.c_int32(0)
        self._chk(self._L.liodom_map_num_cells(self.h, C.byref(n)))
        return n.value

    def status(self):
        s = C.c_uint32(0)
        self._chk(self._L.liodom_map_status(self.h, C.byref(s)))
        return s.value

    # --- the map as a blob ---
    def state_size(self):
        """Exact size, in bytes, of a blob of the map as it is now (liodom_map_state_size)."""
        n = C.c_int64(0)
        self._chk(self._L.liodom_map_state_size(self.h, C.byref(n)))
        return n.value

    def export_state(self):
        """The map's logical state as bytes (liodom_map_export_state); parse_map_state reads it.  Works on an attached map too."""
        cap = self.state_size()
        buf = (C.c_ubyte * cap)()
        n = C.c_int64(0)
        self._chk(self._L.liodom_map_export_state(self.h, buf, cap, C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def import_state(self, blob):
        """Makes the map what `blob` says (liodom_map_import_state): any map with the same voxel sizes and resolution will do,
        whatever its capacities.  LiodomError with .code ERR_INVALID_ARG / ERR_CAPACITY (map untouched), ERR_BUSY while attached."""
        b = bytes(blob)
        self._chk(self._L.liodom_map_import_state(self.h, b, len(b)))

    def reset(self):
        """The map as it was created: no cells, status 0; capacities and allocations kept (liodom_map_reset).  ERR_BUSY while
        attached."""
        self._chk(self._L.liodom_map_reset(self.h))


def pose_T34(pose7):
    """[qx qy qz qw tx ty tz] as a 3 x 4 matrix, the quaternion normalised in double first (as liodom_seed_stream does)."""
    p = np.asarray(pose7, np.float64).reshape(7)
    qx, qy, qz, qw = p[:4] / np.sqrt(np.sum(p[:4] * p[:4]))
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    return np.ascontiguousarray(np.concatenate([R, p[4:].reshape(3, 1)], axis=1))


class Places:
    """liodom_places_t: a device-resident set of places — one binary polar descriptor per key frame's edge cloud (sensor frame),
    with the key frame's pose and a tag — and the K nearest places of a query cloud, with the yaw offset each matches at
    (include/liodom_hip.h "finding the place").  Touches no handle and no map."""

    def __init__(self, max_places=4096, max_edges=16384, **geom):
        L = load()
        g = PlaceGeometry()
        L.liodom_place_geometry_default(C.byref(g))
        for k, v in geom.items():
            if k not in ("n_rings", "n_layers", "r_max", "z_min", "z_max"):
                raise KeyError(k)
            setattr(g, k, v)
        self.h = C.c_void_p()
        self._L = L
        self._chk(L.liodom_places_create(C.byref(g), int(max_places), int(max_edges), C.byref(self.h)))
        self.geometry = (int(g.n_rings), int(g.n_layers), float(g.r_max), float(g.z_min), float(g.z_max))
        self.words = int(g.n_rings) * int(g.n_layers)
        self.max_places, self.max_edges = int(max_places), int(max_edges)

    def _chk(self, rc):
        if rc != 0:
            e = LiodomError("liodom_places error %d: %s" % (rc, (self._L.liodom_last_error() or b"").decode()))
            e.code = rc      # LIODOM_ERR_* (ERR_INVALID_ARG, ERR_CAPACITY, ...)
            raise e

    def close(self):
        if self.h:
            self._L.liodom_places_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _rows(edges_list):
        """n clouds [E_i, 4] packed at one stride -> (packed [n, stride, 4], counts (n,), stride)."""
        clouds = [np.ascontiguousarray(e, dtype=np.float32).reshape(-1, 4) for e in edges_list]
        counts = np.array([c.shape[0] for c in clouds], np.int32).reshape(-1)
        stride = int(counts.max()) if len(clouds) else 0
        packed = np.zeros((max(len(clouds), 1), max(stride, 1), 4), np.float32)
        for i, c in enumerate(clouds):
            packed[i, :c.shape[0]] = c
        return packed, (counts if len(clouds) else np.zeros(1, np.int32)), (max(stride, 1) if len(clouds) else 0)

    def count(self):
        n = C.c_int32()
        self._chk(self._L.liodom_places_count(self.h, C.byref(n)))
        return n.value

    def reset(self):
        """No places; capacities and allocations are kept (liodom_places_reset)."""
        self._chk(self._L.liodom_places_reset(self.h))

    def describe(self, edges_list):
        """The descriptors of n edge clouds (liodom_places_describe) -> (desc [n, W] uint64, bits (n,) int32)."""
        packed, counts, stride = self._rows(edges_list)
        n = len(edges_list)
        desc, bits = np.zeros((max(n, 1), self.words), np.uint64), np.zeros(max(n, 1), np.int32)
        self._chk(self._L.liodom_places_describe(self.h, _fp(packed), stride, _ip(counts), n, desc.ctypes.data_as(C.POINTER(C.c_uint64)), _ip(bits)))
        return desc[:n], bits[:n]

    def add(self, edges, pose7, id=0):
        """Describes one edge cloud (sensor frame) and appends it as a place taken at pose7 = [qx qy qz qw tx ty tz] with the tag
        `id` (liodom_places_add) -> its index.  LiodomError with .code ERR_CAPACITY when the database is full (untouched)."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        p = np.ascontiguousarray(pose7, dtype=np.float64).reshape(7)
        idx = C.c_int32(-1)
        self._chk(self._L.liodom_places_add(self.h, _fp(e), e.shape[0], _dp(p), int(id), C.byref(idx)))
        return idx.value

    def query(self, edges_list, k=1, want_bits=False):
        """The k best places of each of n edge clouds (liodom_places_query) -> a structured array [n, k] (PLACE_MATCH_DTYPE: index,
        distance, shift, bits_place, id, pose [7], place_pose [7]; index -1 beyond the number of places), best first; with
        want_bits also the popcounts of the queries' descriptors (n,)."""
        packed, counts, stride = self._rows(edges_list)
        n = len(edges_list)
        out = np.zeros((max(n, 1), max(int(k), 1)), PLACE_MATCH_DTYPE)
        bits = np.zeros(max(n, 1), np.int32)
        self._chk(self._L.liodom_places_query(self.h, _fp(packed), stride, _ip(counts), n, int(k), out.ctypes.data_as(C.c_void_p),
                                              _ip(bits) if want_bits else None))
        return (out[:n], bits[:n]) if want_bits else out[:n]

    def query_desc(self, desc, k=1):
        """The k best places of each of n descriptors [n, W] uint64 (liodom_places_query_desc) -> as query."""
        d = np.ascontiguousarray(desc, dtype=np.uint64).reshape(-1, self.words)
        n = d.shape[0]
        out = np.zeros((max(n, 1), max(int(k), 1)), PLACE_MATCH_DTYPE)
        self._chk(self._L.liodom_places_query_desc(self.h, d.ctypes.data_as(C.POINTER(C.c_uint64)), n, int(k), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def state_size(self):
        n = C.c_int64()
        self._chk(self._L.liodom_places_state_size(self.h, C.byref(n)))
        return n.value

    def export_state(self):
        """The database as one blob (liodom_places_export_state; parse_place_state reads it)."""
        cap = self.state_size()
        buf = (C.c_ubyte * cap)()
        n = C.c_int64()
        self._chk(self._L.liodom_places_export_state(self.h, buf, cap, C.byref(n)))
        return bytes(memoryview(buf)[:n.value])

    def import_state(self, blob):
        """Makes the database what `blob` says (liodom_places_import_state): any database of the same geometry will do, whatever its
        capacity.  LiodomError with .code ERR_INVALID_ARG / ERR_CAPACITY (database untouched)."""
        b = bytes(blob)
        self._chk(self._L.liodom_places_import_state(self.h, b, len(b)))


def make_graph_options(**kw):
    """GraphOptions with the defaults of liodom_graph_options_default (20 steps, PCG to 1e-8 in at most 6 x free nodes iterations,
    gradient tolerance 1e-9, cost tolerance 1e-10)."""
    o = GraphOptions()
    load().liodom_graph_options_default(C.byref(o))
    for k, v in kw.items():
        if k not in ("max_iterations", "max_pcg_iterations", "pcg_tolerance", "gradient_tolerance", "cost_tolerance"):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def make_graph_cov_options(**kw):
    """GraphCovOptions with the defaults of liodom_graph_cov_options_default (PCG to 1e-8 in at most 6 x free nodes iterations,
    columns per launch chosen by the library)."""
    o = GraphCovOptions()
    load().liodom_graph_cov_options_default(C.byref(o))
    for k, v in kw.items():
        if k not in ("max_pcg_iterations", "batch_columns", "pcg_tolerance"):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def make_odom_edge_options(**kw):
    """OdomEdgeOptions with the defaults of liodom_odom_edge_options_default (inflation 1, no floors: the raw records)."""
    o = OdomEdgeOptions()
    load().liodom_odom_edge_options_default(C.byref(o))
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[:] = [int(x) for x in v]
        elif k in ("inflation", "floor_rotation", "floor_translation"):
            setattr(o, k, float(v))
        else:
            raise KeyError(k)
    return o


def _intervals(scan_from, scan_to):
    f = np.ascontiguousarray(np.asarray(scan_from, np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(scan_to, np.int32).reshape(-1))
    if f.shape != t.shape:
        raise ValueError("one scan_to per scan_from")
    return f, t


def pose_cov_records(dicts):
    """A list of pose_cov_dict dicts (Liodom.pose_covariance_log) as a POSE_COV_DTYPE array, what chain_odometry_edges takes."""
    out = np.zeros(len(dicts), POSE_COV_DTYPE)
    for k, d in enumerate(dicts):
        for name in POSE_COV_DTYPE.names:
            out[name][k] = d[name]
    return out


def chain_odometry_edges(poses, records, scan_from, scan_to, out=None, **options):
    """liodom_chain_odometry_edges: the odometry edges of the intervals (scan_from[i], scan_to[i]) of a stream given as host
    arrays — poses [m, 7] and records (POSE_COV_DTYPE, m), entry k is scan k — on the current device; needs no handle.
    -> a structured array (ODOM_EDGE_DTYPE); `out` (optional): the array the records are written into.  **options as
    make_odom_edge_options.  A refused call raises LiodomError with .code and leaves `out` untouched."""
    L = load()
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    r = np.ascontiguousarray(records, dtype=POSE_COV_DTYPE).reshape(-1)
    if r.shape[0] != p.shape[0]:
        raise ValueError("one record per pose")
    f, t = _intervals(scan_from, scan_to)
    if out is None:
        out = np.zeros(f.shape[0], ODOM_EDGE_DTYPE)
    if out.dtype != ODOM_EDGE_DTYPE or out.shape != (f.shape[0],) or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous ODOM_EDGE_DTYPE array with one record per interval")
    rc = L.liodom_chain_odometry_edges(_dp(p), r.ctypes.data_as(C.c_void_p), p.shape[0], _ip(f), _ip(t), f.shape[0],
                                       C.byref(make_odom_edge_options(**options)), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        e = LiodomError("liodom_chain_odometry_edges failed (%d): %s" % (rc, (L.liodom_last_error() or b"").decode()))
        e.code = rc
        raise e
    return out


def graph_edges(i, j, z, info, kind=0):
    """n edge records (GRAPH_EDGE_DTYPE) from i (n,), j (n,), z [n, 7] and info [n, 6, 6] or one [6, 6] for all."""
    i = np.asarray(i, np.int32).reshape(-1)
    out = np.zeros(i.shape[0], GRAPH_EDGE_DTYPE)
    out["i"], out["j"], out["kind"] = i, np.asarray(j, np.int32).reshape(-1), kind
    out["z"] = np.asarray(z, np.float64).reshape(-1, 7)
    out["info"] = np.asarray(info, np.float64).reshape((-1, 6, 6))
    return out


GRAPH_LOSSES = ("none", "huber", "cauchy", "geman_mcclure")      # LIODOM_GRAPH_LOSS_*


class PoseGraph:
    """liodom_graph_t: a pose graph over key frames — nodes [qx qy qz qw tx ty tz], free or fixed, and edges "X_i^-1 o X_j was
    measured as z with information info" — linearised and optimised on the device (include/liodom_hip.h "closing loops").
    Touches no handle and no map."""

    def __init__(self, max_nodes=4096, max_edges=16384):
        self._L = load()
        self.h = C.c_void_p()
        self._chk(self._L.liodom_graph_create(int(max_nodes), int(max_edges), C.byref(self.h)))
        self.max_nodes, self.max_edges = int(max_nodes), int(max_edges)

    def _chk(self, rc):
        if rc != 0:
            e = LiodomError("liodom_graph error %d: %s" % (rc, (self._L.liodom_last_error() or b"").decode()))
            e.code = rc
            raise e

    def close(self):
        if self.h:
            self._L.liodom_graph_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._chk(self._L.liodom_graph_reset(self.h))

    def count(self):
        """(nodes, edges)."""
        n, e = C.c_int32(), C.c_int32()
        self._chk(self._L.liodom_graph_count(self.h, C.byref(n), C.byref(e)))
        return n.value, e.value

    def add_nodes(self, poses, fixed=None):
        """Appends poses [n, 7] (fixed: n flags, None: all free) -> the index of the first."""
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.int32)
        if f is not None and f.shape[0] != p.shape[0]:
            raise ValueError("one fixed flag per pose")
        first = C.c_int32(-1)
        self._chk(self._L.liodom_graph_add_nodes(self.h, _dp(p), None if f is None else _ip(f), p.shape[0], C.byref(first)))
        return first.value

    def add_edges(self, edges):
        """Appends edge records (GRAPH_EDGE_DTYPE; graph_edges makes them)."""
        e = np.ascontiguousarray(edges, dtype=GRAPH_EDGE_DTYPE).reshape(-1)
        self._chk(self._L.liodom_graph_add_edges(self.h, e.ctypes.data_as(C.c_void_p), e.shape[0]))

    def set_fixed(self, first, fixed):
        f = np.ascontiguousarray(np.asarray(fixed).reshape(-1) != 0, dtype=np.int32)
        self._chk(self._L.liodom_graph_set_fixed(self.h, int(first), f.shape[0], _ip(f)))

    def poses(self, first=0, n=None):
        n = self.count()[0] - int(first) if n is None else int(n)
        out = np.zeros((max(n, 1), 7), np.float64)
        self._chk(self._L.liodom_graph_get_poses(self.h, int(first), n, _dp(out)))
        return out[:n]

    def set_poses(self, first, poses):
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        self._chk(self._L.liodom_graph_set_poses(self.h, int(first), p.shape[0], _dp(p)))

    def edges(self, first=0, n=None):
        n = self.count()[1] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), GRAPH_EDGE_DTYPE)
        self._chk(self._L.liodom_graph_get_edges(self.h, int(first), n, out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def linearize(self):
        """At the current poses -> (chi2 per edge (E,), gradient [N, 6] (0 for fixed nodes), diagonal blocks [N, 6, 6])."""
        N, E = self.count()
        chi2, g, D = np.zeros(max(E, 1)), np.zeros((max(N, 1), 6)), np.zeros((max(N, 1), 6, 6))
        self._chk(self._L.liodom_graph_linearize(self.h, _dp(chi2), _dp(g), _dp(D)))
        return chi2[:E], g[:N], D[:N]

    def multiply(self, x, lam=0.0):
        """(H + lam diag H) x at the current poses, x [N, 6] -> [N, 6]; rows and columns of fixed nodes dropped."""
        N = self.count()[0]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(N, 6)
        y = np.zeros((max(N, 1), 6))
        self._chk(self._L.liodom_graph_multiply(self.h, float(lam), _dp(x) if N else None, _dp(y)))
        return y[:N]

    def optimize(self, **options):
        """Levenberg-Marquardt with the conjugate gradients on the device (liodom_graph_optimize; keywords: make_graph_options)
        -> a dict of the report, termination as one of GRAPH_TERMINATIONS."""
        o, r = make_graph_options(**options), GraphReport()
        self._chk(self._L.liodom_graph_optimize(self.h, C.byref(o), C.byref(r)))
        d = {k: getattr(r, k) for k, _ in GraphReport._fields_}
        d["termination"] = GRAPH_TERMINATIONS[r.termination]
        return d

    def set_loss(self, kind, loss, scale=1.0):
        """The robust loss of the edges of `kind` (0 .. 15): loss one of GRAPH_LOSSES or its number, scale c > 0 in units of
        sqrt(chi2) (liodom_graph_set_loss).  reset() keeps it."""
        if isinstance(loss, str):
            if loss not in GRAPH_LOSSES:
                raise ValueError("unknown loss %r (one of %s)" % (loss, ", ".join(GRAPH_LOSSES)))
            loss = GRAPH_LOSSES.index(loss)
        self._chk(self._L.liodom_graph_set_loss(self.h, int(kind), int(loss), float(scale)))

    def loss(self, kind):
        """(name, scale) of the loss set on `kind`; the scale of "none" is 0."""
        l, c = C.c_int32(), C.c_double()
        self._chk(self._L.liodom_graph_get_loss(self.h, int(kind), C.byref(l), C.byref(c)))
        return GRAPH_LOSSES[l.value], c.value

    def set_edge_active(self, first, active):
        """Switches edges first .. first + len(active) - 1 on (true) or off: an inactive edge stays in edges() and gives nothing
        to the cost, the gradient, H, a node's degree or the preconditioner's chain."""
        a = np.ascontiguousarray(np.asarray(active).reshape(-1) != 0, dtype=np.int32)
        self._chk(self._L.liodom_graph_set_edge_active(self.h, int(first), a.shape[0], _ip(a)))

    def edge_active(self, first=0, n=None):
        n = self.count()[1] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 1), np.int32)
        self._chk(self._L.liodom_graph_get_edge_active(self.h, int(first), n, _ip(out)))
        return out[:n] != 0

    def edge_weights(self):
        """At the current poses -> (rho (E,), weight (E,)): the loss of each edge's chi2 and its derivative, the factor on the
        edge in the gradient and H; both 0 for an inactive edge."""
        E = self.count()[1]
        rho, w = np.zeros(max(E, 1)), np.zeros(max(E, 1))
        self._chk(self._L.liodom_graph_edge_weights(self.h, _dp(rho), _dp(w)))
        return rho[:E], w[:E]

    # ---- covariances and the loop gate (include/liodom_hip.h "covariances of the graph"; keywords: make_graph_cov_options) ----
    def solve_columns(self, nodes, **opt):
        """Columns of Sigma = H^-1 at the current poses (liodom_graph_solve_columns) -> (x [n, 6, N, 6], status (n, 6) of
        GRAPH_COV_STATUS_DTYPE): x[k, b] is the column of component b of node nodes[k], laid out as delta is; status[k, b] its
        iterations, status (GRAPH_COV_*) and the recurrence's |r|."""
        v = np.ascontiguousarray(np.asarray(nodes).reshape(-1), dtype=np.int32)
        n, N = v.shape[0], self.count()[0]
        x = np.zeros((max(n, 1), 6, max(N, 1), 6))
        st = np.zeros((max(n, 1), 6), GRAPH_COV_STATUS_DTYPE)
        o = make_graph_cov_options(**opt)
        self._chk(self._L.liodom_graph_solve_columns(self.h, _ip(v) if n else None, n, C.byref(o), _dp(x), st.ctypes.data_as(C.c_void_p)))
        return x[:n], st[:n]

    def covariance(self, rows, cols=None, **opt):
        """Blocks of Sigma = H^-1 at the current poses (liodom_graph_covariance) -> (blocks [n, 6, 6], status (n,) of GRAPH_COV_*):
        blocks[k] = Sigma[rows[k], cols[k]], half-angle rotation first, world frame; cols None: the marginals Sigma[n, n]."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int32)
        c = r.copy() if cols is None else np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
        if c.shape[0] != r.shape[0]:
            raise ValueError("one column node per row node")
        n = r.shape[0]
        blocks, st = np.zeros((max(n, 1), 6, 6)), np.zeros(max(n, 1), np.int32)
        o = make_graph_cov_options(**opt)
        self._chk(self._L.liodom_graph_covariance(self.h, _ip(r) if n else None, _ip(c) if n else None, n, C.byref(o), _dp(blocks), _ip(st)))
        return blocks[:n], st[:n]

    def gate_edges(self, edges, **opt):
        """The chi-square gate of candidate edges (GRAPH_EDGE_DTYPE, not added) -> (d2 (n,), status (n,) of GRAPH_COV_*): the
        squared Mahalanobis distance between each edge's z and the relative pose the graph predicts, under the graph's own
        covariance plus the edge's (liodom_graph_gate_edges); NaN unless the status is ok or not_converged."""
        e = np.ascontiguousarray(edges, dtype=GRAPH_EDGE_DTYPE).reshape(-1)
        n = e.shape[0]
        d2, st = np.zeros(max(n, 1)), np.zeros(max(n, 1), np.int32)
        o = make_graph_cov_options(**opt)
        self._chk(self._L.liodom_graph_gate_edges(self.h, e.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(o), _dp(d2), _ip(st)))
        return d2[:n], st[:n]

    def cov_counters(self):
        """(column launches, columns solved) by the three calls above since the graph was made."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self._L.liodom_graph_cov_counters(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value
