"""The place descriptor, its distance and the K best places, restated in NumPy (include/liodom_hip.h "finding the place"; DESIGN.md
§3).  Every quantity the device computes is an integer here too, and the GPU tests hold the two EQUAL.

All point arithmetic is float32, one rounding per operation (NumPy never fuses a multiply with an add); the tables are the floats
of api.place_tables — the ones the library stores in the database and in its blob.  Also here: the project's circle
(test_gpu_map_paging's run) as key frames and queries, computed once and never modified."""
import math

import numpy as np

from liodom_amd import api

DEFAULT = api.place_geometry()
F = np.float32
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def words(geom):
    return int(geom[0]) * int(geom[1])


def sectors(x, y, tables):
    """The sector 0 .. 63 of float32 points (x, y): j = #{i : |y| C_i >= |x| S_i}, then by quadrant (x < 0, y < 0 as written)."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        j = np.zeros(x.shape, np.int64)
        for c, s in zip(tables["C"], tables["S"]):
            j += (ay * F(c) >= ax * F(s)).astype(np.int64)
    xn, yn = x < F(0), y < F(0)
    return np.where(yn, np.where(xn, 32 + j, 63 - j), np.where(xn, 31 - j, j))


def bins(points, geom):
    """Per point: (word, sector), word = -1 for a point that sets nothing."""
    g = api.place_geometry(*geom)
    t = api.place_tables(g)
    p = np.asarray(points, F)
    p = p.reshape(-1, p.shape[-1])[:, :3] if p.size else np.zeros((0, 3), F)      # [n, 3] or [n, 4]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        sec = sectors(x, y, t)
        r2 = x * x + y * y                                        # float32: two multiplies, one add
        ring = (r2[:, None] >= t["R2"][None, :]).sum(axis=1)
        layer = (z[:, None] >= t["Z"][None, 1:]).sum(axis=1)
        ok = finite & (ring < g[0]) & ~(z < t["Z"][0]) & (layer < g[1])
    word = np.where(ok, ring * g[1] + layer, -1)
    return word, sec


def describe(points, geom=DEFAULT):
    """(desc (W,) uint64, bits) of one cloud [n, 3 or 4]."""
    word, sec = bins(points, geom)
    desc = np.zeros(words(geom), np.uint64)
    np.bitwise_or.at(desc, word[word >= 0], np.uint64(1) << sec[word >= 0].astype(np.uint64))
    return desc, int(np.bitwise_count(desc).sum())


def rotl(desc, s):
    """Every word rotated left by s (0 .. 63)."""
    d, s = np.asarray(desc, np.uint64), int(s) % 64
    return d.copy() if s == 0 else ((d << np.uint64(s)) | (d >> np.uint64(64 - s)))


def distances(q, k):
    """d(s), s = 0 .. 63, of a query q (W,) against places k [n, W] -> int64 [n, 64]."""
    k = np.asarray(k, np.uint64).reshape(-1, len(q))
    return np.stack([np.bitwise_count(rotl(q, s)[None, :] ^ k).sum(axis=1).astype(np.int64) for s in range(64)], axis=1)


def match(q, k):
    """(distance (n,), shift (n,)) of a query against every place: the smallest d(s), the lowest such s."""
    d = distances(q, k)
    return d.min(axis=1), d.argmin(axis=1)                        # (argmin returns the first minimum)


def topk(q, places, kk):
    """The kk best places of a query, ranked by (distance, index): [(index, distance, shift)], (-1, 0, 0) beyond the places."""
    places = np.asarray(places, np.uint64).reshape(-1, len(q))
    out = []
    if len(places):
        dist, shift = match(q, places)
        order = np.lexsort((np.arange(len(places)), dist))
        out = [(int(i), int(dist[i]), int(shift[i])) for i in order[:kk]]
    return out + [(-1, 0, 0)] * (kk - len(out))


def match_pose(place_pose, shift):
    """place_pose o Rz(shift * 2 pi / 64) in double, the place's quaternion normalised first (place_state_format.h:
    place_match_pose, operation for operation)."""
    p = [float(v) for v in np.asarray(place_pose, np.float64).reshape(7)]
    norm = math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3])
    ax, ay, az, aw = p[0] / norm, p[1] / norm, p[2] / norm, p[3] / norm
    a = float(shift) * (2.0 * math.pi / 64.0)
    bz, bw = math.sin(a / 2.0), math.cos(a / 2.0)
    return np.array([ax * bw + ay * bz, ay * bw - ax * bz, aw * bz + az * bw, aw * bw - az * bz, p[4], p[5], p[6]])


def expected_matches(q, places, kk, ids, poses, bits):
    """What liodom_places_query_desc returns for one query, as a PLACE_MATCH_DTYPE array (kk,)."""
    out = np.zeros(kk, api.PLACE_MATCH_DTYPE)
    out["index"] = -1
    for r, (i, d, s) in enumerate(topk(q, places, kk)):
        if i < 0:
            continue
        out[r] = (i, d, s, int(bits[i]), int(ids[i]), match_pose(poses[i], s), np.asarray(poses[i], np.float64))
    return out


def yaw_of(pose7):
    qx, qy, qz, qw = (float(v) for v in pose7[:4])
    return math.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))


def rot_z(points, a):
    """The cloud turned by +a about z, rounded to float32 (x, y, z, intensity kept)."""
    p = np.asarray(points, F).reshape(-1, 4).astype(np.float64)
    c, s = math.cos(a), math.sin(a)
    out = p.copy()
    out[:, 0], out[:, 1] = c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1]
    return out.astype(F)


# ---------------------------------------------------------------------------------------------
# the project's circle: key frames and queries
# ---------------------------------------------------------------------------------------------
H, W_SCAN, REGIONS, EPR = 16, 900, 8, 10
SPEED, YAW_RATE, MAX_RANGE = 1.0, 1.91, 40.0
KEY_SCANS = list(range(0, 188, 4))                 # 47 key frames at their ground-truth poses
QUERY_SCANS = list(range(188, 225))                # 37 scans of the second lap ...
QUERY_YAWS = (0.0, 1.0, 2.5)                       # ... each as it is and turned about z: 111 queries
N_SITE_SCANS = 188                                 # the site map of the end-to-end test: scans 0 .. 187
_CIRCLE = {}


def circle_params(orc):
    return orc.make_params(scan_lines=H, scan_regions=REGIONS, edges_per_region=EPR, max_range=MAX_RANGE)


def circle(orc, synth):
    """dict(scans, edges, gt) of scans 0 .. 224 (oracle edges, sensor frame), keys = [(scan, edges, gt)], queries = [(scan, yaw,
    edges turned by yaw, true pose = gt o Rz(-yaw))]."""
    if "run" not in _CIRCLE:
        cfg = synth.make_cfg(H, W_SCAN, 0, yaw_rate_deg=YAW_RATE, speed=SPEED)
        po = circle_params(orc)
        scans, edges, gts = [], [], []
        for k in range(QUERY_SCANS[-1] + 1):
            x, gt = synth.scan(cfg, 0, k)
            scans.append(x); gts.append(np.array(gt, np.float64)); edges.append(orc.extract(po, x, H, W_SCAN)["edges"])
        queries = []
        for k in QUERY_SCANS:
            for a in QUERY_YAWS:
                true = gts[k].copy()
                if a != 0.0:
                    h = -a / 2.0
                    qx, qy, qz, qw = gts[k][:4]
                    bz, bw = math.sin(h), math.cos(h)
                    true[:4] = [qx * bw + qy * bz, qy * bw - qx * bz, qw * bz + qz * bw, qw * bw - qz * bz]
                queries.append((k, a, edges[k] if a == 0.0 else rot_z(edges[k], a), true))
        _CIRCLE["run"] = dict(scans=scans, edges=edges, gt=gts, keys=[(k, edges[k], gts[k]) for k in KEY_SCANS], queries=queries)
    return _CIRCLE["run"]


def circle_model(orc, synth, geom=DEFAULT):
    """The model's database and answers on the circle: dict(desc [47, W], bits, q_desc [111, W], q_bits, top3 = per query the 3
    best [(index, distance, shift)])."""
    key = ("model",) + tuple(geom)
    if key not in _CIRCLE:
        run = circle(orc, synth)
        d = [describe(e, geom) for _, e, _ in run["keys"]]
        q = [describe(e, geom) for _, _, e, _ in run["queries"]]
        desc = np.stack([a for a, _ in d])
        _CIRCLE[key] = dict(desc=desc, bits=np.array([b for _, b in d], np.int32), q_desc=np.stack([a for a, _ in q]),
                            q_bits=np.array([b for _, b in q], np.int32), top3=[topk(a, desc, 3) for a, _ in q])
    return _CIRCLE[key]


def angle_diff(a, b):
    return abs((a - b + math.pi) % (2.0 * math.pi) - math.pi)
