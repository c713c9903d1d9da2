"""Pure-NumPy reference of the edge deskew model (include/liodom_hip.h, liodom_config_t.deskew; liodom_math.h deskew_motion /
deskew_point).  Test helper: written from the model's statement, not from the device code.

    delta    D = T_{k-2}^-1 T_{k-1} (3 x 4), the motion the constant-velocity prediction applies
    q        unit quaternion of D's rotation (Eigen's Quaterniond(D.rotation())), w >= 0: theta = 2 atan2(|v|, w), axis = v / |v|
    s        d / 2 pi - floor(d / 2 pi), d = dir (atan2(y, x) - a0): 0 = start of the sweep, 1 = its end
    p'       R(u theta)^T (p - u t),  u = 1 - s
"""
import math

import numpy as np


def rotation_of(T34, mode=1):
    """Eigen::Transform::rotation(): mode 1 = orthonormal polar factor (Eigen 3.3), 0 = linear()."""
    A = np.asarray(T34, dtype=np.float64).reshape(3, 4)[:, :3]
    if mode == 0:
        return A.copy()
    U, _, Vt = np.linalg.svd(A)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        U[:, -1] = -U[:, -1]
        R = U @ Vt
    return R


def quat_from_rot(R):
    """Eigen::Quaterniond(Matrix3d), [x y z w]."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def delta_of(T_a, T_b):
    """T_a^-1 T_b for two 3 x 4 poses."""
    A = np.asarray(T_a, dtype=np.float64).reshape(3, 4)
    B = np.asarray(T_b, dtype=np.float64).reshape(3, 4)
    R = A[:, :3].T @ B[:, :3]
    t = A[:, :3].T @ (B[:, 3] - A[:, 3])
    return np.hstack([R, t[:, None]])


def pose34(p7):
    """[qx qy qz qw tx ty tz] -> 3 x 4."""
    x, y, z, w = p7[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.hstack([R, np.asarray(p7[4:7], dtype=np.float64)[:, None]])


def motion(delta12, rotation_mode=1):
    """(axis[3], theta, t[3]) of a 3 x 4 motion."""
    D = np.asarray(delta12, dtype=np.float64).reshape(3, 4)
    q = quat_from_rot(rotation_of(D, rotation_mode))
    if q[3] < 0.0:
        q = -q
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    theta = 2.0 * math.atan2(n, q[3])
    axis = q[:3] / n if n > 0.0 else np.zeros(3)
    if n == 0.0:
        theta = 0.0
    return axis, theta, D[:, 3].copy()


def sweep_fraction(xyz, direction, a0_deg):
    """s in [0, 1) of each point from its azimuth."""
    a = np.arctan2(xyz[:, 1].astype(np.float64), xyz[:, 0].astype(np.float64))
    d = float(direction) * (a - float(np.float32(a0_deg)) * (math.pi / 180.0))
    f = d / (2.0 * math.pi)
    return f - np.floor(f)


def deskew_edges(edges, delta12, direction, a0_deg, rotation_mode=1):
    """Deskewed copy of an [E, 4] float32 XYZI edge cloud (intensity unchanged)."""
    e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
    axis, theta, t = motion(delta12, rotation_mode)
    out = e.copy()
    if theta == 0.0 and not np.any(t):
        return out
    u = 1.0 - sweep_fraction(e[:, :3], direction, a0_deg)
    p = e[:, :3].astype(np.float64) - u[:, None] * t[None, :]
    phi = u * theta
    c, s = np.cos(phi), np.sin(phi)
    kxp = np.cross(np.broadcast_to(axis, p.shape), p)
    kp = p @ axis
    # R(phi)^T p = p cos phi - sin phi (k x p) + (1 - cos phi)(k . p) k
    r = p * c[:, None] - kxp * s[:, None] + (kp * (1.0 - c))[:, None] * axis[None, :]
    out[:, :3] = r.astype(np.float32)
    return out


def ulp_diff(a, b):
    """Per-element distance in float32 ulps (same-sign floats; 0 for bit-equal values)."""
    ai = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    bi = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)
