"""Designed pose states for the pose chain that runs between the solves — k_imu_override, iso_from_qt, finalize_scan's
quat_from_pose and predict_next, rotation_of, transform_point of the new frame — and a restatement of that chain that is generic
over its arithmetic: Python floats (IEEE double, libm) or mpmath at 50 digits.  The cases and the restatement are NumPy / mpmath
only; the runners at the end also call the oracle and the host-compiled header (hostcheck_lib.py builds it on first use).  No GPU.

A case is (odom, prev_odom, imu_q, laser_to_base, rotation_mode, use_imu) in the reference's sense (odom_ = the last final pose,
prev_odom_ = the one before; laser_odometry.cc:148-195), the number of consecutive scans without correspondences it runs, and
`aim`: the decisions it is built to reach, by call site.  tests/test_designed_poses.py proves every aim on the float64
restatement; no case passes by missing its target.

Values are exact float64 by construction: rotation matrices are the correctly rounded entries of the rational rotation matrix
of an INTEGER quaternion (rot(x, y, z, w): entries integer / |q|^2, rounded once), translations and IMU quaternions are
literals.  rot(0, 0, 1, 10) is a yaw of 2 atan(0.1) = 0.1993 rad ("0.2 rad"), rot(0, 0, 3, 20) of 0.2978 rad ("0.3 rad").

The restatement (class Chain) is written from laser_odometry.cc:148-195,222-227,403, Eigen's Quaternion(Matrix3) and
toRotationMatrix, and tf's setRotation / getRPY / setRPY / getRotation, not from liodom_math.h.  Every data-dependent branch
goes through Chain.decide(site, value): the float64 run records what it decided; the 50-digit run is PINNED to those decisions
(the same formulas along the branch the float64 inputs select — a 50-digit m[6] of 1 - 1e-17 must not leave the gimbal branch
that the double 1.0 took), so it is the high-precision value of the operation the double code performs.  Chain(mutate=...)
transcribes the rules a wrong kernel would follow.

Call sites of one scan (Chain.scan): 'imu.rpy', 'bl.quat', 'bl.rpy', 'new.tfquat', 'start.quat' (use_imu only: the override and
the start point's quaternion), 'pose.quat' (the returned pose), 'pred.quat' (the next prediction's start point).

Families (each docstring says which decision it pins):
  quat_branch, gimbal, imu_quat, mount, drift, far, chain.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

Case = namedtuple("Case", "name family odom prev_odom imu_q l2b mode use_imu scans aim start_q")

PI = math.pi
PI_INSIDE = math.nextafter(math.pi, 0.0)      # the last double before atan2's cut
IDENT_Q = (0.0, 0.0, 0.0, 1.0)
ULP1 = 2.0 ** -53                      # spacing of doubles just below 1
EPS = 2.0 ** -52                       # ... and just above
SCANS_CHAIN = 32                       # see chain()

# The step's edges: 64 points on a 2.5 m lattice of the shell 6 .. 24 m around the sensor.  Any ball of radius 1 m holds at most
# ONE of them, under any rigid pose; a window of P = 3 frames therefore never offers the five neighbours within 1 m that a
# correspondence needs (laser_odometry.cc:323-324), whatever the poses of those frames.  The first frame of a stream — the
# window of every single-scan case — additionally sits FAR away from every designed pose (no window point within kilometres).
FAR = np.array([3.0e5, -2.0e5, 1.0e3])
PREV_FRAMES = 3


def edges64():
    pts = []
    for ix in range(-10, 11):
        for iy in range(-10, 11):
            for iz in (-1, 0, 1):
                p = (2.5 * ix + 0.25 * iz, 2.5 * iy - 0.5 * iz, 2.5 * iz)
                r = math.sqrt(p[0] ** 2 + p[1] ** 2)
                if 6.0 <= r <= 24.0 and (ix * 7 + iy * 3 + iz * 5) % 11 == 0:
                    pts.append(p)
    e = np.zeros((64, 4), np.float32)
    e[:, :3] = np.array(pts[:64], np.float32)
    e[:, 3] = np.arange(64, dtype=np.float32)
    assert len(pts) >= 64
    return e


def far_frame():
    f = edges64()
    f[:, :3] = (f[:, :3].astype(np.float64) + FAR).astype(np.float32)
    return f


# ---------------------------------------------------------------------------------------------
# exact constructors
# ---------------------------------------------------------------------------------------------
def rot(x, y, z, w):
    """3 x 3 rotation of the integer quaternion (x, y, z, w): each entry the double nearest to the rational entry."""
    n = x * x + y * y + z * z + w * w
    e = [[n - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), n - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), n - 2 * (x * x + y * y)]]
    return np.array([[float(Fraction(v, n)) for v in row] for row in e])


def iso(R=None, t=(0.0, 0.0, 0.0)):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) if R is None else R
    T[:, 3] = t
    return T


def signed_zeros(T, signs):
    """T with the signs of the six off-diagonal entries of its rotation block — (0,1) (0,2) (1,0) (1,2) (2,0) (2,1), zeros in the
    matrices this is used on — set as given: +0 and -0 are different inputs to a sum that ends in atan2."""
    T = np.array(T, np.float64)
    for (r, c), sg in zip(((0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)), signs):
        assert T[r, c] == 0.0
        T[r, c] = math.copysign(0.0, sg)
    return T


def compose(A, B):
    """A * B in double, in iso_mul's order (used to STATE a previous pose from a pose and a relative motion)."""
    return np.array(Chain().iso_mul(list(A.reshape(12)), list(B.reshape(12)))).reshape(3, 4)


def mm3(A, B):
    """3 x 3 (or 3 x 3 by 3-vector) product in Python floats, each entry a left-to-right sum: the same doubles on every machine."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if B.ndim == 1:
        return np.array([float(A[r, 0]) * float(B[0]) + float(A[r, 1]) * float(B[1]) + float(A[r, 2]) * float(B[2]) for r in range(3)])
    return np.array([[float(A[r, 0]) * float(B[0, c]) + float(A[r, 1]) * float(B[1, c]) + float(A[r, 2]) * float(B[2, c]) for c in range(3)] for r in range(3)])


def qmul(a, b):
    """Hamilton product of [x y z w] quaternions in double (to state an IMU orientation as yaw * pitch * roll)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)


# ---------------------------------------------------------------------------------------------
# the chain, generic over its arithmetic
# ---------------------------------------------------------------------------------------------
MUTATIONS = ("gimbal_signs", "tie_ge", "keep_imu_yaw", "l2b_not_inverted", "ignore_mode")


class Chain:
    """mp = None: Python floats.  mp = the mpmath module (mp.mp.dps set by the caller): multiprecision; `pinned` = the decisions
    of the float64 run of the same case, replayed in order."""

    def __init__(self, mp=None, pinned=None, mutate=()):
        self.mp, self.pinned, self.mutate = mp, (list(pinned) if pinned is not None else None), frozenset(mutate)
        assert self.mutate <= frozenset(MUTATIONS)
        self.trace, self.site, self.notes = [], "", {}

    # --- arithmetic ---
    def num(self, x):
        return self.mp.mpf(float(x)) if self.mp else float(x)

    def vec(self, a):
        return [self.num(v) for v in np.asarray(a, np.float64).reshape(-1)]

    def sqrt(self, x):
        return self.mp.sqrt(x) if self.mp else math.sqrt(x)

    def fn(self, name, *a):
        return getattr(self.mp if self.mp else math, name)(*a)

    def pi(self):
        return self.mp.pi if self.mp else 3.14159265358979323846

    def decide(self, what, value, **facts):
        """A data-dependent branch.  Recorded as (site.what, value, facts); a pinned run takes the recorded value."""
        label = self.site + "." + what
        if self.pinned is not None:
            plabel, pvalue, _ = self.pinned[len(self.trace)]
            assert plabel == label, (plabel, label)
            value = pvalue
        self.trace.append((label, value, facts))
        return value

    # --- Eigen ---
    def iso_mul(self, A, B):
        C = [None] * 12
        for r in range(3):
            for c in range(3):
                C[r * 4 + c] = A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c] + A[r * 4 + 2] * B[8 + c]
            C[r * 4 + 3] = A[r * 4] * B[3] + A[r * 4 + 1] * B[7] + A[r * 4 + 2] * B[11] + A[r * 4 + 3]
        return C

    def iso_inverse(self, A):
        C = [None] * 12
        for r in range(3):
            for c in range(3):
                C[r * 4 + c] = A[c * 4 + r]
        for r in range(3):
            C[r * 4 + 3] = -(C[r * 4] * A[3] + C[r * 4 + 1] * A[7] + C[r * 4 + 2] * A[11])
        return C

    def quat_from_rot(self, T):
        """Eigen::Quaterniond(Matrix3d): trace > 0, else the largest diagonal entry by two strict comparisons."""
        d = [T[0], T[5], T[10]]
        t = d[0] + d[1] + d[2]
        i = 0
        ge = "tie_ge" in self.mutate
        if (d[1] >= d[0]) if ge else (d[1] > d[0]):
            i = 1
        if (d[2] >= d[i]) if ge else (d[2] > d[i]):
            i = 2
        top = max(d)
        branch = self.decide("quat", "pos" if t > 0 else "xyz"[i], trace=float(t), tie=sum(1 for v in d if v == top) > 1)
        q = [None] * 4
        if branch == "pos":
            s = self.sqrt(t + 1)
            q[3] = self.num(0.5) * s
            s = self.num(0.5) / s
            q[0] = (T[9] - T[6]) * s
            q[1] = (T[2] - T[8]) * s
            q[2] = (T[4] - T[1]) * s
        else:
            i = "xyz".index(branch)
            j, k = (i + 1) % 3, (i + 2) % 3
            s = self.sqrt(T[i * 5] - T[j * 5] - T[k * 5] + 1)
            q[i] = self.num(0.5) * s
            s = self.num(0.5) / s
            q[3] = (T[k * 4 + j] - T[j * 4 + k]) * s
            q[j] = (T[j * 4 + i] + T[i * 4 + j]) * s
            q[k] = (T[k * 4 + i] + T[i * 4 + k]) * s
        return q

    def iso_from_qt(self, q, t):
        x, y, z, w = q
        tx, ty, tz = 2 * x, 2 * y, 2 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        return [1 - (tyy + tzz), txy - twz, txz + twy, t[0],
                txy + twz, 1 - (txx + tzz), tyz - twx, t[1],
                txz - twy, tyz + twx, 1 - (txx + tyy), t[2]]

    def rotation_of(self, T, mode):
        """Transform::rotation(): mode 1 = the orthonormal polar factor of linear() (Eigen 3.3), mode 0 = linear() (Eigen >= 3.4)."""
        if mode == 0 or "ignore_mode" in self.mutate:
            return list(T)
        if self.mp:
            mp = self.mp
            X = mp.matrix(3, 3)
            for r in range(3):
                for c in range(3):
                    X[r, c] = T[r * 4 + c]
            for _ in range(60):                       # Newton on the polar factor: exact arithmetic, quadratic
                Y = (X + mp.inverse(X).T) / 2
                done = mp.norm(Y - X, "inf") < mp.mpf(10) ** -(mp.mp.dps - 4)
                X = Y
                if done:
                    break
            R = [[X[r, c] for c in range(3)] for r in range(3)]
        else:
            A = np.array([[T[r * 4 + c] for c in range(3)] for r in range(3)])
            if np.array_equal(mm3(A.T, A), np.eye(3)):       # an exactly orthonormal matrix is its own polar factor
                R = A.tolist()
            else:
                U, _, Vt = np.linalg.svd(A)
                R = (U @ Vt).tolist()
        out = list(T)
        for r in range(3):
            for c in range(3):
                out[r * 4 + c] = R[r][c]
        return out

    def quat_from_pose(self, T, mode):
        return self.quat_from_rot(self.rotation_of(T, mode))

    # --- tf LinearMath ---
    def tf_matrix(self, q):
        x, y, z, w = q
        d = x * x + y * y + z * z + w * w
        s = 2 / d
        xs, ys, zs = x * s, y * s, z * s
        wx, wy, wz = w * xs, w * ys, w * zs
        xx, xy, xz = x * xs, x * ys, x * zs
        yy, yz, zz = y * ys, y * zs, z * zs
        return [1 - (yy + zz), xy - wz, xz + wy, xy + wz, 1 - (xx + zz), yz - wx, xz - wy, yz + wx, 1 - (xx + yy)]

    def tf_get_rpy(self, m):
        """getEulerYPR, solution 1.  Returns roll, pitch, yaw."""
        lock = self.decide("rpy", "lock+" if (abs(m[6]) >= 1 and m[6] < 0) else ("lock-" if abs(m[6]) >= 1 else "free"), m6=float(m[6]))
        if lock != "free":
            up = lock == "lock+"
            if "gimbal_signs" in self.mutate:
                up = not up
            rpy = self.fn("atan2", m[7], m[8]), (self.pi() / 2 if up else -self.pi() / 2), self.num(0)
        else:
            pitch = -self.fn("asin", m[6])
            cp = self.fn("cos", pitch)
            rpy = self.fn("atan2", m[7] / cp, m[8] / cp), pitch, self.fn("atan2", m[3] / cp, m[0] / cp)
        self.notes[self.site + ".rpy"] = tuple(float(v) for v in rpy)      # (what the conditions of the gimbal family read)
        return rpy

    def tf_set_rpy(self, roll, pitch, yaw):
        ci, cj, ch = self.fn("cos", roll), self.fn("cos", pitch), self.fn("cos", yaw)
        si, sj, sh = self.fn("sin", roll), self.fn("sin", pitch), self.fn("sin", yaw)
        cc, cs, sc, ss = ci * ch, ci * sh, si * ch, si * sh
        return [cj * ch, sj * sc - cs, sj * cc + ss, cj * sh, sj * ss + cc, sj * cs - sc, -sj, cj * si, cj * ci]

    def tf_quat(self, m):
        """tf::Matrix3x3::getRotation: trace > 0, else the largest diagonal entry by nested strict comparisons."""
        t = m[0] + m[4] + m[8]
        if "tie_ge" in self.mutate:
            i = (2 if m[4] <= m[8] else 1) if m[0] <= m[4] else (2 if m[0] <= m[8] else 0)
        else:
            i = (2 if m[4] < m[8] else 1) if m[0] < m[4] else (2 if m[0] < m[8] else 0)
        d = [m[0], m[4], m[8]]
        branch = self.decide("tfquat", "pos" if t > 0 else "xyz"[i], trace=float(t), tie=sum(1 for v in d if v == max(d)) > 1)
        q = [None] * 4
        if branch == "pos":
            s = self.sqrt(t + 1)
            q[3] = s * self.num(0.5)
            s = self.num(0.5) / s
            q[0], q[1], q[2] = (m[7] - m[5]) * s, (m[2] - m[6]) * s, (m[3] - m[1]) * s
        else:
            i = "xyz".index(branch)
            j, k = (i + 1) % 3, (i + 2) % 3
            s = self.sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1)
            q[i] = s * self.num(0.5)
            s = self.num(0.5) / s
            q[3] = (m[k * 3 + j] - m[j * 3 + k]) * s
            q[j] = (m[j * 3 + i] + m[i * 3 + j]) * s
            q[k] = (m[k * 3 + i] + m[i * 3 + k]) * s
        return q

    def imu_override(self, odom, imu_q, l2b, mode):
        """laser_odometry.cc:152-183."""
        self.site = "imu"
        imu_roll, imu_pitch, imu_yaw = self.tf_get_rpy(self.tf_matrix(imu_q))
        self.site = "bl"
        odom_bl = self.iso_mul(odom, l2b)
        q_bl = self.quat_from_pose(odom_bl, mode)
        _, _, bl_yaw = self.tf_get_rpy(self.tf_matrix(q_bl))
        self.site = "new"
        m = self.tf_set_rpy(imu_roll, imu_pitch, imu_yaw if "keep_imu_yaw" in self.mutate else bl_yaw)
        q_new = self.tf_quat(m)
        odom_bl = self.iso_from_qt(q_new, [odom_bl[3], odom_bl[7], odom_bl[11]])
        return self.iso_mul(odom_bl, l2b if "l2b_not_inverted" in self.mutate else self.iso_inverse(l2b))

    def predict(self, odom, prev):
        """:148-150: odom * (prev^-1 * odom)."""
        return self.iso_mul(odom, self.iso_mul(self.iso_inverse(prev), odom))

    def scan(self, odom, prev, imu_q, l2b, mode, use_imu, start_q=None):
        """One scan without correspondences from (odom_, prev_odom_): :148-195, two solves that change nothing, :222-227, :403.
        start_q: the start point's quaternion is GIVEN (a tie case: what the previous solve left), not derived.
        Returns dict(final, pose_q, pred, pred_q): the final pose (= the next prev_odom_), the returned quaternion, the next
        prediction (with use_imu the un-overridden one: the device stores it when the scan ends) and its quaternion."""
        pred = self.predict(odom, prev)
        if use_imu:
            pred = self.imu_override(pred, imu_q, l2b, mode)
        self.site = "start"
        q = list(start_q) if start_q is not None else self.quat_from_pose(pred, mode)
        final = self.iso_from_qt(q, [pred[3], pred[7], pred[11]])
        self.site = "pose"
        pose_q = self.quat_from_pose(final, mode)
        nxt = self.predict(final, odom)
        self.site = "pred"
        return dict(final=final, pose_q=pose_q, pred=nxt, pred_q=self.quat_from_pose(nxt, mode), start=pred)

    def run(self, case):
        """The case's scans.  Returns the list of per-scan results."""
        odom, prev = self.vec(case.odom), self.vec(case.prev_odom)
        imu_q, l2b = self.vec(case.imu_q), self.vec(case.l2b)
        out = []
        for k in range(case.scans):
            sq = self.vec(case.start_q) if (case.start_q is not None and k == 0) else None
            r = self.scan(odom, prev, imu_q, l2b, case.mode, case.use_imu, sq)
            out.append(r)
            odom, prev = r["final"], odom
        return out

    def odom_message(self, prev, cur, l2b, dt, mode):
        """publishOdom :395-436: orientation, position, linear and angular twist (13)."""
        self.site = "msg"
        bl = self.iso_mul(cur, l2b)
        q = self.quat_from_pose(bl, mode)
        d = self.iso_mul(self.iso_inverse(self.iso_mul(prev, l2b)), bl)
        self.site = "twist"
        roll, pitch, yaw = self.tf_get_rpy(self.tf_matrix(self.quat_from_pose(d, mode)))
        return q + [bl[3], bl[7], bl[11], d[3] / dt, d[7] / dt, d[11] / dt, roll / dt, pitch / dt, yaw / dt]


def decisions(trace, site):
    """The values decided at `site` (e.g. 'pose.quat'), in order."""
    return [v for label, v, _ in trace if label == site]


def facts(trace, site):
    return [f for label, _, f in trace if label == site]


# ---------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------
I34 = iso()
YAW02 = rot(0, 0, 1, 10)               # 0.1993 rad about z
YAW03 = rot(0, 0, 3, 20)               # 0.2978 rad about z
STEP = iso(YAW02, (3.0, 0.0, 0.0))     # the relative motion of `far` and `chain`: 3 m, "0.2 rad"
E_DRIFT = np.array([[0.25, -0.5, 0.125], [0.375, 0.0625, -0.75], [-0.3125, 0.875, 0.1875]])


def _case(name, family, odom, prev=None, imu_q=IDENT_Q, l2b=None, mode=1, use_imu=0, scans=1, aim=None, start_q=None):
    odom = np.asarray(odom, np.float64)
    return Case(name, family, odom, odom.copy() if prev is None else np.asarray(prev, np.float64), tuple(float(v) for v in imu_q),
                I34.copy() if l2b is None else np.asarray(l2b, np.float64), mode, use_imu, scans, dict(aim or {}),
                None if start_q is None else tuple(float(v) for v in start_q))


def quat_branch():
    """Pins every outcome of Eigen's Quaternion(Matrix3) (quat_from_rot) at 'pose.quat' — and, with the override on, of tf's
    getRotation (tf_quat_from_matrix) at 'new.tfquat': trace > 0; trace <= 0 with the largest diagonal entry at x, y, z; the
    exact half turns about each axis (trace -1, two diagonal entries tied at -1 BELOW the largest: no tie of the largest); 120
    degrees about (1,1,1) (trace exactly 0, all three entries tied: the strict > keeps x); traces a few ulps either side of 0
    (start_q = (1,1,1,1)/2 scaled by 1 -+ 2^-52, mode 0); and a tie of the two largest entries whose two candidates give
    DIFFERENT quaternions (mode 0, a non-unit start point: the matrix is not a rotation, so the branches are not equivalent).
    The stationary stream (prev = odom) keeps the matrix exact through the prediction where its entries are 0 and +-1."""
    t = (1.0, -2.0, 0.5)
    out = []
    for use_imu in (0, 1):
        tag = "_imu" if use_imu else ""
        site = "new.tfquat" if use_imu else "pose.quat"
        out += [
            _case("qb_pos" + tag, "quat_branch", iso(rot(1, 2, 2, 9), t), use_imu=use_imu, aim={"pose.quat": "pos"}),
            _case("qb_pi_z" + tag, "quat_branch", iso(rot(0, 0, 1, 0), t), use_imu=use_imu, aim={site: "z"}),
            _case("qb_big_z" + tag, "quat_branch", iso(rot(1, 2, 9, 1), t), use_imu=use_imu, aim={site: "z"}),
        ]
    out += [
        # tf's getRotation at y: roll pi from the IMU on a pose whose yaw is pi (R = Rz(pi) Rx(pi) = the half turn about y), and near it
        _case("qb_pi_y_imu", "quat_branch", iso(rot(0, 0, 1, 0), t), imu_q=(1.0, 0.0, 0.0, 0.0), use_imu=1, aim={"new.tfquat": "y", "pose.quat": "y"}),
        _case("qb_big_y_imu", "quat_branch", iso(rot(0, 0, 8, 1), t), imu_q=(8.0, 0.0, 0.0, 1.0), use_imu=1, aim={"new.tfquat": "y", "pose.quat": "y"}),
        _case("qb_big_x_imu", "quat_branch", iso(rot(0, 0, 1, 8), t), imu_q=(8.0, 0.0, 0.0, 1.0), use_imu=1, aim={"new.tfquat": "x", "pose.quat": "x"}),
        _case("qb_pi_x", "quat_branch", iso(rot(1, 0, 0, 0), t), aim={"pose.quat": "x"}),
        _case("qb_pi_y", "quat_branch", iso(rot(0, 1, 0, 0), t), aim={"pose.quat": "y"}),
        _case("qb_big_x", "quat_branch", iso(rot(9, 2, 1, 1), t), aim={"pose.quat": "x"}),
        _case("qb_big_y", "quat_branch", iso(rot(2, 9, 1, 1), t), aim={"pose.quat": "y"}),
        _case("qb_120", "quat_branch", iso(rot(1, 1, 1, 1), t), aim={"pose.quat": "x", "pose.trace": 0.0, "pose.tie": True}),
        _case("qb_120_m0", "quat_branch", iso(rot(1, 1, 1, 1), t), mode=0, aim={"pose.quat": "x", "pose.trace": 0.0, "pose.tie": True}),
        _case("qb_trace_above", "quat_branch", iso(rot(1, 1, 1, 1), t), mode=0, start_q=[0.5 * (1 - 2.0 ** -52)] * 4,
              aim={"pose.quat": "pos", "pose.trace_ulps": (6, 6)}),
        _case("qb_trace_below", "quat_branch", iso(rot(1, 1, 1, 1), t), mode=0, start_q=[0.5 * (1 + 2.0 ** -52)] * 4,
              aim={"pose.quat": "x", "pose.trace_ulps": (-6, -6), "pose.tie": True}),
        # the two largest diagonal entries tied (x^2 = y^2), the start point 1 + 2^-10 too long: candidates x and y differ by ~1e-3
        _case("qb_tie_xy", "quat_branch", iso(rot(6, -6, 3, 1), t), mode=0, start_q=[v * (1 + 2.0 ** -10) / 8.0 for v in (6, -6, 2.5, 1)],
              aim={"pose.quat": "x", "pose.tie": True}),
        _case("qb_tie_yz", "quat_branch", iso(rot(1, 6, -6, 3), t), mode=0, start_q=[v * (1 + 2.0 ** -10) / 8.0 for v in (1, 6, -6, 2.5)],
              aim={"pose.quat": "y", "pose.tie": True}),
    ]
    return out


def _imu_ypr(yaw_t, pitch_t, roll_t):
    """IMU orientation yaw * pitch * roll from half-angle tangents (unnormalised: tf divides the norm out)."""
    return qmul(qmul((0.0, 0.0, yaw_t, 1.0), (0.0, pitch_t, 0.0, 1.0)), (roll_t, 0.0, 0.0, 1.0))


def gimbal():
    """Pins tf's getRPY (tf_get_rpy) at 'imu.rpy' and 'bl.rpy': the lock branch with m[6] exactly -1 (pitch +pi/2: 'lock+') and
    +1 ('lock-'), reached exactly because (0, +-1, 0, 1) has |q|^2 = 2 and 2 / 2 = 1; m[6] 2 and 4 ulps inside +-1 ('free', with
    cos(pitch) ~ 1e-8 dividing the atan2 arguments); pitch at +-(pi/2 - 1e-8) and +-(pi/2 - 1e-4) (half-angle tangent 1 - d);
    yaw at +pi and at -pi exactly, the last double inside the cut on either side and 1.9e-9 inside; roll likewise (1.8e-12 inside).
    The aims state the SIGNED angle.  With use_imu the pitch of the IMU becomes the pitch of the pose,
    so the lock cases also put the POSE at a quarter turn."""
    odom = iso(YAW03, (4.0, -1.0, 0.5))
    out = []
    for name, q, aim in [
        ("gb_lock_up", (0.0, 1.0, 0.0, 1.0), {"imu.rpy": "lock+", "imu.m6": -1.0}),
        ("gb_lock_down", (0.0, -1.0, 0.0, 1.0), {"imu.rpy": "lock-", "imu.m6": 1.0}),
        ("gb_lock_up_rolled", qmul((0.0, 1.0, 0.0, 1.0), (0.25, 0.0, 0.0, 1.0)), {"imu.rpy": "lock+"}),
        ("gb_near_up_1", (0.0, 1.0 - 2.0 ** -26, 0.0, 1.0), {"imu.rpy": "free", "imu.m6_ulps": (2, 2)}),
        ("gb_near_up_2", (0.0, 1.0 - 2.0 ** -25, 0.0, 1.0), {"imu.rpy": "free", "imu.m6_ulps": (4, 4)}),
        ("gb_near_down_1", (0.0, -(1.0 - 2.0 ** -26), 0.0, 1.0), {"imu.rpy": "free", "imu.m6_ulps": (2, 2)}),
        ("gb_near_down_2", (0.0, -(1.0 - 2.0 ** -25), 0.0, 1.0), {"imu.rpy": "free", "imu.m6_ulps": (4, 4)}),
        ("gb_pitch_p_1e8", _imu_ypr(0.125, 1.0 - 1e-8, 0.0625), {"imu.rpy": "free", "imu.pitch_gap": (0.5e-8, 3e-8)}),
        ("gb_pitch_m_1e8", _imu_ypr(0.125, -(1.0 - 1e-8), 0.0625), {"imu.rpy": "free", "imu.pitch_gap": (0.5e-8, 3e-8)}),
        ("gb_pitch_p_1e4", _imu_ypr(0.125, 1.0 - 1e-4, 0.0625), {"imu.rpy": "free", "imu.pitch_gap": (0.5e-4, 2e-4)}),
        ("gb_pitch_m_1e4", _imu_ypr(0.125, -(1.0 - 1e-4), 0.0625), {"imu.rpy": "free", "imu.pitch_gap": (0.5e-4, 2e-4)}),
        ("gb_roll_pi", (1.0, 0.0, 0.0, 0.0), {"imu.rpy": "free", "imu.roll": PI}),
        # m[7] = yz + wx = -0 + -0: atan2(-0, -1) = -pi exactly, the other side of the cut
        ("gb_roll_mpi", (1.0, -0.0, 0.0, -0.0), {"imu.rpy": "free", "imu.roll": -PI}),
        # m[7] = +-2^-51, m[8] = -1: the last double before the cut, on either side
        ("gb_roll_pi_ulp", (1.0, 0.0, 0.0, 2.0 ** -52), {"imu.rpy": "free", "imu.roll": PI_INSIDE}),
        ("gb_roll_mpi_ulp", (1.0, 0.0, 0.0, -2.0 ** -52), {"imu.rpy": "free", "imu.roll": -PI_INSIDE}),
        ("gb_roll_pi_inside", (1.0, 0.0, 0.0, 2.0 ** -40), {"imu.rpy": "free", "imu.roll_gap": (1e-13, 1e-11)}),
        ("gb_roll_mpi_inside", (1.0, 0.0, 0.0, -2.0 ** -40), {"imu.rpy": "free", "imu.roll_gap": (1e-13, 1e-11)}),
    ]:
        out.append(_case(name, "gimbal", odom, imu_q=q, use_imu=1, aim=aim))
    half_turn = iso(rot(0, 0, 1, 0), (4.0, -1.0, 0.5))
    out += [
        _case("gb_yaw_pi", "gimbal", half_turn, imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1, aim={"bl.rpy": "free", "bl.yaw": PI}),
        # yaw -pi exactly needs m[3] = xy + wz = -0 + -0 at the base link: signed zeros in the pose, the previous pose and the mounting
        # that survive the sums of iso_mul (found by search over the 2^18 sign patterns; mode 0: linear() goes through untouched)
        _case("gb_yaw_mpi", "gimbal", signed_zeros(half_turn, (-1, -1, -1, 1, -1, -1)), prev=half_turn, imu_q=(0.0625, -0.125, 0.0, 1.0),
              l2b=signed_zeros(I34, (1, 1, 1, -1, -1, 1)), mode=0, use_imu=1, aim={"bl.rpy": "free", "bl.yaw": -PI}),
        # rot(0, 0, 2^52, +-1) = [[-1, -+2^-51, 0], [+-2^-51, -1, 0], [0, 0, 1]] exactly: m[3] = +-2^-51, the last double before the cut
        _case("gb_yaw_pi_ulp", "gimbal", iso(rot(0, 0, 2 ** 52, 1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1,
              aim={"bl.rpy": "free", "bl.yaw": PI_INSIDE}),
        _case("gb_yaw_mpi_ulp", "gimbal", iso(rot(0, 0, 2 ** 52, -1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1,
              aim={"bl.rpy": "free", "bl.yaw": -PI_INSIDE}),
        _case("gb_yaw_pi_inside", "gimbal", iso(rot(0, 0, 2 ** 30, 1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1,
              aim={"bl.rpy": "free", "bl.yaw_gap": (1e-10, 1e-8)}),
        _case("gb_yaw_mpi_inside", "gimbal", iso(rot(0, 0, 2 ** 30, -1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1,
              aim={"bl.rpy": "free", "bl.yaw_gap": (1e-10, 1e-8)}),
        # the base-link orientation itself in the lock branch: a pose pitched by a quarter turn
        _case("gb_bl_lock_up", "gimbal", iso(rot(0, 1, 0, 1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1, aim={"bl.rpy": "lock+"}),
        _case("gb_bl_lock_down", "gimbal", iso(rot(0, -1, 0, 1), (4.0, -1.0, 0.5)), imu_q=(0.0625, -0.125, 0.0, 1.0), use_imu=1, aim={"bl.rpy": "lock-"}),
    ]
    return out


def imu_quat():
    """Pins tf's setRotation (tf_matrix_from_quat: the division by |q|^2) at the override's input: identity; q and -q (the same
    orientation: the results must be equal); norms 1e-3 and 1e3; one dominant and three tiny components."""
    odom = iso(rot(1, -1, 3, 12), (-7.0, 2.5, 0.25))
    prev = compose(odom, iso(rot(0, 0, -1, 10), (-0.75, 0.125, 0.0)))
    q = (0.09, -0.12, 0.2, 0.96)
    return [
        _case("iq_identity", "imu_quat", odom, prev, IDENT_Q, use_imu=1),
        _case("iq_q", "imu_quat", odom, prev, q, use_imu=1),
        _case("iq_minus_q", "imu_quat", odom, prev, tuple(-v for v in q), use_imu=1, aim={"same_as": "iq_q"}),
        _case("iq_norm_1e-3", "imu_quat", odom, prev, tuple(v * 1e-3 for v in q), use_imu=1, aim={"close_to": "iq_q"}),
        _case("iq_norm_1e3", "imu_quat", odom, prev, tuple(v * 1e3 for v in q), use_imu=1, aim={"close_to": "iq_q"}),
        _case("iq_dominant", "imu_quat", odom, prev, (1e-9, -3e-10, 2e-9, 1.0), use_imu=1),
        _case("iq_dominant_x", "imu_quat", odom, prev, (1.0, 1e-9, -3e-10, 2e-9), use_imu=1, aim={"new.tfquat": "x"}),
    ]


def mount():
    """Pins the two uses of laser_to_base in the override (:164 odom * l2b, :182 * l2b^-1): a lever arm of metres, rotations of
    0.3 rad, a sensor mounted upside down (roll pi) and one on its side (pitch pi/2: the base-link orientation of a LEVEL laser
    pose is then in the gimbal lock)."""
    odom = iso(YAW02, (12.0, 5.0, -1.0))
    prev = compose(odom, iso(rot(0, 0, -1, 20), (-1.5, 0.0, 0.0)))
    q = (0.05, 0.08, -0.3, 0.95)
    return [
        _case("mt_lever", "mount", odom, prev, q, iso(None, (1.5, -0.75, 2.0)), use_imu=1),
        _case("mt_rot_03", "mount", odom, prev, q, iso(mm3(rot(3, 0, 0, 20), rot(0, 3, 0, 20)), (0.5, 0.25, 1.0)), use_imu=1),
        _case("mt_rot_03_m0", "mount", odom, prev, q, iso(mm3(rot(3, 0, 0, 20), rot(0, 3, 0, 20)), (0.5, 0.25, 1.0)), mode=0, use_imu=1),
        _case("mt_upside_down", "mount", odom, prev, q, iso(rot(1, 0, 0, 0), (0.0, 0.0, 1.0)), use_imu=1),
        _case("mt_on_its_side", "mount", iso(None, (12.0, 5.0, -1.0)), iso(None, (11.0, 5.0, -1.0)), q, iso(rot(0, 1, 0, 1), (0.25, 0.0, 0.5)), use_imu=1,
              aim={"bl.rpy": "lock+"}),
    ]


def drift():
    """Pins rotation_of: odom = R (I + eps E) for eps 1e-15, 1e-9, 1e-4, both pose_rotation_mode values.  Mode 1 must return the
    polar factor (the quaternion of the returned pose is then a unit quaternion), mode 0 the linear part untouched (it is not)."""
    R = rot(2, -3, 1, 7)
    out = []
    for eps in (1e-15, 1e-9, 1e-4):
        A = mm3(R, np.eye(3) + eps * E_DRIFT)
        for mode in (0, 1):
            for use_imu in (0, 1):
                out.append(_case("dr_%g_m%d%s" % (eps, mode, "_imu" if use_imu else ""), "drift", iso(A, (2.0, 3.0, -1.0)), imu_q=(0.1, -0.05, 0.0, 1.0),
                                 mode=mode, use_imu=use_imu, aim={"eps": eps}))
    return out


def far():
    """Pins the cancellation in iso_inverse / iso_mul: translations of 10 km and more with a relative motion inv(prev) * cur of
    3 m and 0.2 rad."""
    out = []
    for name, t in (("fr_10km", (1.0e4, -1.2e4, 35.0)), ("fr_100km", (-1.0e5, 7.0e4, -250.0))):
        odom = iso(rot(1, -2, 9, 11), t)
        prev = compose(odom, iso(rot(0, 0, -1, 10), tuple(float(v) for v in -mm3(YAW02.T, np.array([3.0, 0.0, 0.0])))))
        out.append(_case(name, "far", odom, prev, aim={"step": (3.0, 0.1993)}))
        out.append(_case(name + "_imu", "far", odom, prev, imu_q=(0.02, -0.03, 0.0, 1.0), l2b=iso(None, (1.0, 0.0, 1.5)), use_imu=1, aim={"step": (3.0, 0.1993)}))
    return out


def chain():
    """Pins the constant-velocity recursion pred = T (T_prev^-1 T) over SCANS_CHAIN = 32 consecutive scans without
    correspondences at 0.2 rad and 3 m per scan (6.4 rad in all, a full turn about z: the returned quaternion goes through the
    'pos' and the 'z' case of Eigen's constructor and back; x and y belong to quat_branch), both rotation modes, with and without
    the override.  32: on the CPU model the mode-0 start pose, 7.6e-11 off orthonormal, is still at 4e-11 after 8 scans (the
    tan^2(theta/2) growth of DESIGN.md's finding needs more than a quarter turn), at 1.7e-7 after 16, 7.0e-4 after 24 and 6.6e-4
    after 32, with a largest defect of 5e-3 on the way — the growth is there, the pose is not yet lost (at 48 scans the defect is
    0.6) — while mode 1 and the override (which rebuilds the rotation from angles every scan) stay below 2e-15."""
    R0 = rot(1, 2, -1, 8)
    A = mm3(R0, np.eye(3) + 1e-9 * E_DRIFT)
    odom = iso(A, (20.0, -10.0, 1.0))
    prev = compose(iso(R0, (20.0, -10.0, 1.0)), iso(rot(0, 0, -1, 10), tuple(float(v) for v in -mm3(YAW02.T, np.array([3.0, 0.0, 0.0])))))
    out = []
    for mode in (0, 1):
        out.append(_case("ch_m%d" % mode, "chain", odom, prev, mode=mode, scans=SCANS_CHAIN))
        out.append(_case("ch_m%d_imu" % mode, "chain", odom, prev, imu_q=(0.03, -0.02, 0.0, 1.0), l2b=iso(rot(1, 0, 0, 20), (0.5, 0.0, 1.0)),
                         mode=mode, use_imu=1, scans=SCANS_CHAIN))
    return out


FAMILIES = dict(quat_branch=quat_branch, gimbal=gimbal, imu_quat=imu_quat, mount=mount, drift=drift, far=far, chain=chain)


def all_cases():
    out = {}
    for fam in FAMILIES.values():
        for c in fam():
            assert c.name not in out
            out[c.name] = c
    return out


CASES = all_cases()


# ---------------------------------------------------------------------------------------------
# runners shared by the CPU and the GPU suite (results cached per case: a reference is computed once and never changed)
# ---------------------------------------------------------------------------------------------
_cache = {}


def _arr(r):
    """A Chain.scan result as float64 arrays: final [12], pose [7] (quaternion, translation), pred [12], pred_q [4]."""
    f = np.array([float(v) for v in r["final"]])
    return dict(final=f, pose=np.array([float(v) for v in r["pose_q"]] + [f[3], f[7], f[11]]),
                pred=np.array([float(v) for v in r["pred"]]), pred_q=np.array([float(v) for v in r["pred_q"]]))


def float_run(name):
    """The float64 restatement of the case: (per-scan results, the decisions it took, 1 / conditioning of its getRPY calls)."""
    if ("f", name) not in _cache:
        ch = Chain()
        res = [_arr(r) for r in ch.run(CASES[name])]
        _cache[("f", name)] = (res, ch.trace, ch.notes)
    return _cache[("f", name)]


def mp_run(name, dps=50):
    """The same formulas at `dps` digits along the float64 run's decisions, rounded to double at the very end."""
    if ("mp", name) not in _cache:
        import mpmath
        with mpmath.workdps(dps):
            ch = Chain(mp=mpmath, pinned=float_run(name)[1])
            res = [_arr(r) for r in ch.run(CASES[name])]
        _cache[("mp", name)] = res
    return _cache[("mp", name)]


def hostcheck_lib():
    """tests/hostcheck.cc — liodom_math.h compiled for the host, without contraction (built and described by hostcheck_lib.py)."""
    import hostcheck_lib
    return hostcheck_lib.load()


def _dp(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_double))


def device_state(name):
    """What a stream's state record holds when the case's first scan starts (kernels_state.h): odom = the prediction formed when
    the previous scan finished, prev_odom = final_odom = the case's odom, param_q / param_t = the solve's start point — by the
    host-compiled header, which is what finalize_scan would have left."""
    case, L = CASES[name], hostcheck_lib()
    p19 = np.zeros(19)
    T, P = np.ascontiguousarray(case.odom.reshape(12)), np.ascontiguousarray(case.prev_odom.reshape(12))
    L.hc_predict_next(_dp(T), _dp(P), case.mode, _dp(p19))
    st = dict(odom=p19[:12].copy(), prev_odom=T.copy(), final_odom=T.copy(), param_q=p19[12:16].copy(), param_t=p19[16:19].copy(),
              imu_q=np.array(case.imu_q))
    if case.start_q is not None:
        st["param_q"] = np.array(case.start_q)
    return st


def hc_run(name):
    """The case on the host-compiled header, scan by scan in the kernels' order.  Per scan: final, pose, pred, pred_q, and the
    record the device exports afterwards (odom, prev_odom, final_odom, param_q, param_t)."""
    if ("hc", name) not in _cache:
        case, L = CASES[name], hostcheck_lib()
        st = device_state(name)
        odom, prev, pq, pt = st["odom"].copy(), st["prev_odom"].copy(), st["param_q"].copy(), st["param_t"].copy()
        imu, l2b = np.array(case.imu_q), np.ascontiguousarray(case.l2b.reshape(12))
        out = []
        for _ in range(case.scans):
            fin, pose = np.zeros(12), np.zeros(7)
            L.hc_scan_no_match(_dp(odom), _dp(prev), _dp(pq), _dp(pt), _dp(imu), _dp(l2b), case.mode, case.use_imu, _dp(fin), _dp(pose))
            out.append(dict(final=fin, pose=pose, pred=odom.copy(), pred_q=pq.copy(),
                            record=dict(odom=odom.copy(), prev_odom=prev.copy(), final_odom=fin.copy(), param_q=pq.copy(), param_t=pt.copy())))
        _cache[("hc", name)] = out
    return _cache[("hc", name)]


def hc_transform(T12, xyzi):
    import ctypes as C
    x = np.ascontiguousarray(xyzi, np.float32)
    out = np.zeros_like(x)
    fp = C.POINTER(C.c_float)
    hostcheck_lib().hc_transform(_dp(np.ascontiguousarray(T12, np.float64).reshape(12)), x.ctypes.data_as(fp), x.shape[0], out.ctypes.data_as(fp))
    return out


def orc_run(orc, name):
    """The case on the oracle's own Odometer.step(), from the designed state, behind one far-away first frame.  Per scan: final,
    pose, the newest window frame.  None for a case with a given start point (the oracle derives its start point itself)."""
    case = CASES[name]
    if case.start_q is not None:
        return None
    if ("orc", name) not in _cache:
        po = orc.make_params(scan_lines=16, scan_regions=6, edges_per_region=10, prev_frames=PREV_FRAMES, pose_rotation_mode=case.mode)
        od = orc.Odometer(po)
        od.step(far_frame())
        od.set_imu(np.array(case.imu_q), use_imu=bool(case.use_imu))
        od.set_laser_to_base(case.l2b)
        od.set_state(case.odom, case.prev_odom, True)
        e, out = edges64(), []
        for _ in range(case.scans):
            pose, info = od.step(e)
            assert list(info.matches) == [0, 0] and [info.lm[0].termination, info.lm[1].termination] == [4, 4], (name, list(info.matches))
            fin, _ = od.state()
            out.append(dict(final=fin.reshape(12).copy(), pose=pose.copy(), frame=od.window()[-64:].copy()))
        od.close()
        _cache[("orc", name)] = out
    return _cache[("orc", name)]


def scale_of(name):
    """Size of the numbers a case's translation arithmetic handles (the 1e-13 of a rotation entry is relative to 1)."""
    c = CASES[name]
    return max(1.0, float(np.abs(c.odom[:, 3]).max()), float(np.abs(c.prev_odom[:, 3]).max()))


def pose_distance(a, b, scale=1.0, with_pred=False):
    """Largest difference of two scan results over final (rotation entries absolute, translations relative to `scale`) and the
    returned quaternion (q and -q are the same rotation); with_pred: the next prediction and its quaternion as well."""
    d = np.abs(a["final"] - b["final"])
    d[[3, 7, 11]] /= scale
    qa, qb = a["pose"][:4], b["pose"][:4]
    out = float(max(d.max(), min(np.abs(qa - qb).max(), np.abs(qa + qb).max())))
    if with_pred:
        d = np.abs(a["pred"] - b["pred"])
        d[[3, 7, 11]] /= scale
        qa, qb = a["pred_q"], b["pred_q"]
        out = float(max(out, d.max(), min(np.abs(qa - qb).max(), np.abs(qa + qb).max())))
    return out


def yardstick(orc, name):
    """The oracle's distance to the 50-digit value, worst scan of the case: what the device's bars are measured in.  A case with a
    given start point takes the host-compiled header in the oracle's place."""
    if ("y", name) not in _cache:
        ref = mp_run(name)
        got = orc_run(orc, name) or hc_run(name)
        _cache[("y", name)] = max(pose_distance(g, r, scale_of(name)) for g, r in zip(got, ref))
    return _cache[("y", name)]


CUT_CASES = [n for n, c in CASES.items() if "imu.roll" in c.aim or "bl.yaw" in c.aim]


def cut_agrees(got_final, want_final):
    """Which side of atan2's cut an angle of +-pi came out on, and whether it is pi or the double before it, shows only in the
    entries of the final pose that are sin(angle) times something: 1.2e-16 at +-pi, 5.7e-16 one step inside, with the angle's
    sign.  They are products and sums of factors that are each accurate to a few ulps RELATIVE, so a correct implementation has
    them with the right sign and, generously, within a factor 1.5 (oracle and header differ by up to 3 % there, through the last
    bits of the polar factor; pi against the double before it is a factor 4.6).  True when every entry of want_final between
    1e-20 and 1e-12 in magnitude has that in got_final; there must be such an entry."""
    want, got = np.asarray(want_final).reshape(12), np.asarray(got_final).reshape(12)
    idx = [i for i in range(12) if 1e-20 < abs(want[i]) < 1e-12]
    return bool(idx) and all(got[i] * want[i] > 0 and 1 / 1.5 <= got[i] / want[i] <= 1.5 for i in idx)
