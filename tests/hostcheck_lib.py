"""The one builder of tests/libhostcheck.so: tests/hostcheck.cc, i.e. the product's arithmetic header liodom_math.h compiled for the
host with -ffp-contract=off, and the ctypes prototypes of its entry points.  Rebuilt when the library is older than either source."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(HERE, "libhostcheck.so")
    src = os.path.join(HERE, "hostcheck.cc")
    hdr = os.path.join(HERE, "..", "liodom_amd", "csrc", "liodom_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    fp = C.POINTER(C.c_float)
    L.hc_velodyne_ring.restype = C.c_int
    L.hc_velodyne_ring.argtypes = [C.c_double] * 5 + [C.c_int]
    L.hc_curvature.restype = C.c_double
    L.hc_curvature.argtypes = [fp, fp, fp, C.c_int]
    L.hc_eig3.argtypes = [dp, dp]
    L.hc_line_gate.restype = C.c_int
    L.hc_line_gate.argtypes = [fp, fp, fp]
    L.hc_transform.argtypes = [dp, fp, C.c_int, fp]
    L.hc_pose_ops.argtypes = [dp, dp, dp, dp]
    L.hc_predict.argtypes = [dp, dp, dp]
    L.hc_predict_next.argtypes = [dp, dp, C.c_int, dp]
    L.hc_quat_from_pose.argtypes = [dp, C.c_int, dp]
    L.hc_scan_no_match.argtypes = [dp, dp, dp, dp, dp, dp, C.c_int, C.c_int, dp, dp]
    L.hc_imu_override.argtypes = [dp, dp, dp, dp, C.c_int]
    L.hc_odom_message.argtypes = [dp, dp, dp, C.c_double, dp, C.c_int]
    L.hc_rotation_of.argtypes = [dp, C.c_int, dp]
    L.hc_lm_controller.restype = C.c_int
    L.hc_lm_controller.argtypes = [dp, C.c_int, dp, dp, dp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.hc_accumulate.argtypes = [dp, C.c_int, dp, dp, C.c_double, C.c_double, dp]
    L.hc_lm_solve.restype = C.c_int
    L.hc_lm_solve.argtypes = [dp, C.c_int, dp, dp, C.c_double, C.c_double, C.c_int,
                              C.POINTER(C.c_int), C.POINTER(C.c_int), dp, dp]
    L.hc_lm_ptol_decision.restype = C.c_int
    L.hc_lm_ptol_decision.argtypes = [dp, dp, dp, dp, C.c_double]
    _lib = L
    return L
