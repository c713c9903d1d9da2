"""tests/odom_edge_host.cc — the odometry-edge leaf functions of liodom_math.h — compiled for the host with -ffp-contract=off into
a directory the caller names, and the ctypes prototypes of its entry points."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(directory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check"
    so = os.path.join(str(directory), "libodomedgehost.so")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-ffp-contract=off", "-shared", "-o", so,
                        os.path.join(ROOT, "tests", "odom_edge_host.cc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    L.oeh_chain.restype = None
    L.oeh_chain.argtypes = [dp, vp, ip, ip, C.c_int, C.c_double, C.c_double, C.c_double, vp]
    L.oeh_totals.restype = None
    L.oeh_totals.argtypes = [dp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp]
    L.oeh_term.restype = None
    L.oeh_term.argtypes = [dp, dp, C.c_double, C.c_double, C.c_double, dp]
    L.oeh_usable.restype = C.c_int
    L.oeh_usable.argtypes = [vp, C.c_int]
    L.oeh_edge_covariance.restype = None
    L.oeh_edge_covariance.argtypes = [dp, dp, dp]
    L.oeh_information.restype = C.c_int
    L.oeh_information.argtypes = [dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def chain(L, poses, recs, scan_from, scan_to, inflation=1.0, floor_rotation=0.0, floor_translation=0.0):
    """The host-compiled header's records (api.ODOM_EDGE_DTYPE) of the intervals; 0 <= from < to < m is the caller's business."""
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    r = np.ascontiguousarray(recs, dtype=api.POSE_COV_DTYPE).reshape(-1)
    f = np.ascontiguousarray(np.asarray(scan_from, np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray(scan_to, np.int32).reshape(-1))
    assert r.shape[0] == p.shape[0] and f.shape == t.shape and np.all((0 <= f) & (f < t) & (t < p.shape[0]))
    out = np.zeros(f.shape[0], api.ODOM_EDGE_DTYPE)
    L.oeh_chain(_dp(p), r.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_int32)),
                f.shape[0], inflation, floor_rotation, floor_translation, out.ctypes.data_as(C.c_void_p))
    return out


def totals(L, poses, recs, a, b, inflation=1.0, floor_rotation=0.0, floor_translation=0.0):
    p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
    r = np.ascontiguousarray(recs, dtype=api.POSE_COV_DTYPE).reshape(-1)
    tot = np.zeros(24)
    L.oeh_totals(_dp(p), r.ctypes.data_as(C.c_void_p), int(a), int(b), inflation, floor_rotation, floor_translation, _dp(tot))
    return tot
