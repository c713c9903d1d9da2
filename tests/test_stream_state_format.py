"""The stream-state blob of liodom_export_stream_state (layout: csrc/kernels_state.h): api.parse_stream_state on a
blob assembled here from the documented layout, and the four entry points in the header and in the cross-compiled library.
CPU only; no compute calls."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["liodom_reset_stream", "liodom_stream_state_size", "liodom_export_stream_state", "liodom_import_stream_state"]


def assemble(P=5, frame_count=7, counts=(3, 1, 0, 2, 4), n_recv=0, mapping=0, use_imu=1, magic=b"LIODOMST", version=1, total=None):
    """A blob written field by field from the documented layout."""
    rng = np.random.default_rng(1)
    n_frames = len(counts)
    n_points = int(sum(counts))
    odom, prev, fin = (rng.normal(size=12) for _ in range(3))
    q, t, imu = rng.normal(size=4), rng.normal(size=3), rng.normal(size=4)
    pts = rng.normal(size=(n_points + n_recv, 4)).astype(np.float32)
    n_counts = (P + 3) // 4 * 4
    size = 64 + 416 + 4 * n_counts + 16 * (n_points + n_recv)
    header = magic + struct.pack("<IIQ", version, 64, size if total is None else total)
    header += struct.pack("<6I", P, mapping, 0, use_imu, 1, 0) + struct.pack("<4I", 0, 0, 0, 0)       # fingerprint, reserved
    assert len(header) == 64
    record = b"".join(np.asarray(a, "<f8").tobytes() for a in (odom, prev, fin, q, t))
    record += struct.pack("<5iI", 1, 0, frame_count, n_frames, frame_count, 6)                       # ..., scan_counter, status
    record += struct.pack("<4i", n_points, n_recv, use_imu, 0) + np.asarray(imu, "<f8").tobytes()
    assert len(record) == 416
    cnt = struct.pack("<%di" % n_counts, *(list(counts) + [0] * (n_counts - n_frames)))
    blob = header + record + cnt + pts.astype("<f4").tobytes()
    assert len(blob) == size
    return blob, dict(odom=odom, prev_odom=prev, final_odom=fin, param_q=q, param_t=t, imu_q=imu, pts=pts, n_points=n_points)


def test_parse_reads_every_documented_field():
    blob, want = assemble(n_recv=3, mapping=1)
    st = api.parse_stream_state(blob)
    assert st["version"] == 1 and st["total_bytes"] == len(blob)
    assert [st[k] for k in ("local_map_size", "mapping", "filter_local_map", "use_imu", "pose_rotation_mode", "lm_apply_step_on_ftol")] == [5, 1, 0, 1, 1, 0]
    for k in ("odom", "prev_odom", "final_odom"):
        assert st[k].shape == (3, 4) and np.array_equal(st[k].ravel(), want[k])
    assert np.array_equal(st["param_q"], want["param_q"]) and np.array_equal(st["param_t"], want["param_t"])
    assert np.array_equal(st["imu_q"], want["imu_q"]) and st["has_imu"] == 1
    assert (st["initialized"], st["append_raw"], st["frame_count"], st["n_frames"], st["scan_counter"], st["status"]) == (1, 0, 7, 5, 7, 6)
    # frames oldest first, back to back: the order of liodom_get_window
    assert list(st["frame_counts"]) == [3, 1, 0, 2, 4]
    assert np.array_equal(st["window"], want["pts"][:10]) and np.array_equal(st["received_map"], want["pts"][10:])
    assert [len(f) for f in st["frames"]] == [3, 1, 0, 2, 4]
    assert np.array_equal(st["frames"][0], want["pts"][0:3]) and np.array_equal(st["frames"][3], want["pts"][4:6])
    assert np.array_equal(st["frames"][4], want["pts"][6:10])


def test_parse_a_stream_that_never_ran():
    blob, _ = assemble(P=6, frame_count=0, counts=(), use_imu=0)
    st = api.parse_stream_state(blob)
    assert len(blob) == 64 + 416 + 4 * 8 and st["n_frames"] == 0 and st["frames"] == [] and st["window"].shape == (0, 4)


def test_parse_rejects_bad_magic_version_and_size():
    blob, _ = assemble()
    with pytest.raises(ValueError):
        api.parse_stream_state(bytes([blob[0] ^ 1]) + blob[1:])
    with pytest.raises(ValueError):
        api.parse_stream_state(assemble(version=2)[0])
    with pytest.raises(ValueError):
        api.parse_stream_state(blob[:-16])
    with pytest.raises(ValueError):
        api.parse_stream_state(blob[:200])
    with pytest.raises(ValueError):
        api.parse_stream_state(assemble(total=12345)[0])
    with pytest.raises(ValueError):
        api.parse_stream_state(blob + b"\0" * 16)


def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "liodom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*liodom_handle_t\s*\*" % name, src), "not declared: " + name
        assert name in api.EXPORTED_SYMBOLS
    la.build()
    L = C.CDLL(la.lib_path())
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export: " + name
    assert all(hasattr(la.Liodom, m) for m in ("reset_stream", "export_stream_state", "import_stream_state"))
