"""The stream-state blob of liodom_export_stream_state (layout: csrc/stream_state_format.h): api.parse_stream_state
on a blob assembled here from the documented layout, the four entry points in the header and in the cross-compiled library, and
stream_state_validate as a stand-alone host program (tests/stream_state_validate_main.cc), built plain and under AddressSanitizer +
UBSan and run as a program: every named case of stream_state_cases.py, every prefix and every flipped byte of header, record and
counts.  CPU only; no compute calls, nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api
import stream_state_cases as ssc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["liodom_reset_stream", "liodom_stream_state_size", "liodom_export_stream_state", "liodom_import_stream_state"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}


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
    for src in ("stream_state_format.h", "pose7.h"):               # a change to either rebuilds the library
        assert os.path.join(ROOT, "liodom_amd", "csrc", src) in api._SRC


# ---- the validator as a program of its own ---------------------------------------------------------------------------------------
def good_blobs():
    """(good blob, the handle that takes it): local_map_size 5 (three padding entries behind the counts) and 8 (none), a mapping
    blob with a received map, and a stream whose window is not full yet.  Capacities somewhat above what the blob needs."""
    out = []
    for kw in (dict(), dict(P=8, frame_count=11, counts=(3, 1, 0, 2, 4, 1, 5, 2)), dict(n_recv=3, mapping=1), dict(frame_count=4, counts=(3, 1, 2, 4))):
        blob = assemble(**kw)[0]
        mapping = kw.get("mapping", 0)
        out.append((blob, ssc.Taker(ssc.fingerprint_of(blob), bool(mapping), 6, 4 if mapping else 0)))
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the validator program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("stream_state") / ("validate_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "stream_state_validate_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def _args(path, taker):
    return [str(path)] + [str(x) for x in taker.fingerprint] + [str(int(taker.mapping)), str(taker.edge_cap), str(taker.recv_cap)]


def test_validator_judges_every_named_case(exe, tmp_path):
    seen = set()
    for g, (good, taker) in enumerate(good_blobs()):
        for i, c in enumerate(ssc.cases(good, taker)):
            path = tmp_path / ("%d_%d.blob" % (g, i))
            path.write_bytes(c.blob)
            r = subprocess.run([exe, "judge"] + _args(path, c.taker), capture_output=True, text=True, timeout=60)
            assert r.returncode == 0 and not r.stderr, (c.name, r.stdout, r.stderr)
            code, _, why = r.stdout.strip().partition(" ")
            assert int(code) == c.code, (g, c.name, r.stdout)
            assert (why != "") == (c.code != ssc.OK), (g, c.name, r.stdout)
            seen.add(c.name)
    # every case the list can make has been made by one of the good blobs
    assert {"a count in a padding entry, the sum kept", "count 1 above edge_cap, count 3 negative", "n_recv 1, sizes consistent, mapping off",
            "n_recv equal to recv_cap", "recv_cap one below n_recv", "n_recv above recv_cap and a wrong sum"} <= seen, sorted(seen)


def test_validator_sweeps_prefixes_and_flipped_bytes(exe, tmp_path):
    for g, (good, taker) in enumerate(good_blobs()):
        path = tmp_path / ("good_%d.blob" % g)
        path.write_bytes(good)
        r = subprocess.run([exe, "sweep"] + _args(path, taker), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
        m = re.fullmatch(r"stream_state_validate: (\d+) cases, (\d+) flipped bytes refused, 0 failures", r.stdout.strip())
        head = 480 + 4 * ((taker.fingerprint[0] + 3) // 4 * 4)
        assert m and int(m.group(1)) == len(good) + 4 + head, r.stdout
        # what a flipped byte cannot break: reserved header words (16), the record's 47 doubles, status, has_imu and pad
        assert int(m.group(2)) == head - 16 - 8 * 47 - 12, r.stdout


def test_parse_accepts_every_accepted_case():
    n = 0
    for good, taker in good_blobs():
        for c in ssc.cases(good, taker):
            if c.code == ssc.OK:
                st = api.parse_stream_state(c.blob)
                assert st["total_bytes"] == len(c.blob) and st["local_map_size"] == taker.fingerprint[0], c.name
                n += 1
    assert n >= 19
