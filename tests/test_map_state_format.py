"""The map-state blob of liodom_map_export_state (layout: csrc/map_state_format.h): api.build_map_state and
api.parse_map_state against each other and against the oracle's cell keys, the four entry points in the header and in the
cross-compiled library, and map_state_validate as a stand-alone host program under AddressSanitizer and UBSan.
CPU only; no compute calls."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["liodom_map_state_size", "liodom_map_export_state", "liodom_map_import_state", "liodom_map_reset"]
SIZES = [(40.0, 50.0, 0.4), (10.0, 10.0, 0.25), (25.0, 30.0, 0.3)]


def cell_points(rng, n, corner, res):
    """n float32 points in the cell whose lower corner is `corner`, on an x-major lattice of 3-leaf steps well inside the cell."""
    i = np.arange(n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = corner[0] + res * (1.5 + 3 * (i % 8))
    p[:, 1] = corner[1] + res * (1.5 + 3 * ((i // 8) % 8))
    p[:, 2] = corner[2] + res * (1.5 + 3 * (i // 64))
    p[:, 3] = rng.uniform(0, 100, n)
    return p


def three_cells(sizes, counts=(1, 255, 257), corners=((0, 0, 0), (1, 0, 0), (0, -1, 0))):
    xy, z, res = sizes
    rng = np.random.default_rng(3)
    return [cell_points(rng, n, (c[0] * xy, c[1] * xy, c[2] * z), res) for n, c in zip(counts, corners)]


def check_round_trip(sizes, cells, status=0):
    xy, z, res = sizes
    blob = api.build_map_state(xy, z, res, cells, status=status)
    n_points = sum(len(c) for c in cells)
    assert len(blob) == 64 + 32 * len(cells) + 16 * n_points
    st = api.parse_map_state(blob, sizes=sizes)
    assert st["version"] == 1 and st["total_bytes"] == len(blob) and st["status"] == status
    assert (st["voxel_xysize"], st["voxel_zsize"], st["resolution"]) == (xy, z, res)
    assert st["keys"].shape == (len(cells), 3) and st["corner_leaf"].shape == (len(cells), 3)
    assert list(st["counts"]) == [len(c) for c in cells] and len(st["cells"]) == len(cells)
    for c, got, key, corner in zip(cells, st["cells"], st["keys"], st["corner_leaf"]):
        assert np.array_equal(got.view(np.uint32), np.asarray(c, np.float32).view(np.uint32))
        assert list(key) == api.map_cell_key(c[0, :3], xy, z)
        assert list(corner) == api.map_cell_corner_leaf(c[0, :3], xy, z, res)
    want = np.concatenate(cells) if cells else np.zeros((0, 4), np.float32)
    assert st["points"].shape == (n_points, 4) and np.array_equal(st["points"].view(np.uint32), want.view(np.uint32))
    return blob, st


@pytest.mark.parametrize("sizes", SIZES)
def test_build_then_parse_returns_the_input(sizes):
    xy, z, res = sizes
    rng = np.random.default_rng(5)
    blob, st = check_round_trip(sizes, [])
    assert len(blob) == 64 and st["points"].shape == (0, 4) and st["cells"] == []
    check_round_trip(sizes, [np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)])
    blob, st = check_round_trip(sizes, three_cells(sizes), status=8 | 64)
    assert len(blob) == 64 + 96 + 16 * 513
    # documented key values: int(floor(x / size) * size + size / 2), corner = leaf of the cell's lower corner
    assert list(st["keys"][0]) == [int(xy / 2), int(xy / 2), int(z / 2)] and list(st["keys"][1]) == [int(xy + xy / 2), int(xy / 2), int(z / 2)]
    assert list(st["corner_leaf"][0]) == [0, 0, 0]
    # keys negative on every axis, and far out
    neg = [cell_points(rng, 3, (-xy, -2 * xy, -z), res), cell_points(rng, 2, (-1000 * xy, -xy, -3 * z), res)]
    _, st = check_round_trip(sizes, neg)
    assert (st["keys"] < 0).all() and (st["corner_leaf"] < 0).all()
    assert list(st["keys"][0]) == [int(-xy + xy / 2), int(-2 * xy + xy / 2), int(-z + z / 2)]
    # first = exclusive prefix sum of count, records in creation order
    rec = np.frombuffer(blob, "<i4", 8 * 3, 64).reshape(3, 8)
    assert list(rec[:, 6]) == [1, 255, 257] and list(rec[:, 7]) == [0, 1, 256]
    with pytest.raises(ValueError):
        api.build_map_state(xy, z, res, [np.zeros((0, 4), np.float32)])


@pytest.mark.parametrize("sizes", SIZES)
def test_keys_are_the_oracles(orc, sizes):
    """Points on cell faces, just beside them and inside, on both sides of 0, grouped by build_map_state's key in
    first-appearance order and fed to the oracle's Map one group at a time: every group makes exactly one new cell (so the
    oracle gives all its points one key, and another key than every earlier group), and getMap is the groups back to back."""
    xy, z, res = sizes
    pts = []
    for kx in (-3, -2, -1, 0, 1, 2):
        for ky in (-1, 0):
            for kz in (-1, 0):
                x0, y, zz = kx * xy, ky * xy + 0.3 * xy, kz * z + 0.3 * z
                for x in (x0, np.nextafter(np.float32(x0), np.float32(-1e9)), np.nextafter(np.float32(x0), np.float32(1e9)),
                          x0 + 4.5 * res, x0 + 9.5 * res, x0 + xy - 4.5 * res):
                    pts.append((x, y, zz, float(len(pts))))
    pts = np.array(pts, np.float32)
    groups, order = {}, []
    for p in pts:
        k = tuple(api.map_cell_key(p[:3], xy, z))
        if k not in groups:
            groups[k] = []
            order.append(k)
        groups[k].append(p)
    cells = []
    for k in order:
        g = np.array(groups[k], np.float32)
        g = g[np.argsort(g[:, 0], kind="stable")]
        # one point per leaf, ascending leaf order (x is the fastest leaf axis; y and z are shared): what a cell's cloud looks like
        leaf = np.floor(g[:, 0] * (np.float32(1.0) / np.float32(res)))
        g = g[np.concatenate([[True], np.diff(leaf) > 0])]
        cells.append(g)
    assert len(cells) >= 24
    st = api.parse_map_state(api.build_map_state(xy, z, res, cells))
    assert [tuple(k) for k in st["keys"]] == [tuple(api.map_cell_key(c[0, :3], xy, z)) for c in cells]
    mo = orc.Map(xy, z, res)
    for i, c in enumerate(cells):
        mo.update(c)
        assert mo.num_cells() == i + 1, (i, order[i])
    got = mo.all()
    assert np.array_equal(got.view(np.uint32), st["points"].view(np.uint32))


def _patched(blob, off, fmt, value):
    return blob[:off] + struct.pack(fmt, value) + blob[off + struct.calcsize(fmt):]


def test_parse_rejects_what_the_validator_rejects():
    sizes = SIZES[0]
    blob = api.build_map_state(*sizes, three_cells(sizes))
    api.parse_map_state(blob, sizes=sizes)
    rec = lambda c, field: 64 + 32 * c + 4 * field      # noqa: E731   fields: key 0-2, corner_leaf 3-5, count 6, first 7
    bad = {
        "empty": b"",
        "truncated header": blob[:63],
        "truncated records": blob[:100],
        "truncated points": blob[:-1],
        "one point short": blob[:-16],
        "too long": blob + b"\0" * 16,
        "magic": b"LIODOMST" + blob[8:],
        "version": _patched(blob, 8, "<I", 2),
        "header_bytes": _patched(blob, 12, "<I", 128),
        "total_bytes": _patched(blob, 16, "<Q", len(blob) + 16),
        "n_cells": _patched(blob, 48, "<i", 4),
        "n_cells negative": _patched(blob, 48, "<i", -1),
        "n_cells huge": _patched(blob, 48, "<i", 2 ** 31 - 1),
        "n_points": _patched(blob, 56, "<q", 512),
        "n_points negative": _patched(blob, 56, "<q", -1),
        "count negative": _patched(blob, rec(1, 6), "<i", -1),
        "count huge": _patched(blob, rec(1, 6), "<i", 2 ** 31 - 1),
        "first not the prefix": _patched(blob, rec(2, 7), "<i", 255),
        "first negative": _patched(blob, rec(0, 7), "<i", -1),
        "first huge": _patched(blob, rec(2, 7), "<i", 2 ** 31 - 1),
        "counts do not add up": _patched(blob, rec(2, 6), "<i", 258),
        "key 2^20": _patched(blob, rec(1, 0), "<i", 1 << 20),
        "key -2^20 - 1": _patched(blob, rec(1, 2), "<i", -(1 << 20) - 1),
        "duplicate key": blob[:rec(2, 0)] + blob[rec(0, 0):rec(0, 3)] + blob[rec(2, 3):],
    }
    for name, b in bad.items():
        assert len(b) != len(blob) or b != blob, name
        with pytest.raises(ValueError):
            api.parse_map_state(b)
            pytest.fail("accepted: " + name)
    # the fingerprint must match bit for bit
    for other in ((40.0, 50.0, 0.4 + 1e-12), (40.0, 50.000000000000007, 0.4), (10.0, 50.0, 0.4)):
        with pytest.raises(ValueError):
            api.parse_map_state(blob, sizes=other)
    # the limits themselves are keys
    ok = _patched(_patched(blob, rec(1, 0), "<i", -(1 << 20)), rec(1, 1), "<i", (1 << 20) - 1)
    assert list(api.parse_map_state(ok)["keys"][1][:2]) == [-(1 << 20), (1 << 20) - 1]


def test_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "liodom_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*liodom_map_t\s*\*" % name, src), "not declared: " + name
        assert name in api.EXPORTED_SYMBOLS
    la.build()
    L = C.CDLL(la.lib_path())
    for name in SYMBOLS:
        assert hasattr(L, name), "missing export: " + name
    assert all(hasattr(la.Map, m) for m in ("state_size", "export_state", "import_state", "reset"))
    assert os.path.join(ROOT, "liodom_amd", "csrc", "map_state_format.h") in api._SRC


def test_validator_stand_alone_under_host_sanitizers(tmp_path):
    """map_state_validate compiled for the host alone with ASan + UBSan into a program of its own (tests/map_state_validate_main.cc),
    which derives every hostile blob from a good one — each truncation length, each header field, counts and firsts at the int32
    limits, duplicate keys, n_cells = INT32_MAX — and expects the documented return code; any read beyond `bytes` is a sanitizer
    error and fails the run."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the validator's driver"
    exe = str(tmp_path / "map_state_validate")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "map_state_validate_main.cc")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sizes = SIZES[2]
    good = tmp_path / "good.mapstate"
    good.write_bytes(api.build_map_state(*sizes, three_cells(sizes)))
    r = subprocess.run([exe, str(good)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"map_state_validate: \d{4,} cases, 0 failures", r.stdout), r.stdout
