"""The place-state blob of liodom_places_export_state (layout: csrc/place_state_format.h): api.build_place_state and
api.parse_place_state against each other, and place_state_validate as a stand-alone host program (tests/place_state_validate_main.cc),
built plain and under AddressSanitizer + UBSan and run as a program: well-formed blobs and each malformed one.  No GPU, nothing
sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from liodom_amd import api
import place_designed as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
GEOMS = [api.place_geometry(2, 2, 30.0, -1.0, 5.0), api.place_geometry(), api.place_geometry(7, 9, 80.0, -3.0, 15.0)]
_EXE = {}


def good_blob(geom, n=3, seed=4):
    rng = np.random.default_rng(seed)
    W = geom[0] * geom[1]
    desc = pd.random_desc(rng, n, W, density=0.2)
    return api.build_place_state(geom, desc, np.arange(100, 100 + n), pd.poses_for(n)), desc


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the validator program"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("place_state") / ("validate_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "place_state_validate_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


@pytest.mark.parametrize("geom", GEOMS[:2])
def test_validator_on_well_formed_and_malformed_blobs(exe, geom, tmp_path):
    blob, _ = good_blob(geom)
    path = tmp_path / "good.blob"
    path.write_bytes(blob)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and int(r.stdout.split()[1]) > 1000


@pytest.mark.parametrize("geom", GEOMS)
def test_build_then_parse_returns_the_input(geom):
    W = geom[0] * geom[1]
    blob, desc = good_blob(geom, n=5)
    assert len(blob) == 64 + 656 + (8 * W + 72) * 5
    st = api.parse_place_state(blob, geom=geom)
    assert st["version"] == 1 and st["total_bytes"] == len(blob) and st["geometry"] == geom and st["count"] == 5
    assert np.array_equal(st["desc"], desc) and list(st["ids"]) == [100, 101, 102, 103, 104]
    assert np.array_equal(st["bits"], np.bitwise_count(desc).sum(axis=1)) and np.array_equal(st["poses"], pd.poses_for(5))
    t = api.place_tables(geom)
    assert all(np.array_equal(st["tables"][k], t[k]) for k in "CSZ") and np.array_equal(st["tables"]["R2"], t["R2"])
    raw = np.frombuffer(blob, "<f4", 164, 64)
    assert np.array_equal(raw[0:15], t["C"]) and np.array_equal(raw[16:31], t["S"]) and raw[15] == raw[31] == 0
    assert np.array_equal(raw[32:32 + geom[0]], t["R2"]) and not raw[32 + geom[0]:96].any()
    assert np.array_equal(raw[96:97 + geom[1]], t["Z"]) and not raw[97 + geom[1]:].any()
    empty = api.build_place_state(geom, np.zeros((0, W), np.uint64), [], np.zeros((0, 7)))
    assert len(empty) == 720 and api.parse_place_state(empty)["count"] == 0


def test_parse_rejects_what_the_validator_rejects():
    geom = GEOMS[0]
    blob, _ = good_blob(geom)
    recs = 720 + 8 * 4 * 3

    def bad(b, **kw):
        with pytest.raises(ValueError):
            api.parse_place_state(bytes(b), **kw)

    for cut in (0, 63, 64, 719, 720, len(blob) - 1):
        bad(blob[:cut])
    bad(b"LIODOMMP" + blob[8:])
    bad(blob + b"\0" * 8)
    for off, val in ((8, np.array([2], "<u4")), (12, np.array([65], "<u4")), (16, np.array([len(blob) + 1], "<u8")), (24, np.array([65], "<i4")),
                     (24, np.array([0], "<i4")), (28, np.array([33], "<i4")), (32, np.array([np.nan], "<f8")), (32, np.array([31.0], "<f8")),
                     (40, np.array([5.0], "<f8")), (56, np.array([2], "<i4")), (60, np.array([1], "<i4")), (64 + 4, np.array([0.5], "<f4")),
                     (64 + 60, np.array([1.0], "<f4")), (720, np.array([0], "<u8")), (recs + 8, np.array([-1], "<i4")),
                     (recs + 12, np.array([1], "<i4")), (recs + 16, np.array([np.inf], "<f8")), (recs + 72 + 16 + 8 * 6, np.array([np.nan], "<f8")),
                     (recs + 16 + 24, np.array([1.1], "<f8"))):
        b = bytearray(blob)
        b[off:off + val.nbytes] = val.tobytes()
        bad(b)
    bad(blob, geom=api.place_geometry(2, 2, 30.0, -1.0, 5.0000000001))
    bad(blob, geom=api.place_geometry(4, 1, 30.0, -1.0, 5.0))
    assert api.parse_place_state(blob, geom=geom)["count"] == 3
