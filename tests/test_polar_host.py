"""The geometry class of the host C++ mirror (liodom_amd/host) without a device: PolarGeometry::fromAngles / toC / layout, driven by a
stand-alone program (tests/polarhost.cc).  The tables are compared with NumPy's to one unit in the last place of a float: both
sides round a double sine or cosine to float once, and two correctly working libms may differ in the double's last bit, which
moves the rounded float by at most one step.  The layout is polarref's arithmetic; a table of the wrong length is refused."""
import os
import subprocess

import numpy as np
import pytest

import polarref

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(os.path.dirname(HERE), "liodom_amd", "host")
LIB = os.path.join(os.path.dirname(HERE), "liodom_amd", "lib")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def build_program(tmp_path):
    assert os.path.exists(os.path.join(HOST, "libliodom_host.so")), "libliodom_host.so not built (__graft_entry__.build())"
    exe = str(tmp_path / "polarhost")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(HERE, "polarhost.cc"), "-L" + HOST, "-lliodom_host",
                           "-L" + LIB, "-lliodom_hip", "-Wl,-rpath," + HOST, "-Wl,-rpath," + LIB])
    return exe


class Reader:
    def __init__(self, path):
        self.raw, self.at = open(path, "rb").read(), 0

    def take(self, dtype, n):
        a = np.frombuffer(self.raw, dtype, n, self.at)
        self.at += a.nbytes
        return a


def check_tables(rd, alt, enc, H, W, rb, ib):
    cos_alt, sin_alt, cos_baz, sin_baz = (rd.take(np.float32, H) for _ in range(4))
    cos_enc, sin_enc = rd.take(np.float32, W), rd.take(np.float32, W)
    lay = rd.take(np.int64, 4)
    refused = rd.take(np.int32, 1)[0]
    # fromAngles: a double sine / cosine rounded to float once
    for got, want in ((cos_alt, np.cos(alt)), (sin_alt, np.sin(alt)), (cos_enc, np.cos(enc)), (sin_enc, np.sin(enc))):
        w = want.astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - w) <= np.spacing(np.abs(w)).astype(np.float64)), "table differs by more than one float ulp"
    assert np.array_equal(u32(cos_baz), u32(np.ones(H))) and np.array_equal(u32(sin_baz), u32(np.zeros(H)))
    assert refused == 1, "fromAngles accepted an altitude table of the wrong length"
    # layout(): polarref's arithmetic
    assert tuple(int(v) for v in lay) == tuple(polarref.layout(H, W, rb, ib))


@pytest.mark.parametrize("H,W,rb,ib", [(16, 900, 16, 8), (128, 33, 32, 16), (5, 131, 16, 0), (1, 1, 32, 8)])
def test_from_angles_layout_and_refusal_without_a_device(tmp_path, H, W, rb, ib):
    exe = build_program(tmp_path)
    rng = np.random.default_rng(H * 1000 + W)
    alt, enc = rng.uniform(-0.5, 0.5, H), rng.uniform(-np.pi, np.pi, W)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(alt.tobytes() + enc.tobytes())
    subprocess.run([exe, str(fin), str(fout)] + [str(v) for v in (H, W, rb, ib)], check=True, timeout=60)
    rd = Reader(fout)
    check_tables(rd, alt, enc, H, W, rb, ib)
    assert rd.at == len(rd.raw)
