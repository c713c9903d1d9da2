"""The polar scan format on the host: the projection arithmetic of liodom_math.h (compiled into the stand-alone program
tests/polarcheck.cc) equals its NumPy restatement (tests/polarref.py) bit for bit on the designed blobs; the blob layout agrees
between polarref, polarcheck and liodom_polar_layout; the new entry points are exported.  CPU only."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import liodom_amd as la
import polarref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def polarcheck(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("polarcheck") / "polarcheck")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "polarcheck.cc")])
    return exe


def _host_project(exe, s, tmp_path):
    head = np.array([s.order, s.height, s.width, s.range_bits, s.intensity_bits, s.T], "<i4").tobytes()
    head += np.array([s.range_unit, s.beam_origin], "<f4").tobytes()
    tabs = b"".join(np.asarray(a, "<f4").tobytes() for a in (s.cos_alt, s.sin_alt, s.cos_baz, s.sin_baz, s.cos_enc, s.sin_enc))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(head + tabs + s.blob().tobytes())
    subprocess.check_call([exe, "project", str(fin), str(fout)])
    return np.fromfile(str(fout), "<f4").reshape(-1, 4)


@pytest.mark.parametrize("name", [r[0] for r in polarref.DESIGNED])
def test_host_projection_equals_reference_bitwise(polarcheck, tmp_path, name):
    s = polarref.designed(name)
    ref = polarref.project(s)
    got = _host_project(polarcheck, s, tmp_path)
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_designed_blobs_hold_the_special_values():
    """The designed blobs are what they claim: NaN columns from ticks T and 0xFFFFFFFF, NaN points from count 0 with w kept, the
    rounding count, both intensity extremes."""
    nan = polarref.NAN_BITS
    for name, order, H, W, rb, ib, T, nz in polarref.DESIGNED:
        s = polarref.designed(name)
        out = polarref.project(s)
        bits = out.view(np.uint32)
        i = np.arange(H * W)
        col = (i // H) if order == 0 else (i % W)
        if W >= 4:
            assert list(s.ticks[:4]) == [0, T - 1, T, 0xFFFFFFFF]
            for c in (2, 3):
                assert (bits[col == c, :3] == nan).all()
            assert not (bits[(col == 0) & (s.counts != 0), :3] == nan).any()
        zero = s.counts == 0
        assert zero.any() or H * W == 1
        assert (bits[zero, :3] == nan).all()
        if ib:
            assert np.array_equal(out[:, 3], s.intensities.astype(np.float32))
            assert s.intensities.max() == (1 << ib) - 1 and (s.intensities.min() == 0 or H * W == 1)
        else:
            assert (bits[:, 3] == 0).all()
        if rb == 32 and H * W > 4:
            assert ((1 << 24) + 1) in s.counts and 0xFFFFFFFF in s.counts
    # 2^24 + 1 is a tie and rounds to even, 2^32 - 1 rounds up to 2^32
    assert np.uint32((1 << 24) + 1).astype(np.float32) == np.float32(16777216.0)
    assert np.uint32(0xFFFFFFFF).astype(np.float32) == np.float32(4294967296.0)


def _geom(H, W, rb, ib):
    z = np.zeros(max(H, 1), np.float32)
    return la.polar_geometry(H, W, rb, ib, 0.002, 0.0, z, z, z, z, z[:1], z[:1])


def test_layout_agrees_for_every_width_combination(polarcheck):
    la.build()
    for (H, W), rb, ib in itertools.product([(1, 1), (5, 131), (16, 70), (128, 33), (64, 1800), (128, 2048), (3, 7)], (16, 32), (0, 8, 16)):
        want = polarref.layout(H, W, rb, ib)
        lay = la.polar_layout(_geom(H, W, rb, ib))
        assert (lay.tick_offset, lay.range_offset, lay.intensity_offset, lay.total_bytes) == want
        got = tuple(int(v) for v in subprocess.check_output([polarcheck, "layout", str(H), str(W), str(rb), str(ib)], text=True).split())
        assert got == want[1:]
        n = H * W
        assert all(o % 16 == 0 for o in want) and want[1] >= 4 * W and want[2] >= want[1] + n * rb // 8 and want[3] >= want[2] + n * ib // 8
        assert want[3] - (want[2] + n * ib // 8) < 16 and (ib != 0 or want[2] == want[3])
    # the HDL-64 blob: 7 KB of ticks + 230 KB of counts + 115 KB of intensities against 1.84 MB packed
    assert polarref.layout(64, 1800, 16, 8)[3] == 7200 + 230400 + 115200
    lay = la.api.PolarLayout()
    L = la.load()
    for bad in ((16, 70, 8, 8), (16, 70, 16, 4), (0, 70, 16, 8), (16, 0, 16, 8), (2049, 1, 16, 8)):
        assert L.liodom_polar_layout(C.byref(_geom(*bad)), C.byref(lay)) == la.api.ERR_INVALID_ARG


def test_polar_symbols_exported_and_bound():
    la.build()
    L = C.CDLL(la.lib_path())
    for n in ("liodom_polar_layout", "liodom_set_polar_geometry", "liodom_project_polar", "liodom_upload_scan_polar",
              "liodom_process_scan_polar", "liodom_scan_buffer_polar", "liodom_extract_edges_device_polar"):
        assert hasattr(L, n), "missing export: " + n
        assert n in la.api.EXPORTED_SYMBOLS
    for m in ("set_polar_geometry", "project_polar", "upload_scan_polar", "process_scan_polar", "scan_buffer_polar", "extract_edges_device_polar"):
        assert hasattr(la.Liodom, m)


def test_pack_polar_equals_reference_blob():
    for name in ("t0_16x70_r16_i8", "t1_128x33_r32_i8_bigT", "t1_5x131_r16_i0_T1"):
        s = polarref.designed(name)
        g = la.polar_geometry(s.height, s.width, s.range_bits, s.intensity_bits, s.range_unit, s.beam_origin, s.cos_alt, s.sin_alt,
                              s.cos_baz, s.sin_baz, s.cos_enc, s.sin_enc)
        assert g.ticks == s.T
        assert np.array_equal(la.pack_polar(g, s.ticks, s.counts, s.intensities), s.blob())


def test_geometry_from_angles_rounds_float64_tables_once():
    alt, baz, enc = np.linspace(-0.4, 0.3, 16), np.full(16, 0.02), 2 * np.pi * np.arange(70) / 70
    g = la.polar_geometry_from_angles(16, 70, alt, baz, enc, range_bits=32, intensity_bits=16, range_unit=0.001, beam_origin=0.015806)
    assert (g.height, g.width, g.range_bits, g.intensity_bits, g.ticks) == (16, 70, 32, 16, 70)
    assert np.array_equal(g.tables["sin_alt"], np.sin(alt).astype(np.float32)) and np.array_equal(g.tables["cos_enc"], np.cos(enc).astype(np.float32))
    assert np.array_equal(g.tables["sin_baz"], np.sin(baz).astype(np.float32))
    assert g.beam_origin == np.float32(0.015806) and g.range_unit == np.float32(0.001)


def test_quantised_generator_scan_is_a_workable_scene(synth):
    """The quantiser's projected cloud is the generator's to within 2 mm counts: 1 mm of range rounding plus the beam angles' fit."""
    for order, H, W in ((0, 16, 900), (1, 16, 512)):
        x, _ = synth.scan(synth.make_cfg(H, W, order), 0, 3)
        p = polarref.project(polarref.quantise(x, H, W, order))
        ok = np.isfinite(x[:, 0])
        assert np.array_equal(ok, np.isfinite(p[:, 0]))
        assert np.abs(p[ok, :3].astype(np.float64) - x[ok, :3]).max() < 2e-3
