"""Export, import and reset of the device map (liodom_map_state_size / _export_state / _import_state / _reset): round trips
into maps of other capacities with bit-identical continuation against the CPU oracle, blobs designed with api.build_map_state
(which pin the unpack and clear kernels independently of the pack kernel), rejections that leave the map as it was, and the
checkpoint of a mapping-mode stream."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import liodom_amd as la
from liodom_amd import api

pytestmark = pytest.mark.gpu

SZ = (40.0, 50.0, 0.4)


def P(*rows):
    a = np.zeros((len(rows), 4), np.float32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pose(yaw, t):
    T = np.eye(4)[:3].copy()
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:, 3] = t
    return T


def clustered_update(rng, k, res, n_max=600):
    """The generator of test_gpu_map.test_random_updates_bit_exact, scaled down: clustered points so that many share a leaf,
    some exactly on leaf / cell boundaries, under a moving pose."""
    n = int(rng.integers(1, n_max))
    centres = rng.uniform(-12, 12, size=(16, 3)) * [1, 1, 0.2]
    pts = centres[rng.integers(0, 16, n)] + rng.normal(0, 0.35, size=(n, 3))
    pts[: n // 20] = np.round(pts[: n // 20] / res) * res
    x = np.zeros((n, 4), np.float32)
    x[:, :3] = pts
    x[:, 3] = rng.uniform(0, 100, n)
    return x, pose(0.02 * k, [0.8 * k, 0.1 * k, 0.01 * k])


def cell_points(rng, n, corner, res):
    """n float32 points of the cell with lower corner `corner`: one per leaf, ascending leaf order (x fastest), 3-leaf steps."""
    i = np.arange(n)
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = corner[0] + res * (1.5 + 3 * (i % 8))
    p[:, 1] = corner[1] + res * (1.5 + 3 * ((i // 8) % 8))
    p[:, 2] = corner[2] + res * (1.5 + 3 * (i // 64))
    p[:, 3] = rng.uniform(0, 100, n)
    return p


def snapshot(m):
    return m.all(), m.num_cells(), m.status()


def same_snapshot(a, b):
    return same(a[0], b[0]) and a[1:] == b[1:]


# ---------------------------------------------------------------------------------------------
# 1. round trip into a map of other capacities, and continuation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(10.0, 10.0, 0.25), SZ])
def test_round_trip_and_continuation(orc, sizes):
    xy, z, res = sizes
    rng = np.random.default_rng(11)
    mo = orc.Map(xy, z, res)
    mg = la.Map(xy, z, res, max_cells=512, cell_capacity=8192, max_update_points=1024, max_modified_cells=128)
    for k in range(8):
        x, T = clustered_update(rng, k, res)
        mo.update(x, T); mg.update(x, T)
    assert mg.status() == 0 and same(mg.all(), mo.all()) and mg.num_cells() > 3
    blob = mg.export_state()
    assert len(blob) == mg.state_size() == 64 + 32 * mg.num_cells() + 16 * mg.all().shape[0]
    st = api.parse_map_state(blob, sizes=sizes)
    assert same(st["points"], mo.all()) and len(st["cells"]) == mo.num_cells() and st["status"] == 0
    assert list(st["counts"][:3]) == [len(c) for c in st["cells"][:3]]
    mi = la.Map(xy, z, res, max_cells=96, cell_capacity=4096, max_update_points=640, max_modified_cells=64)
    mi.update(P((3.0, 3.0, 3.0, 1.0), (-300.0, 3.0, 3.0, 1.0)))      # what the map held before the import is gone afterwards
    mi.import_state(blob)
    assert mi.export_state() == blob
    Ts = [T, pose(0.0, [0.0, 0.0, 0.0]), pose(1.0, [-9.0, 11.0, 1.0])]
    for Tq in Ts:
        assert same(mi.local(Tq, 2, 1), mg.local(Tq, 2, 1)) and same(mi.local(Tq, 1, 0), mg.local(Tq, 1, 0))
    assert same_snapshot(snapshot(mi), snapshot(mg))
    for k in range(8, 14):
        x, T = clustered_update(rng, k, res)
        mo.update(x, T); mg.update(x, T); mi.update(x, T)
        a = mo.all()
        assert same(mg.all(), a) and same(mi.all(), a), k
        assert mi.num_cells() == mg.num_cells() == mo.num_cells(), k
        ref = mo.local(T, 2, 1)
        assert same(mg.local(T, 2, 1), ref) and same(mi.local(T, 2, 1), ref), k
        assert same(mi.local(T, 1, 0), mo.local(T, 1, 0)), k
    assert mi.status() == 0 and mg.status() == 0
    assert mi.export_state() == mg.export_state()
    mg.close(); mi.close()


# ---------------------------------------------------------------------------------------------
# 2. designed blobs: no update and no export made them
# ---------------------------------------------------------------------------------------------
def _designed_cases():
    xy, z, res = SZ
    rng = np.random.default_rng(2)
    corner = lambda kx, ky, kz: (kx * xy, ky * xy, kz * z)      # noqa: E731
    return {
        "0 cells": ([], dict(max_cells=8, cell_capacity=64)),
        "1 cell of 1 point": ([P((1.0, 2.0, 3.0, 4.0))], dict(max_cells=8, cell_capacity=64)),
        "count == cell_capacity": ([cell_points(rng, 5, corner(0, 0, 0), res), cell_points(rng, 300, corner(1, 0, 0), res)],
                                   dict(max_cells=8, cell_capacity=300)),
        "n_cells == max_cells": ([cell_points(rng, 3 + i, corner(i, -i, 0), res) for i in range(7)], dict(max_cells=7, cell_capacity=64)),
        "255, 256, 257 points": ([cell_points(rng, n, corner(i, 0, 0), res) for i, n in enumerate((255, 256, 257))],
                                 dict(max_cells=8, cell_capacity=512)),
        "negative keys": ([cell_points(rng, 9, corner(-1, -2, -1), res), cell_points(rng, 70, corner(-3, -1, -2), res)],
                          dict(max_cells=8, cell_capacity=128)),
        "a key above 10^6": ([cell_points(rng, 4, corner(0, 0, 0), res), cell_points(rng, 66, corner(26000, -1, 0), res)],
                             dict(max_cells=8, cell_capacity=128)),
    }


@pytest.mark.parametrize("case", list(_designed_cases()))
def test_designed_blob_imports_and_exports_byte_for_byte(case):
    xy, z, res = SZ
    cells, caps = _designed_cases()[case]
    blob = api.build_map_state(xy, z, res, cells)
    want = np.concatenate(cells) if cells else np.zeros((0, 4), np.float32)
    if case == "a key above 10^6":
        assert abs(api.parse_map_state(blob)["keys"]).max() > 10 ** 6
    mg = la.Map(xy, z, res, max_update_points=256, max_modified_cells=8, **caps)
    mg.update(P((7.0, 7.0, 7.0, 7.0), (-70.0, 7.0, 7.0, 7.0)))      # something to clear
    mg.import_state(blob)
    assert mg.num_cells() == len(cells) and mg.status() == 0
    assert same(mg.all(), want)
    assert mg.state_size() == len(blob) and mg.export_state() == blob
    # every cell is found through the hash: the xy loop of getLocalMap(0, 0) at a cell's first point starts with that cell
    for c in cells:
        T = pose(0.0, [float(int(c[0, 0])), float(int(c[0, 1])), float(int(c[0, 2]))])
        assert same(mg.local(T, 0, 0)[:len(c)], c), case
    assert mg.status() == 0
    mg.close()


def test_three_hundred_cells_then_updates_against_the_oracle(orc):
    """More cells than one update can create (kMapNewCellsMax = 256) come in through one import; then updates that find
    imported cells through the hash, merge into an imported single-point leaf and create cells whose ids go on at 300."""
    xy, z, res = SZ
    pts = P(*[(i * xy + 20.2, j * xy + 20.2, 1.0, float(i * 15 + j)) for i in range(20) for j in range(15)])
    assert len(pts) == 300
    blob = api.build_map_state(xy, z, res, [pts[i:i + 1] for i in range(300)])
    mo = orc.Map(xy, z, res)
    for i in range(0, 300, 100):
        mo.update(pts[i:i + 100])
    mg = la.Map(xy, z, res, max_cells=512, cell_capacity=64, max_update_points=256, max_modified_cells=128)
    mg.import_state(blob)
    assert mg.num_cells() == mo.num_cells() == 300 and same(mg.all(), mo.all()) and mg.export_state() == blob

    def both(x, T=None):
        mo.update(x, T); mg.update(x, T)
        assert mg.num_cells() == mo.num_cells()
        assert same(mg.all(), mo.all())
        for Tq in (pose(0.0, [25.0, 25.0, 1.0]), pose(0.0, [20 * xy + 5, 30.0, 1.0]), pose(0.3, [400.0, 300.0, 2.0])):
            assert same(mg.local(Tq, 2, 1), mo.local(Tq, 2, 1))

    a = pts[::3].copy(); a[:, 0] += 5.0; a[:, 3] += 1000.0           # imported cells through the hash, other leaves
    both(a)
    assert mg.num_cells() == 300
    b = pts[1::4].copy(); b[:, :3] += 0.05; b[:, 3] += 2000.0        # the imported points' own leaves: centroids of two
    both(b, pose(0.0, [0.0, 0.0, 0.0]))
    assert mg.num_cells() == 300 and mg.all().shape[0] == 300 + len(a)
    c = P(*[(20 * xy + 20.2 + xy * i, 20.2, 1.0, 3000.0 + i) for i in range(40)] + [(45.0, 25.0, 1.0, 1.0)])      # new cells (+ an old one)
    both(c)
    assert mg.num_cells() == 340
    assert same(mg.all()[-40:], c[:40])                              # ids continue at 300: the new cells come last, in input order
    assert mg.status() == 0
    mg.close()


# ---------------------------------------------------------------------------------------------
# 3. rejections leave the map as it was
# ---------------------------------------------------------------------------------------------
def _patched(blob, off, fmt, value):
    return blob[:off] + struct.pack(fmt, value) + blob[off + struct.calcsize(fmt):]


def _mapping_handle():
    H, W = 16, 900
    return la.Liodom(la.make_params(scan_lines=H, scan_regions=6, edges_per_region=10, prev_frames=4, mapping=1),
                     la.make_config(max_points=H * W, max_width=W, recv_capacity=1 << 16))


def test_rejections_leave_the_map_untouched():
    xy, z, res = SZ
    rng = np.random.default_rng(4)
    mg = la.Map(xy, z, res, max_cells=8, cell_capacity=1024, max_update_points=1024, max_modified_cells=8)
    for k in range(2):
        mg.update(*clustered_update(rng, k, res))
    before = snapshot(mg)
    assert before[1] >= 3 and before[2] == 0
    blob = mg.export_state()
    rec = lambda c, field: 64 + 32 * c + 4 * field      # noqa: E731   fields: key 0-2, corner_leaf 3-5, count 6, first 7
    n1 = struct.unpack_from("<i", blob, rec(1, 6))[0]
    invalid = {
        "empty": b"",
        "truncated header": blob[:63],
        "truncated records": blob[:100],
        "one byte short": blob[:-1],
        "one point short": blob[:-16],
        "too long": blob + b"\0" * 16,
        "magic": b"LIODOMST" + blob[8:],
        "version": _patched(blob, 8, "<I", 2),
        "header_bytes": _patched(blob, 12, "<I", 128),
        "total_bytes": _patched(blob, 16, "<Q", len(blob) + 16),
        "n_cells": _patched(blob, 48, "<i", before[1] + 1),
        "n_cells huge": _patched(blob, 48, "<i", 2 ** 31 - 1),
        "n_points": _patched(blob, 56, "<q", before[0].shape[0] - 1),
        "count negative": _patched(blob, rec(1, 6), "<i", -1),
        "count huge": _patched(blob, rec(1, 6), "<i", 2 ** 31 - 1),
        "first not the prefix": _patched(blob, rec(1, 7), "<i", struct.unpack_from("<i", blob, rec(1, 7))[0] + 1),
        "first huge": _patched(blob, rec(2, 7), "<i", 2 ** 31 - 1),
        "counts do not add up": _patched(blob, rec(before[1] - 1, 6), "<i", struct.unpack_from("<i", blob, rec(before[1] - 1, 6))[0] + 1),
        "counts moved": _patched(_patched(blob, rec(0, 6), "<i", struct.unpack_from("<i", blob, rec(0, 6))[0] + 1), rec(1, 6), "<i", n1 - 1),
        "key 2^20": _patched(blob, rec(1, 0), "<i", 1 << 20),
        "key -2^20 - 1": _patched(blob, rec(1, 2), "<i", -(1 << 20) - 1),
        "duplicate key": blob[:rec(2, 0)] + blob[rec(0, 0):rec(0, 3)] + blob[rec(2, 3):],
        "other resolution": api.build_map_state(xy, z, 0.5, [P((1.0, 1.0, 1.0, 1.0))]),
        "other xy size": api.build_map_state(np.nextafter(xy, 100.0), z, res, [P((1.0, 1.0, 1.0, 1.0))]),
        "other z size": api.build_map_state(xy, 25.0, res, []),
    }
    capacity = {
        "more cells than max_cells": api.build_map_state(xy, z, res, [P((i * xy + 1.0, 1.0, 1.0, 1.0)) for i in range(9)]),
        "a cell larger than cell_capacity": api.build_map_state(xy, z, res, [P((1.0, 1.0, 1.0, 1.0)), cell_points(rng, 1025, (xy, 0, 0), res)]),
    }
    for want, cases in ((api.ERR_INVALID_ARG, invalid), (api.ERR_CAPACITY, capacity)):
        for name, b in cases.items():
            with pytest.raises(la.LiodomError) as e:
                mg.import_state(b)
            assert e.value.code == want, (name, str(e.value))
            assert "liodom_map_import_state: " in str(e.value) and len(str(e.value)) > 50, name
            assert same_snapshot(snapshot(mg), before), name
    assert mg.export_state() == blob

    # export into a buffer one byte short: the size needed, and nothing written
    L = la.load()
    need = len(blob)
    buf = (C.c_ubyte * need)(*([0xAB] * need))
    n = C.c_int64(0)
    assert L.liodom_map_export_state(mg.h, buf, need - 1, C.byref(n)) == api.ERR_CAPACITY and n.value == need
    assert bytes(buf) == b"\xab" * need
    assert L.liodom_map_export_state(mg.h, buf, need, C.byref(n)) == 0 and n.value == need and bytes(buf) == blob

    # attached: export works, import and reset are refused until the map is detached
    g = _mapping_handle()
    g.attach_mapper(mg, 2, 1)
    assert mg.export_state() == blob and mg.state_size() == need
    for call in (lambda: mg.import_state(blob), mg.reset):
        with pytest.raises(la.LiodomError) as e:
            call()
        assert e.value.code == api.ERR_BUSY
    assert same_snapshot(snapshot(mg), before)
    g.attach_mapper(None)
    mg.import_state(blob)
    assert same_snapshot(snapshot(mg), before)
    mg.reset()
    assert snapshot(mg)[1:] == (0, 0) and mg.all().shape == (0, 4)
    g.close()
    mg.close()


# ---------------------------------------------------------------------------------------------
# 4. reset, 5. the status bits travel
# ---------------------------------------------------------------------------------------------
def test_reset_gives_a_fresh_map(orc):
    xy, z, res = 25.0, 30.0, 0.3
    caps = dict(max_cells=128, cell_capacity=4096, max_update_points=1024, max_modified_cells=64)
    mg, mf, mo = la.Map(xy, z, res, **caps), la.Map(xy, z, res, **caps), orc.Map(xy, z, res)
    rng = np.random.default_rng(9)
    ups = [clustered_update(rng, k, res) for k in range(5)]
    for x, T in ups[::-1]:                      # another order first: other cell ids, other hash slots, both slabs in use
        mg.update(x, T)
    assert mg.num_cells() > 3 and mg.all().shape[0] > 100
    mg.reset()
    assert mg.num_cells() == 0 and mg.all().shape == (0, 4) and mg.status() == 0
    assert mg.local(ups[0][1], 2, 1).shape == (0, 4) and mg.state_size() == 64
    assert mg.export_state() == api.build_map_state(xy, z, res, [])
    for k, (x, T) in enumerate(ups):
        for m in (mg, mf, mo):
            m.update(x, T)
        a = mo.all()
        assert same(mg.all(), a) and same(mf.all(), a), k
        assert mg.num_cells() == mf.num_cells() == mo.num_cells(), k
        assert same(mg.local(T, 2, 1), mo.local(T, 2, 1)), k
    assert mg.status() == 0 and mg.export_state() == mf.export_state()
    mg.import_state(api.build_map_state(xy, z, res, []))      # a blob of 0 cells is a reset
    assert snapshot(mg)[1:] == (0, 0) and mg.all().shape == (0, 4)
    mg.close(); mf.close()


def _overflowed_map():
    """test_gpu_map.test_capacity_overflow_is_reported's recipe: 98 distinct leaves into a cell of capacity 64."""
    mg = la.Map(40.0, 50.0, 0.4, max_cells=4, cell_capacity=64, max_update_points=256, max_modified_cells=4)
    x = np.zeros((200, 4), np.float32)
    x[:, 0] = np.linspace(0, 39, 200)
    mg.update(x)
    assert mg.status() & 8
    return mg


def test_reset_clears_and_export_carries_the_status_bits():
    mg = _overflowed_map()
    blob = mg.export_state()
    st = api.parse_map_state(blob, sizes=SZ)
    assert st["status"] == mg.status() and st["status"] & 8 and list(st["counts"]) == [64]
    mi = la.Map(40.0, 50.0, 0.4, max_cells=16, cell_capacity=100, max_update_points=64, max_modified_cells=4)
    assert mi.status() == 0
    mi.import_state(blob)
    assert mi.status() == mg.status() and same(mi.all(), mg.all()) and mi.export_state() == blob
    mg.reset()
    assert mg.status() == 0 and mg.num_cells() == 0 and mg.all().shape == (0, 4)
    mi.import_state(api.build_map_state(40.0, 50.0, 0.4, [], status=8))      # 0 cells, and still the bits travel
    assert mi.status() == 8 and mi.num_cells() == 0
    mg.close(); mi.close()


# ---------------------------------------------------------------------------------------------
# 6. checkpoint of a mapping-mode stream: stream state + map state
# ---------------------------------------------------------------------------------------------
def test_checkpoint_of_a_mapping_mode_run(synth):
    H, W, K = 16, 900, 8
    cfg = synth.make_cfg(H, W, 0)
    scans = [synth.scan(cfg, 0, k)[0] for k in range(K)]
    caps = dict(max_cells=128, cell_capacity=16384)
    g1, m1 = _mapping_handle(), la.Map(**caps)
    g1.attach_mapper(m1, 2, 1)
    full, saved = [], None
    for k in range(K):
        p, _ = g1.process_scan(scans[k], H, W)
        full.append((p.copy(), g1.received_map(), m1.all()))
        if k == 3:      # after scan 4: the stream, and the map while it is still attached
            saved = (g1.export_stream_state(0), m1.export_state())
    assert m1.status() == 0 and full[-1][2].shape[0] > 100 and len(full[3][1]) > 0
    g1.attach_mapper(None)
    g1.close(); m1.close()
    g2, m2 = _mapping_handle(), la.Map(max_cells=96, cell_capacity=32768)
    m2.import_state(saved[1])
    g2.import_stream_state(0, saved[0])
    g2.attach_mapper(m2, 2, 1)
    assert same(m2.all(), full[3][2]) and same(g2.received_map(), full[3][1])
    for k in range(4, K):
        p, _ = g2.process_scan(scans[k], H, W)
        assert np.array_equal(p, full[k][0]), k
        assert same(g2.received_map(), full[k][1]), k
        assert same(m2.all(), full[k][2]), k
    assert m2.status() == 0
    g2.attach_mapper(None)
    g2.close(); m2.close()


# ---------------------------------------------------------------------------------------------
# 7. replay harness: map_state_out= / map_state_in=
# ---------------------------------------------------------------------------------------------
def test_replay_harness_saves_and_loads_the_map_state(orc, synth, tmp_path):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "liodom_amd", "host", "liodom_replay")
    if not os.path.exists(exe):
        pytest.skip("liodom_replay not built (run __graft_entry__.build())")
    H, W, K = 16, 900, 5
    cfg = synth.make_cfg(H, W, 0)
    scans = [synth.scan(cfg, 0, k)[0].astype(np.float32) for k in range(K)]
    args = ["scan_lines=16", "scan_regions=6", "edges_per_region=10", "prev_frames=5", "mapping=true"]

    def replay(name, ks, *more):
        sd, od = tmp_path / (name + "_scans"), tmp_path / (name + "_out")
        sd.mkdir(); od.mkdir()
        for k in ks:
            scans[k].tofile(str(sd / ("%06d.bin" % k)))
        r = subprocess.run([exe, str(sd), str(od) + "/"] + args + list(more), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return od

    s5 = tmp_path / "five.mapstate"
    od = replay("five", range(5), "map_state_out=%s" % s5)
    st = api.parse_map_state(s5.read_bytes(), sizes=SZ)
    m = np.fromfile(str(od / "map.bin"), dtype=np.float32).reshape(-1, 4)
    assert same(st["points"], m) and m.shape[0] > 100 and st["status"] == 0
    s3 = tmp_path / "three.mapstate"
    replay("three", range(3), "map_state_out=%s" % s3)
    st3 = api.parse_map_state(s3.read_bytes(), sizes=SZ)
    od = replay("rest", (3, 4), "map_state_in=%s" % s3)
    m = np.fromfile(str(od / "map.bin"), dtype=np.float32).reshape(-1, 4)
    # the oracle's mapper from the same state (a cell's cloud holds one point per leaf in leaf order: feeding it alone rebuilds
    # the cell as it is) and fed the same poses: odom.txt has them with 17 digits (stamp, orientation xyzw, position)
    mo = orc.Map(*SZ)
    for c in st3["cells"]:
        mo.update(c)
    assert same(mo.all(), st3["points"])
    po = orc.make_params(scan_lines=H, scan_regions=6, edges_per_region=10, prev_frames=5, knn_mode=1, mapping=1)
    odom = np.loadtxt(str(od / "odom.txt")).reshape(-1, 14)
    assert odom.shape[0] == 2
    for row, k in zip(odom, (3, 4)):
        T, _ = orc.pose_ops(row[1:5], row[5:8])
        mo.update(orc.extract(po, scans[k], H, W)["edges"], T)
    assert m.shape[0] == mo.all().shape[0] and m.shape[0] > st3["points"].shape[0]
