"""Edge extraction on designed rings (tests/designed_rings.py): k_ring_extract and k_compact_edges, fed by every ring split, on
inputs that reach the tie branch, the cut-off in double, the 64-bit window over the continuity bits, deep carry cascades, the
boundaries of the register path and designed per-ring counts — instead of scenes and jagged rings.

Bar (the project's): the edges of liodom_extract_edges / liodom_get_edges / liodom_wait_edges EXACTLY equal to the oracle's —
ring, index in ring, source index, XYZI bits —, the per-ring counts, and the FP64 smoothness of liodom_get_curvature bit for bit.
The oracle is the single reference; the GPU legs are not compared with each other.  That every family shows what it is designed
to show is asserted on the oracle in tests/test_designed_rings.py; which rings stay on the register path is asserted here from
the shape (designed_rings.register_path / instance_for), not read from the kernel.

Paths: one-stream handles with lidar_type 1 (k_row_compact, a family per launch) and lidar_type 0 (one ring 8 per call; k_ring_split
and, with LIODOM_RING_SPLIT=0, k_classify + k_ring_scatter), each with a max_width that selects the 16- and the 24-item instance;
handles sized exactly to a boundary shape; 3-stream handles and 16-stream lock-step batches (liodom_process_resident) whose
streams carry different families, two launches with different assignments; whole clouds with designed per-ring counts through
liodom_process_scan and the host-mapped mirror.  Run with -m gpu on an MI355X."""
import os

import numpy as np
import pytest

import liodom_amd as la
import designed_rings as dr

pytestmark = pytest.mark.gpu

CASCADES = [(8, "base"), (16, "base"), (64, "base"), (8, "twice"), (16, "twice"), (8, "sector5")]
FAMILIES = {c.name: c for c in [dr.ties(), dr.cutoff(), dr.gaps()] + [dr.cascade(R, v) for R, v in CASCADES]}
BOUNDARIES = {c.name: c for c in dr.boundaries()}
CASES = dict(FAMILIES, **BOUNDARIES)
# the boundary rings that stay on the register path of the instance with 16 / 24 items per lane
FAST16 = {"len256", "sector5", "r64", "r6_min", "r6_long_last", "r7"}
FAST24 = FAST16 | {"len257", "len384", "nr16384"}


class _Env:
    """The LIODOM_* environment of one liodom_create: everything cleared, then `env`; restored afterwards."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: v for k, v in os.environ.items() if k.startswith("LIODOM_")}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)
        os.environ.update(self.saved)


def open_handle(orc, lidar_type, H, R, epr, max_points, max_width, S=1, env=None):
    with _Env(env or {}):
        g = la.Liodom(la.make_params(lidar_type=lidar_type, scan_lines=H, scan_regions=R, edges_per_region=epr),
                      la.make_config(n_streams=S, max_points=max(int(max_points), 16), max_width=int(max_width), debug_buffers=1))
    return g, orc.make_params(lidar_type=lidar_type, scan_lines=H, scan_regions=R, edges_per_region=epr)


_want = {}


def want(orc, po, key, x, H, W):
    """The oracle's answer for one cloud, computed once per (parameters, cloud) and never changed."""
    key = (po.lidar_type, H, po.scan_regions, po.edges_per_region) + tuple(key)
    if key not in _want:
        o = orc.extract(po, x, H, W, want_curv=True)
        o["offs"] = orc.split(po, x, H, W)[0]
        for v in o.values():
            v.setflags(write=False)
        _want[key] = o
    return _want[key]


def assert_edges_equal(g, o, what):
    assert len(g["ring"]) == len(o["ring"]), (what, len(g["ring"]), len(o["ring"]))
    assert np.array_equal(g["ring"], o["ring"]), what
    assert np.array_equal(g["idx_in_ring"], o["idx_in_ring"]), (what, np.nonzero(g["idx_in_ring"] != o["idx_in_ring"])[0][:8])
    assert np.array_equal(g["src"], o["src"]), what
    assert np.array_equal(g["edges"].view(np.uint32), o["edges"].view(np.uint32)), what


def check(g, o, e, H, what, stream=0):
    """Edges, per-ring counts, ring sizes and smoothness bits of the last extraction of `stream` against the oracle's `o`."""
    assert_edges_equal(e, o, what)
    assert np.array_equal(np.bincount(e["ring"], minlength=H), np.bincount(o["ring"], minlength=H)), what
    cg, offs = g.curvature(stream)
    assert np.array_equal(offs, o["offs"]), (what, offs, o["offs"])
    co = o["curv"][:len(cg)]
    m = ~np.isnan(cg)
    assert np.array_equal(np.isnan(cg), np.isnan(co)), what
    assert np.array_equal(cg[m].view(np.uint64), co[m].view(np.uint64)), what


def framed(rows):
    """The rows between two empty ones: the first and the last ring of the cloud are empty."""
    return [None] + list(rows) + [None]


def expected_paths(name, case, ipl):
    """Which of the case's rings stay on the register path of the instance, from the shape alone."""
    fast = [dr.register_path(len(r), case.R, ipl) for r in case.rows]
    if name in BOUNDARIES:
        assert fast == [name in (FAST16 if ipl == 16 else FAST24)], (name, ipl)
    else:
        assert all(fast), (name, ipl)              # every designed family is aimed at the register path
    return fast


@pytest.mark.parametrize("ipl", [16, 24])
@pytest.mark.parametrize("name", list(CASES))
def test_rows_of_one_cloud(orc, name, ipl):
    """lidar_type 1: the family's rings as rows of one cloud, one launch (k_row_compact, k_ring_extract, k_compact_edges)."""
    case = CASES[name]
    x, H, W = dr.pack(framed(case.rows))
    mw = dr.width_for(case.R, ipl)
    assert dr.instance_for(mw, case.R) == ipl
    expected_paths(name, case, ipl)
    g, po = open_handle(orc, 1, H, case.R, case.epr, H * W, mw)
    o = want(orc, po, (name,), x, H, W)
    assert name in ("r6_below_min", "cutoff") or len(o["ring"]) > 0
    check(g, o, g.extract_edges(x, H, W), H, (name, ipl))
    g.close()


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("ipl", [16, 24])
@pytest.mark.parametrize("name", list(CASES))
def test_one_ring_per_call(orc, name, ipl, split):
    """lidar_type 0: every ring of the family alone, as ring 8 of a 16-line cloud; k_ring_split (default) and k_classify +
    k_ring_scatter (LIODOM_RING_SPLIT=0)."""
    case = CASES[name]
    mw = dr.width_for(case.R, ipl)
    expected_paths(name, case, ipl)
    g, po = open_handle(orc, 0, 16, case.R, case.epr, max(len(r) for r in case.rows), mw, env={"LIODOM_RING_SPLIT": split})
    assert g.modes()["ring_split"] == split
    for i, row in enumerate(case.rows):
        o = want(orc, po, (name, i), row, 16, 0)
        assert (o["ring"] == 8).all() and o["offs"][9] - o["offs"][8] == len(row)
        check(g, o, g.extract_edges(row, 16, 0), 16, (name, i, ipl, split))
    g.close()


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_boundary_on_a_handle_of_its_own_size(orc, name):
    """max_points and max_width exactly the ring's: the instance follows from the ring itself.  R = 64: the 1024-thread instance on
    its register path; R = 65 and 16385 points: the generic path, with suppression active (continuous gaps)."""
    case = BOUNDARIES[name]
    row = case.rows[0]
    n = len(row)
    fast = dr.register_path(n, case.R, dr.instance_for(n, case.R))
    assert fast == (name in FAST24), name
    if name in ("r64", "nr16384"):
        assert fast and case.R == 64
    if name in ("r65", "nr16385", "sector4", "len385"):
        assert not fast and dr.continuity(row)[1:].all()
    g, po = open_handle(orc, 0, 16, case.R, case.epr, n, n)
    check(g, want(orc, po, (name, 0), row, 16, 0), g.extract_edges(row, 16, 0), 16, (name, "ring"))
    g.close()
    x, H, W = dr.pack(framed(case.rows))
    g, po = open_handle(orc, 1, H, case.R, case.epr, H * W, n)
    check(g, want(orc, po, (name,), x, H, W), g.extract_edges(x, H, W), H, (name, "rows"))
    g.close()


# ---------------------------------------------------------------------------------------------
# several streams in one launch
# ---------------------------------------------------------------------------------------------
def _stream_inputs(lidar_type):
    """[(name, cloud)], (H, W, points per scan) for the streams of one launch."""
    if lidar_type == 1:
        H, W = dr.STREAM_H, dr.STREAM_W
        return [(name, dr.pack(rows, H=H, W=W)[0]) for name, rows in dr.stream_families()], (H, W, H * W)
    n = dr.STREAM_W
    out = []
    for name, ring in dr.stream_rings():
        x = np.full((n, 4), np.nan, np.float32)
        x[:len(ring)] = ring
        out.append((name, x))
    return out, (16, 0, n)


@pytest.mark.parametrize("lidar_type", [1, 0])
@pytest.mark.parametrize("S", [3, 16])
def test_streams_of_one_launch_carry_different_families(orc, S, lidar_type):
    """liodom_process_resident + liodom_get_edges(s): every stream of the launch has another family, so the streams disagree
    about picks, carry rounds and counts; the second launch on the same handle deals the families out differently.  16 streams,
    lidar_type 0: k_ring_split_lb (LIODOM_RING_SPLIT=0: sixteen one-tile scans would otherwise fit k_ring_split's launch)."""
    inputs, (H, W, n) = _stream_inputs(lidar_type)
    lockstep_lb = S >= 16 and lidar_type == 0
    g, po = open_handle(orc, lidar_type, H, dr.STREAM_R, dr.STREAM_EPR, 16 * 1024 if lidar_type == 0 else n, dr.STREAM_W, S=S,
                        env={"LIODOM_RING_SPLIT": "0"} if lockstep_lb else None)
    assert dr.instance_for(dr.STREAM_W, dr.STREAM_R) == 16
    modes = g.modes()
    assert modes["n_streams"] == str(S)
    if S >= 16:
        # (k_hash_build publishes 8192 slots per stream: this handle's window is small enough for a table of 4096 by its size alone —
        #  the first run of this test ended in an illegal memory access behind the last stream's table)
        assert int(modes["table_size"]) >= 8192, modes
    if lidar_type == 0:
        assert modes["ring_split_lb"] == ("1" if lockstep_lb else "0") and modes["ring_split"] == ("0" if lockstep_lb else "1"), modes
    step = 3 if lidar_type == 1 else 5
    deal = [[(s + (S if S < len(inputs) else step) * k) % len(inputs) for s in range(S)] for k in range(2)]
    assert deal[0] != deal[1] and all(deal[0][s] != deal[1][s] for s in range(S))
    g.alloc_resident(2)
    for k in range(2):
        for s in range(S):
            g.upload_scan(s, k, inputs[deal[k][s]][1])
    for k in range(2):
        g.process_resident(k, n, H, W, readback=True)
        answers = set()
        for s in range(S):
            name, x = inputs[deal[k][s]]
            o = want(orc, po, ("stream", name), x, H, W)
            check(g, o, g.get_edges(s), H, (S, lidar_type, k, s, name), stream=s)
            answers.add((o["ring"].tobytes(), o["idx_in_ring"].tobytes()))
        assert len(answers) == len(set(deal[k])) >= 3          # the streams of the launch disagree about their picks
    # one stream on its own through the same handle
    name, x = inputs[2]
    check(g, want(orc, po, ("stream", name), x, H, W), g.extract_edges(x, H, W, stream=S - 1), H, (S, lidar_type, "alone"), stream=S - 1)
    g.close()


# ---------------------------------------------------------------------------------------------
# k_compact_edges on designed per-ring counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epr", [2, 0])
@pytest.mark.parametrize("H", [16, 129, 254])
def test_designed_counts_per_ring(orc, H, epr):
    """Every ring full (n_edges == H * R * (epr + 1)); rings 0 and H - 1 empty; a run of empty rings in the middle; only the last
    ring non-empty.  liodom_process_scan on the full cloud; liodom_extract_edges on every pattern; the host-mapped mirror
    (liodom_extract_edges_device + liodom_wait_edges) on the full and the mostly empty one."""
    W, R = dr.COUNT_W, dr.COUNT_R
    clouds = {}
    for pattern in dr.COUNT_PATTERNS:
        case = dr.counts(H, pattern, epr)
        clouds[pattern] = (dr.pack(case.rows, W=W)[0], case.info[0]["want"])
    g, po = open_handle(orc, 1, H, R, epr, H * W, W)
    full = H * R * (epr + 1)
    _, info = g.process_scan(clouds["full"][0], H, W)
    assert info.status == 0 and info.n_edges == full, (info.status, info.n_edges, full)
    assert_edges_equal(g.get_edges(), want(orc, po, ("counts", H, "full", epr), clouds["full"][0], H, W), (H, epr, "process_scan"))
    for pattern, (x, cnt) in clouds.items():
        o = want(orc, po, ("counts", H, pattern, epr), x, H, W)
        assert np.array_equal(np.bincount(o["ring"], minlength=H), cnt), pattern
        e = g.extract_edges(x, H, W)
        check(g, o, e, H, (H, epr, pattern))
        assert np.array_equal(np.bincount(e["ring"], minlength=H), cnt) and (pattern != "full" or len(e["ring"]) == full)
    for pattern in ("full", "last_only", "ends_empty"):
        x = clouds[pattern][0]
        t = g.extract_edges_device(x, H, W)
        assert t is not None
        assert_edges_equal(g.wait_edges(t), want(orc, po, ("counts", H, pattern, epr), x, H, W), (H, epr, pattern, "mirror"))
        g.odometry_step_device(t)                      # (hands the slot back)
    g.close()
