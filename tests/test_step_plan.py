"""The plan of a scan's launches (liodom_amd/csrc/step_plan.h: which kernels a step launches, with which grids, on which queue, in
which order, and the state that runs from scan to scan) in a program of its own, built plain and under host sanitizers.  No GPU,
nothing sanitized is loaded into Python.
  1. the launches the parent of the plan issued on an MI355X for the scenarios of tests/step_scenarios.py
     (tests/step_launches_mi355x.json, tools/record_step_launches.py) are reproduced row for row, per kernel instance as the
     fixture's "compare" says, and so are the per-bucket counts of liodom_get_kernel_stats;
  2. the invariants the kernels rely on and a trace cannot show hold over tests/handle_matrix.py crossed with request kinds;
  3. no plan comes within 8 entries of the list's capacity (the driver fails otherwise)."""
import json
import os
import shutil
import subprocess

import pytest

import handle_matrix as hm
import step_scenarios as ss
from test_handle_plan import SAN, case as handle_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
with open(os.path.join(ROOT, "tests", "step_launches_mi355x.json")) as _f:
    FIXTURE = json.load(_f)
with open(os.path.join(ROOT, "tests", "handle_modes_mi355x.json")) as _f:
    HANDLES = {e["name"]: e for e in json.load(_f)}
BUCKETS = ["k_classify", "k_ring_extract", "k_compact_edges", "k_knn", "k_lm_solve", "k_hash_clear", "k_window_insert", "k_hash_alloc",
           "k_hash_scatter", "k_ring_scatter", "k_hash_build", "other"]
# liodom_sizes.h
LM_THREADS, REBUILD_AUX, REBUILD_ALLOC, HB_PERIOD, TILE_PTS = 256, 8, 32, 4, 2048
NO_ROWS = {"k_knn<256, false, true, false>", "k_knn<256, true, false, false>", "k_lm_solve<0, true, false>", "k_lm_solve<1, true, false>",
           "k_rebuild_alloc<false>", "k_pose_cov<false>", "k_chain_redo0<256>", "k_knn_redo<256>", "k_ov_gate", "k_rebuild_fin"}
FIELDS = ("q", "gx", "gy", "block", "lds", "scope", "bucket", "pass", "seq_k", "done_target", "scan_no", "nA", "with_pass", "with_fix",
          "alloc", "tiles", "lb_tag", "wait_edges", "signal_odo")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("step") / ("step_plan_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "step_plan_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def drive(exe, lines):
    """The driver's answer to one block of input: [(request line, [planned entries], state)] and the handle's modes."""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def parse(lines, out):
    """Pairs the requests that plan something (x, o, f) with what the driver printed for them."""
    modes, steps, cur = None, [], []
    it = iter(out)
    planned = [ln for ln in lines if ln.split()[0] in ("x", "o", "f")]
    for ln in it:
        if ln.startswith("H "):
            modes = hm.parse_modes(ln[2:])
        elif ln.startswith("L "):
            name, rest = ln[2:].split(" | ")
            w = rest.split()
            cur.append(dict(zip(FIELDS, [w[0]] + [int(x) for x in w[1:]]), name=name))
        elif ln.startswith("O "):
            w = ln.split()
            cur.append(dict(name=w[1], op=True, scopes=int(w[2]) if len(w) > 2 else 0))
        else:
            assert ln.startswith("S "), ln
            st = dict(kv.split("=") for kv in ln[2:].split())
            steps.append((planned[len(steps)], cur, st))
            cur = []
    assert len(steps) == len(planned), (len(steps), len(planned))
    return modes, steps


def handle_line(exe, name, extra=()):
    """The `handle` line of a matrix entry on the recorded device: its CU count and the smallest k_ring_split occupancy that
    gives the recorded budget (as tests/test_handle_plan.py finds it)."""
    e = HANDLES[name]
    want = hm.parse_modes(e["modes"])["ring_split_max_wgs"]
    for w in range(9):
        ln = "handle " + handle_case(e, e["cus"], w, extra)
        modes = hm.parse_modes(drive(exe, [ln])[0][2:])
        if modes["ring_split_max_wgs"] == want:
            return ln
    raise AssertionError((name, want))


def fold(rows):
    out = []
    for r in rows:
        if out and out[-1][:4] == r:
            out[-1][4] += 1
        else:
            out.append(list(r) + [1])
    return out


def test_scenarios_are_the_recorded_ones():
    assert FIXTURE["compare"] == "per_instance" and list(FIXTURE["scenarios"]) == ss.NAMES
    for sc in ss.SCENARIOS:
        rec = FIXTURE["scenarios"][sc[0]]
        assert rec["handle"] == sc[1] and rec["cus"] == HANDLES[sc[1]]["cus"], sc[0]


def test_recorded_launches_are_reproduced(exe):
    """Per kernel instance, the rows [grid x, grid y, block, dynamic LDS, repeats] in the order of the plan."""
    known = set(drive(exe, ["names"]))
    for sc in ss.SCENARIOS:
        rec = FIXTURE["scenarios"][sc[0]]
        lines = [handle_line(exe, sc[1])] + ss.requests(sc, confirmed=rec["confirmed"])
        _, steps = parse(lines[1:], drive(exe, lines))
        got = {}
        for _, entries, _ in steps:
            for e in entries:
                if "op" not in e:
                    got.setdefault(e["name"], []).append([e["gx"], e["gy"], e["block"], e["lds"]])
        got = {k: fold(v) for k, v in got.items()}
        want = {k: v for k, v in rec["launches"].items() if k in known}
        assert set(got) <= known, sc[0]
        assert sorted(got) == sorted(want), (sc[0], sorted(set(got) ^ set(want)))
        for k in want:
            assert got[k] == want[k], (sc[0], k, got[k], want[k])


def test_recorded_bucket_counts_are_reproduced(exe):
    """With profiling on from the start: one count per event pair the plan opens, the mapper block's included."""
    for sc in ss.SCENARIOS:
        rec = FIXTURE["scenarios"][sc[0]]
        lines = [handle_line(exe, sc[1])] + ss.requests(sc, confirmed=rec["confirmed"], profiling=True)
        _, steps = parse(lines[1:], drive(exe, lines))
        got = dict.fromkeys(BUCKETS, 0)
        for _, entries, _ in steps:
            for e in entries:
                if "op" in e:
                    got["other"] += e["scopes"]
                elif e["scope"] == 1:
                    got[BUCKETS[e["bucket"]]] += 1
        assert got == rec["counts"], (sc[0], got, rec["counts"])


# ---- invariants over the whole matrix ----
N_PTS = 3000      # two tiles


def kinds(S):
    """Request sequences: (name, lines).  Every one starts from a fresh handle."""
    scan = ["x q=o s0=0 count=1 n=%d width=0" % N_PTS, "o s0=0 count=1 pipe=0", "c lag=0 confirmed=1"]
    piped = ["x q=x s0=0 count=%d n=%d width=0" % (S, N_PTS), "o s0=0 count=%d pipe=1" % S, "c lag=0 confirmed=1"]
    unconfirmed = piped[:2] + ["c lag=0 confirmed=0"]
    out = [("scans", scan * 5), ("pipelined", piped * 6), ("pipelined, then a scan", piped * 5 + ["f"] + scan + piped * 3 + ["f"]),
           ("unconfirmed", unconfirmed * 5 + ["f"] + scan), ("profiling", ["p"] + piped * 4), ("suppressed", ["set ov_suppress=1"] + piped * 4),
           ("second handle", ["set alone=0"] + piped * 4), ("mixed", scan * 3 + piped * 2 + scan * 2 + piped * 3),
           ("lagged mapper", ["m lagged=1"] + scan * 3), ("reader", ["set reader=1"] + scan * 2)]
    if S > 2:
        sub = "1,2"
        out.append(("subset", piped * 2 + ["x q=x s0=-1 count=2 n=%d width=0" % N_PTS, "o s0=-4 count=2 pipe=1 list=" + sub] * 3 + piped * 3 +
                    ["x q=o s0=1 count=1 n=%d width=0" % N_PTS, "o s0=1 count=1 pipe=0"]))
    return out


def check_step(name, m, x, req, entries, st, track):
    i = lambda d, k: int(d[k])      # noqa: E731
    G, edge_cap, P, S = i(m, "lm_groups"), i(x, "edge_cap"), i(x, "prev_frames"), i(m, "n_streams")
    knn_grid = int(m["knn_grid"].split("/")[0])
    early = i(m, "early_rebuild")
    cdiv = lambda a, b: (a + b - 1) // b      # noqa: E731
    nC, nP = cdiv(edge_cap * max(1, P - 1), LM_THREADS), cdiv(edge_cap, LM_THREADS)
    names = [e["name"] for e in entries]
    launches = [e for e in entries if "op" not in e]
    words = dict(w.split("=") for w in req.split()[1:])
    count = int(words.get("count", 1))
    for e in launches:
        assert e["gx"] >= 1 and e["gy"] >= 1 and e["block"] >= 64 and e["block"] % 64 == 0, (name, e)
        if e["name"] not in NO_ROWS:      # the list instance exactly for a step over a stream list
            assert e["name"].endswith(("<true>", ", true>")) == (int(words.get("s0", 0)) < 0), (name, e)
    if req.startswith("x"):
        tiles = cdiv(N_PTS, TILE_PTS)
        for e in launches:
            assert e["q"] == words["q"] and e["tiles"] == tiles, (name, e)
            if e["name"].startswith("k_ring_split_lb"):
                assert e["gx"] == tiles * count and e["lb_tag"] != 0, (name, e)
            elif e["name"].startswith(("k_ring_split<", "k_classify", "k_ring_scatter")):
                assert (e["gx"], e["gy"]) == (tiles, count), (name, e)
                if e["name"].startswith("k_ring_split<"):
                    assert tiles * count <= i(m, "ring_split_max_wgs") and i(m, "ring_split"), (name, e)
            else:
                assert e["gy"] == count, (name, e)
        assert names[-1].startswith("k_compact_edges") and names[-2].startswith("k_ring_extract"), (name, names)
        assert st["lb_tag"] != "0" or not any(n.startswith("k_ring_split_lb") for n in names), name
        return
    chain = any(n.startswith("k_knn<256, false, true") for n in names)
    overlapped = chain or any(n.startswith("k_knn<256, true") for n in names)
    if req.startswith("f"):
        assert all(e["name"] == "k_chain_redo0<256>" and e["with_pass"] == 0 and e["with_fix"] == 1 and e["gx"] == e["nA"] == cdiv(edge_cap, 256) for e in entries), (name, entries)
        assert st["fix"] == "0", name
        return
    # solver blocks sit at 0, 8, ..., (G - 1) * 8, and every role a solve launch decodes is covered
    for e in launches:
        if e["name"].startswith("k_lm_solve"):
            fin = e["name"].startswith("k_lm_solve<1")
            assert e["gx"] >= (G - 1) * 8 + 1 and e["lds"] >= 4 * edge_cap, (name, e)
            if chain:
                assert e["gx"] == (G - 1) * 8 + 1 and e["q"] == "o", (name, e)
            elif early:
                assert e["gx"] >= G + (nP + REBUILD_AUX + nC if fin else nC + nP), (name, e)
        if e["name"].startswith("k_knn<") and not chain:
            second_alloc = early and e["pass"] == 1 and e["seq_k"] == 0
            assert e["gx"] == knn_grid + (REBUILD_AUX if second_alloc else 0), (name, e)
    if chain:
        # never with count != 1, under profiling, suppressed, beside a second handle, or in the first two scans after a reset
        assert count == 1 and not track["profiling"] and not track["suppressed"] and track["alone"] and track["since_reset"] >= 2, (name, track)
        assert words.get("pipe") == "1" and i(m, "chain") == 1, name
        by = {e["name"]: e for e in launches}
        first = by["k_knn<256, false, true, false>"]
        assert first["gx"] == knn_grid and first["q"] == "k" and first["wait_edges"] != 0, (name, first)
        track["done"] = (track["done"] + knn_grid) % 2 ** 32
        for k in ("k_lm_solve<0, true, false>", "k_lm_solve<1, true, false>"):
            assert by[k]["done_target"] == track["done"] == int(st["chain_count"]), (name, by[k], track["done"])
        second = by["k_knn<256, true, false, false>"]
        assert second["gx"] == knn_grid + cdiv(edge_cap * max(1, P - 1), 256) + cdiv(edge_cap, 256) and second["q"] == "k", (name, second)
        fin = by["k_rebuild_fin"]
        assert fin["gx"] == cdiv(edge_cap, LM_THREADS) + REBUILD_AUX + cdiv(edge_cap * max(1, P - 1), LM_THREADS), (name, fin)
        if i(m, "speculate"):
            redo0, redo = by["k_chain_redo0<256>"], by["k_knn_redo<256>"]
            assert redo0["gx"] == redo0["nA"] + knn_grid + 1 and redo0["nA"] == cdiv(edge_cap, 256) and redo0["with_pass"] == 1, (name, redo0)
            assert redo0["with_fix"] == track["fix"], (name, redo0, track)      # (read before this scan overwrites it)
            assert redo["gx"] == REBUILD_ALLOC + knn_grid and redo["alloc"] == REBUILD_ALLOC, (name, redo)
            assert "k_ov_gate" not in by and "k_rebuild_alloc<false>" not in by, name
        else:
            assert by["k_ov_gate"]["q"] == "k" and by["k_rebuild_alloc<false>"]["gx"] == REBUILD_ALLOC, name
        assert all(e["scope"] == 0 for e in launches), name
    if overlapped:
        seqs = {e["seq_k"] for e in launches if e["name"].startswith(("k_lm_solve", "k_knn<256, true", "k_knn<256, false, true", "k_ov_gate", "k_knn_redo"))}
        assert len(seqs) == 1 and 0 not in seqs and seqs == {int(st["ov_seq"])}, (name, seqs, st)
        assert count == 1 and not track["profiling"] and not track["suppressed"] and track["since_reset"] >= 2, (name, track)
    else:
        assert all(e.get("seq_k", 0) == 0 for e in launches), name
    # every switch plans exactly the event operation of the switch
    ops = [n for n in names if n in ("ev_ov", "ev_ch")]
    want = []
    if overlapped and not track["ov_prev"]:
        want.append("ev_ov")
    if chain and not track["chain_prev"] and track["ov_prev"]:
        want.append("ev_ov")
    if not chain and track["chain_prev"]:
        want.append("ev_ch")
    assert ops == want, (name, ops, want, track)
    if "ev_ch" in names:      # the flush's repair, if any, in front of the event
        k = names.index("ev_ch")
        assert all(e["name"] == "k_chain_redo0<256>" and e["with_pass"] == 0 for e in entries[:k] if "op" not in e and e["q"] == "k"), (name, names)
    track.update(ov_prev=overlapped, chain_prev=chain, fix=1 if (chain and i(m, "speculate")) else (0 if "ev_ch" in names else track["fix"]))
    track["since_reset"] += 1
    # a multi-stream step rebuilds all its streams if any one is due
    streams = [int(s) for s in words["list"].split(",")] if "list" in words else list(range(int(words["s0"]), int(words["s0"]) + count))
    hb = [int(v) for v in st["hb"].split(",")]
    if i(x, "lds_hash_build") and not early:
        before = [track["hb"][s] for s in streams]
        due = not i(m, "hash_incr") or any(b < 0 or b >= HB_PERIOD - 1 for b in before)
        assert any(n.startswith("k_hash_build") for n in names) == due and any(n.startswith("k_hash_append") for n in names) == (not due), (name, names, before)
        # (equal afterwards whenever the step rebuilt or they were equal before; streams that a single-stream call has put out of
        #  step advance together until the first of them is due)
        assert [hb[s] for s in streams] == ([0] * len(streams) if due else [b + 1 for b in before]), (name, hb, streams)
        assert all(hb[s] == track["hb"][s] for s in range(S) if s not in streams), name
    else:
        assert hb == track["hb"], name
    track["hb"] = hb


def run_kind(exe, hl, lines, name):
    m, steps = parse(lines, drive(exe, [hl] + lines))
    x = m      # (the handle line carries the extras behind the modes)
    S = int(m["n_streams"])
    track = dict(profiling=False, suppressed=False, alone=True, since_reset=0, ov_prev=False, chain_prev=False, fix=0, done=0, hb=[-1] * S)
    k = 0
    for ln in lines:
        if ln == "p":
            track["profiling"] = True
        elif ln.startswith("set"):
            track["suppressed"] = track["suppressed"] or "ov_suppress=1" in ln
            track["alone"] = track["alone"] and "alone=0" not in ln
            if "chain_count=" in ln:
                track["done"] = int(ln.split("chain_count=")[1].split()[0])
        elif ln == "r":
            track.update(since_reset=0, ov_prev=False, chain_prev=False, fix=0, done=0, hb=[-1] * S)
        elif ln.split()[0] in ("x", "o", "f"):
            req, entries, st = steps[k]
            k += 1
            if ln == "f":
                track["fix"] = 0
            check_step((name, ln), m, x, req, entries, st, track)
    return steps


def test_invariants_over_the_matrix(exe):
    for e in HANDLES.values():
        hl = handle_line(exe, e["name"])
        S = e["config"].get("n_streams", 1)
        for kind, lines in kinds(S):
            if kind in ("lagged mapper", "reader") and not e["params"].get("mapping"):
                continue
            run_kind(exe, hl, lines, (e["name"], kind))


def test_counters_wrap_without_becoming_zero(exe):
    """seq_k and lb_tag skip 0 (it means "not overlapped" / "no tag"); done_target follows the device counter modulo 2^32."""
    piped = ["x q=x s0=0 count=1 n=%d width=0" % N_PTS, "o s0=0 count=1 pipe=1", "c lag=0 confirmed=1"]
    for name in ("hdl64", "ouster128", "hdl64 LIODOM_CHAIN=0"):
        lines = piped * 2 + ["set ov_seq=4294967294 chain_count=4294967000"] + piped * 4
        steps = run_kind(exe, handle_line(exe, name), lines, (name, "wrap"))
        seqs = [int(st["ov_seq"]) for req, _, st in steps if req.startswith("o")]
        assert seqs[-4:] == [4294967295, 1, 2, 3], (name, seqs)
    lb = ["x q=x s0=0 count=256 n=%d width=0" % N_PTS]      # 512 tiles: over k_ring_split's budget
    _, steps = parse(["set lb_tag=4294967294"] + lb * 3, drive(exe, [handle_line(exe, "s256"), "set lb_tag=4294967294"] + lb * 3))
    tags = [e["lb_tag"] for _, entries, _ in steps for e in entries if e["name"].startswith("k_ring_split_lb")]
    assert tags == [4294967295, 1, 2], tags


def test_ring_extract_instance(exe):
    """The k_ring_extract instance by pick-list threads (64 per four regions, 256 / 1024) and by the longest region of the expected
    ring width (16 or 24 items per lane: more than 256 items take the big one).  Shapes the matrix does not have."""
    rows = [("scan_regions=8 max_width=1800", "k_ring_extract<256, 16, false>", 128),      # 1790 / 8 = 223, the last region 229
            ("scan_regions=8 max_width=2048", "k_ring_extract<256, 24, false>", 128),      # 2038 / 8 = 254, the last region 260
            ("scan_regions=16 max_width=2048", "k_ring_extract<256, 16, false>", 256),
            ("scan_regions=20 max_width=2048", "k_ring_extract<1024, 16, false>", 320),
            ("scan_regions=20 edges_per_region=4 max_width=5400", "k_ring_extract<1024, 24, false>", 320),      # 5390 / 20 = 269
            ("scan_regions=8 max_width=0 max_points=131072", "k_ring_extract<256, 24, false>", 128)]      # max_points / scan_lines = 2048
    for words, want, block in rows:
        lines = ["handle scan_lines=64 cus=256 wgs_per_cu=2 " + words, "x q=o s0=0 count=1 n=%d width=0" % N_PTS]
        _, steps = parse(lines[1:], drive(exe, lines))
        e = [e for e in steps[0][1] if e["name"].startswith("k_ring_extract")]
        assert len(e) == 1 and e[0]["name"] == want and (e[0]["gx"], e[0]["gy"], e[0]["block"]) == (64, 1, block), (words, e)


def test_reset_starts_over_except_for_the_sequence(exe):
    """reset() followed by the same requests gives the same plans, except for the continuing ov_seq (and the lb_tag, which the
    extraction side keeps)."""
    for name in ("hdl64", "ouster128", "s16", "s4", "vlp16"):
        S = HANDLES[name]["config"].get("n_streams", 1)
        piped = ["x q=x s0=0 count=%d n=%d width=0" % (S, N_PTS), "o s0=0 count=%d pipe=1" % S, "c lag=0 confirmed=1"]
        lines = piped * 6 + ["f", "r"] + piped * 6 + ["f"]
        steps = run_kind(exe, handle_line(exe, name), lines, (name, "reset"))
        half = len(steps) // 2
        strip = lambda es: [{k: v for k, v in e.items() if k not in ("seq_k", "lb_tag", "wait_edges", "signal_odo")} for e in es]      # noqa: E731
        for (_, a, sa), (_, b, sb) in zip(steps[:half], steps[half:]):
            assert strip(a) == strip(b), (name, a, b)
            for k in ("ov_warm", "ov_prev", "chain_prev", "chain_count", "fix", "hb"):
                assert sa[k] == sb[k], (name, k)
        first, second = [int(s["ov_seq"]) for _, _, s in steps[:half]], [int(s["ov_seq"]) for _, _, s in steps[half:]]
        assert second[0] == first[-1] and all(b - a == first[-1] for a, b in zip(first, second)), (name, first, second)
