"""The plan of a handle (liodom_amd/csrc/handle_plan.h: every code path and capacity liodom_create decides) in a program of its
own, built plain and under host sanitizers.  No GPU, nothing sanitized is loaded into Python.
  1. the decisions the parent of the plan took on an MI355X (tests/handle_modes_mi355x.json, tools/record_handle_modes.py) are
     reproduced key by key;
  2. the invariants the kernels rely on hold over the matrix crossed with other devices (CU counts, k_ring_split occupancies);
  3. safe mode entered after a timeout has the paths of safe mode at creation and the capacities of the handle without it;
  4. the refusals keep their codes, messages and order, sizes beyond 32 bits are refused, serialisers switch the flags off."""
import json
import os
import shutil
import subprocess

import pytest

import handle_matrix as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_EXE = {}
HB_PERIOD, LDS_SLOTS = 4, 8192      # kHbPeriod, kLdsSlots (liodom_sizes.h)
with open(os.path.join(ROOT, "tests", "handle_modes_mi355x.json")) as _f:
    FIXTURE = json.load(_f)
INVALID_ARG, CAPACITY = -1, -3


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("plan") / ("handle_plan_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "handle_plan_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def case(entry, cus, wgs, extra=()):
    """One line of the driver's input for a fixture entry on a device of `cus` CUs holding `wgs` k_ring_split workgroups per CU."""
    p = dict(entry["params"])
    if "prev_frames" in p:
        p["local_map_size"] = p.pop("prev_frames")
    words = dict(p, **entry["config"])
    words.update(entry["switches"])
    words.update(cus=cus, wgs_per_cu=wgs)
    words.update(extra)
    return " ".join("%s=%s" % kv for kv in words.items())


def run(exe, cases):
    """The driver's answers: ("plan", modes, extras) or ("refused", code, message) per case."""
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases), (len(lines), len(cases))
    out = []
    for ln in lines:
        if ln.startswith("refused "):
            _, code, msg = ln.split(" ", 2)
            out.append(("refused", int(code), msg))
        else:
            assert ln.startswith("plan "), ln
            modes, extras = ln[5:].split(" || ")
            out.append(("plan", modes, hm.parse_modes(extras)))
    return out


def test_matrix_is_the_recorded_one():
    assert [e["name"] for e in FIXTURE] == hm.NAMES
    for e, (group, name, p, c, sw) in zip(FIXTURE, hm.MATRIX):
        assert (e["group"], e["params"], e["config"], e["switches"]) == (group, p, c, sw), name


def test_recorded_decisions_are_reproduced(exe):
    """Every creation-time key of every recorded handle.  The recording had no scan processed and the probe passing, so the
    whole text must match: the runtime counters are zero on both sides and pipe_flags stays in the comparison."""
    for e in FIXTURE:
        want = hm.parse_modes(e["modes"])
        assert want[hm.PROBE_KEY] == "1", e["name"]
        for k in hm.RUNTIME_KEYS:
            assert set(want[k]) <= set("0./"), (e["name"], k, want[k])
        # the smallest k_ring_split occupancy that gives the recorded budget
        answers = run(exe, [case(e, e["cus"], w) for w in range(9)])
        got = next((a for a in answers if a[0] == "plan" and hm.parse_modes(a[1])["ring_split_max_wgs"] == want["ring_split_max_wgs"]), None)
        assert got is not None, (e["name"], want["ring_split_max_wgs"], answers[0])
        assert got[1] == e["modes"], (e["name"], [(k, v, want.get(k)) for k, v in hm.parse_modes(got[1]).items() if want.get(k) != v])


SWEEP_CUS, SWEEP_WGS = (32, 64, 256, 304), (0, 1, 2, 3)


def check_invariants(name, m, x, entry):
    """m: the keys of liodom_get_modes, x: the driver's extras, both as integers where they are."""
    i = lambda d, k: int(d[k])      # noqa: E731
    edge_cap, map_cap, ts, sorted_cap = i(x, "edge_cap"), i(x, "map_cap"), i(m, "table_size"), i(m, "sorted_cap")
    P, S = i(x, "prev_frames"), i(m, "n_streams")
    early, lds, lockstep = i(m, "early_rebuild"), i(x, "lds_hash_build"), i(x, "lockstep")
    mapping, filt = entry["params"].get("mapping", 0), entry["params"].get("filter_local_map", 0)
    assert sorted_cap - i(m, "hb_spill_base") == (HB_PERIOD - 1) * edge_cap, name
    assert ts & (ts - 1) == 0 and ts >= 2 * map_cap, name
    if early:
        assert ts >= 2 * (map_cap + 8 * edge_cap), name
        assert S <= 4 and not mapping and not filt and not lds, name
    if lds:
        assert ts >= LDS_SLOTS, name
    if i(m, "hash_incr"):
        assert i(m, "knn8") and lds and P > HB_PERIOD and sorted_cap >= 2 * map_cap + (HB_PERIOD - 1) * edge_cap, name
    if i(x, "chain_ok") or i(x, "ov_ok"):
        assert S == 1 and early, name
    if i(m, "speculate"):
        assert i(x, "chain_ok") or i(x, "ov_ok"), name
    assert (i(m, "knn_queries") == 4) == bool(lockstep) and (i(m, "knn_partials") == 0) == bool(lockstep), name
    assert int(m["knn_grid"].split("/")[1]) % 4 == 0 and i(x, "mask_stride") % 128 == 0, name
    assert lockstep == (S >= 16), name


def test_invariants_over_devices(exe):
    cases, names = [], []
    for e in FIXTURE:
        for cus in SWEEP_CUS:
            for w in SWEEP_WGS:
                cases.append(case(e, cus, w))
                names.append((e["name"], cus, w, e))
    for (name, cus, w, e), a in zip(names, run(exe, cases)):
        assert a[0] == "plan", (name, cus, w, a)
        check_invariants((name, cus, w), hm.parse_modes(a[1]), a[2], e)


MODE_KEYS = ("early_rebuild", "hash_build", "pipe_flags", "flag_gate", "lm_groups", "knn8", "hash_incr", "knn_overlap", "safe_mode",
             "ring_split", "ring_split_max_wgs", "ring_split_lb", "chain", "speculate", "knn_instance", "knn_queries", "knn_partials")
MODE_EXTRAS = ("lockstep", "lds_hash_build", "use_flags", "flag_gate_raw", "ov_ok", "chain_ok", "map_rows")
CAPACITY_KEYS = ("table_size", "sorted_cap", "hb_spill_base", "knn_grid")
CAPACITY_EXTRAS = ("edge_cap", "map_cap", "used_cap", "ovf_base", "recv_cap", "ring_id_stride", "tile_cap", "split_pad", "lb_hpad",
                   "ring_pitch", "ring_stride", "mask_stride", "knn8_grid", "slots_per_ring", "ring_lds_bytes")


def test_safe_mode_after_a_timeout(exe):
    """plan_enter_safe_mode(plan(entry)): the paths of plan(entry + LIODOM_SAFE_MODE=1), the capacities of plan(entry)."""
    for cus, w in [(256, 2), (64, 1)]:
        for e in FIXTURE:
            base, later, created = run(exe, [case(e, cus, w), case(e, cus, w, [("then_safe", 1)]), case(e, cus, w, [("LIODOM_SAFE_MODE", 1)])])
            name = (e["name"], cus, w)
            assert base[0] == later[0] == created[0] == "plan", name
            mb, ml, mc = (hm.parse_modes(a[1]) for a in (base, later, created))
            for k in MODE_KEYS:
                assert ml[k] == mc[k], (name, k, ml[k], mc[k])
            for k in MODE_EXTRAS:
                assert later[2][k] == created[2][k], (name, k)
            for k in CAPACITY_KEYS:
                assert ml[k] == mb[k], (name, k)
            for k in CAPACITY_EXTRAS:
                assert later[2][k] == base[2][k], (name, k)
            for m, x in ((ml, later[2]), (mc, created[2])):
                assert (x["use_flags"], x["chain_ok"], m["early_rebuild"], m["ring_split"], m["ring_split_lb"], m["lm_groups"]) == \
                    ("0", "0", "0", "0", "0", "1"), name
                assert m["safe_mode"] == "1" and m["pipe_flags"] == "0" and m["chain"] == "0" and m["knn_overlap"] == "0", name


RANGE = "liodom_create: parameter out of range"
PICKS = "pick lists (scan_regions * (edges_per_region + 1)) exceed 160 KiB of LDS"
SOLVE = "liodom_create: edge capacity too large for the solve's LDS tile"
REFUSED = {
    "scan_lines 0": ("scan_lines=0", INVALID_ARG, RANGE),
    "scan_lines 255": ("scan_lines=255", INVALID_ARG, RANGE),
    "no regions": ("scan_regions=0", INVALID_ARG, RANGE),
    "negative edges": ("edges_per_region=-1", INVALID_ARG, RANGE),
    "empty window": ("local_map_size=0", INVALID_ARG, RANGE),
    "window of 257": ("local_map_size=257", INVALID_ARG, RANGE),
    "no stream": ("n_streams=0", INVALID_ARG, RANGE),
    "no points": ("max_points=0", INVALID_ARG, RANGE),
    "empty range": ("min_range=5 max_range=5", INVALID_ARG, RANGE),
    # 8 x 4100 slots: 4 + 1 bytes each on top of the 2 KiB of continuity bits
    "pick lists": ("scan_lines=1 scan_regions=8 edges_per_region=4099", CAPACITY, PICKS),
    "range before pick lists": ("scan_lines=0 scan_regions=8 edges_per_region=4099", INVALID_ARG, RANGE),
    # 65 x 8 x 71 = 36 920 edges, 36 928 rounded up: 4 bytes each + 16 KiB are over 160 KiB; the pick lists (568 slots) fit
    "solve": ("scan_lines=65 scan_regions=8 edges_per_region=70", INVALID_ARG, SOLVE),
    "pick lists before solve": ("scan_lines=254 scan_regions=8 edges_per_region=4099", CAPACITY, PICKS),
    # products the 32-bit arithmetic of earlier versions overflowed in: all over 160 KiB of pick lists
    "slots beyond 32 bits": ("scan_regions=2147483647 edges_per_region=2147483647", CAPACITY, PICKS),
    "edges beyond 32 bits": ("scan_lines=254 scan_regions=65536 edges_per_region=1023", CAPACITY, PICKS),
}
OVERFLOW = "liodom_create: capacities (window, received map, points per scan) exceed 32-bit sizes"
TOO_LARGE = {
    "received map fills 32 bits": "mapping=1 recv_capacity=2147483647",
    "table beyond 2^30 slots": "mapping=1 recv_capacity=600000000",
    "ring ids past 32 bits": "max_points=2147483647",
    "incremental hash array beyond 32 bits": "scan_lines=16 n_streams=16 local_map_size=256 edges_per_region=200 scan_regions=11 mapping=0",
}


def test_refusals_keep_code_message_and_order(exe):
    names = list(REFUSED)
    for name, a in zip(names, run(exe, [REFUSED[n][0] + " cus=256 wgs_per_cu=2" for n in names])):
        assert a == ("refused",) + REFUSED[name][1:], (name, a)
    # the largest shapes that pass
    ok = run(exe, ["scan_lines=1 scan_regions=8 edges_per_region=4000 cus=256 wgs_per_cu=2", "scan_lines=64 scan_regions=8 edges_per_region=71 cus=256 wgs_per_cu=2"])      # 36 864 edges: 160 KiB exactly
    assert [a[0] for a in ok] == ["plan", "plan"], ok


def test_sizes_beyond_32_bits_are_refused(exe):
    """Parameters the range check accepts whose capacities do not fit DevView's ints: refused with LIODOM_ERR_CAPACITY (the
    sanitized build would report the overflow otherwise)."""
    names = list(TOO_LARGE)
    answers = run(exe, [TOO_LARGE[n] + " cus=256 wgs_per_cu=2" for n in names])
    for name, a in zip(names[:3], answers[:3]):
        assert a == ("refused", CAPACITY, OVERFLOW), (name, a)
    # (16 streams x 256 frames x 35 392 edges: twice the window + the spill list still fits — the largest lock-step window)
    assert answers[3][0] == "plan" and int(hm.parse_modes(answers[3][1])["sorted_cap"]) < 2 ** 31, answers[3]
    ok = run(exe, ["mapping=1 recv_capacity=500000000 cus=256 wgs_per_cu=2"])      # 2 x (0.5e9 + window) < 2^30
    assert ok[0][0] == "plan" and hm.parse_modes(ok[0][1])["table_size"] == str(2 ** 30), ok


def test_a_serialiser_switches_the_flags_off(exe):
    hdl64 = FIXTURE[0]
    for name in ("AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "ROCPROFILER_PMC", "ROCPROF_COUNTERS"):
        on, zero, empty = run(exe, [case(hdl64, 256, 2, [(name, v)]) for v in ("3", "0", "")])
        assert on[2]["use_flags"] == "0" and hm.parse_modes(on[1])["pipe_flags"] == "0", name
        assert zero[2]["use_flags"] == "1" and empty[2]["use_flags"] == "1", name


def test_switch_clamps(exe):
    """The validity rules of read_handle_env."""
    s16 = next(e for e in FIXTURE if e["name"] == "s16")
    rows = [([("LIODOM_REBUILD_DELTA", "0.45")], "rebuild_delta", "0.450"), ([("LIODOM_REBUILD_DELTA", "0.46")], "rebuild_delta", "0.250"),
            ([("LIODOM_REBUILD_DELTA", "0")], "rebuild_delta", "0.250"), ([("LIODOM_REBUILD_DELTA", "-1")], "rebuild_delta", "0.250"),
            ([("LIODOM_SPECULATE", "9")], "speculate", "7"), ([("LIODOM_SPECULATE", "-2")], "speculate", "0")]
    for sw, key, want in rows:
        a, = run(exe, [case(FIXTURE[0], 256, 2, sw)])
        assert hm.parse_modes(a[1])[key] == want, (sw, a[1])
    rows = [([("LIODOM_WAIT_MS", "1")], "wait_ticks", "100000"), ([("LIODOM_WAIT_MS", "0.5")], "wait_ticks", "5000000"),
            ([("LIODOM_WAIT_MS", "10000")], "wait_ticks", "1000000000"), ([("LIODOM_WAIT_MS", "10001")], "wait_ticks", "5000000"),
            ([("LIODOM_HB_NEW_ROOM", "0")], "hb_new_room", "1"), ([("LIODOM_HB_SLACK", "-5")], "hb_slack_min", "0"),
            ([("LIODOM_LDS_CELLS_MAX", "0")], "lds_cells_max", "1"), ([("LIODOM_LDS_CELLS_MAX", "99999")], "lds_cells_max", "6144"),
            ([("LIODOM_RING_PITCH", "3")], "ring_pitch", "8"), ([], "wait_ticks", "5000000")]
    for sw, key, want in rows:
        a, = run(exe, [case(s16, 256, 2, sw)])
        assert a[2][key] == want, (sw, key, a[2][key])
