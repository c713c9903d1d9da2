"""The bookkeeping of the pipeline edge buffers and the cursor of a staging ring (liodom_amd/csrc/edge_pipe.h) in a program of their
own (tests/edge_pipe_main.cc), built plain and under host sanitizers.  No GPU, nothing sanitized is loaded into Python.  The driver's
verdict and state after every operation against the restatement of tests/edge_pipe_cases.py, on the designed scripts, on every
sequence of operations up to length 5, on fixed-seed random walks and across the wrap of the sequence counters; and the properties a
caller relies on, read from the driver's output alone."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

import edge_pipe_cases as ec
from test_handle_plan import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
OPS = ["x", "s 0", "s 1", "s 2", "c", "r", "ra", "y", "z", "p"]
# Every sequence of the ten operations: 111 110 of them up to length 5, 543 210 driver lines in one process (the test takes 5 s with
# the plain driver and 7 s with the sanitized one on the machine this was written on; length 6 is ten times that).
DEPTH = 5
NEAR_WRAP = 2 ** 32 - 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("pipe") / ("edge_pipe_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "edge_pipe_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def drive(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def start(flags, ext=0, odo=0):
    """The driver's lines that begin a sequence, and what it answers to them."""
    lines = ["new flags=%d" % flags] + (["set ext=%d odo=%d" % (ext, odo)] if ext or odo else [])
    return lines, ["new | " + ec.Model(flags).state()]


def expected(flags, ops, ext=0, odo=0):
    m = ec.Model(flags, ext, odo)
    out = []
    for o in ops:
        v = m.op(o)
        out.append(v + " | " + m.state())
    return out


def fields(line):
    verdict, st = line.split(" | ")
    return verdict, dict(kv.split("=") for kv in st.split())


def check_properties(ops, lines, ext=0, odo=0):
    """From the driver's lines alone: a slot is given out only when the scan it held has been collected (or a reset has voided it),
    tk is non-zero exactly for the slots given out and not collected, and the two idle states are the documented ones."""
    held, flying, tickets = set(), [], []
    fresh = fields("new | " + ec.Model().state())[1]
    prev = dict(fresh, ext=str(ext), odo=str(odo))
    for o, ln in zip(ops, lines):
        v, st = fields(ln)
        w = v.split()
        if o == "x" and w[0] == "ok":
            slot = int(w[1])
            assert slot not in held and int(w[2]) != 0, (ops, o, ln)
            held.add(slot)
            tickets.append(slot)
        elif o[0] == "s" and w[0] == "ok":
            flying.append(tickets[int(o.split()[1])])
        elif o == "c" and w[0] == "ok":
            assert int(w[1]) == flying.pop(0) and int(w[2]) == len(flying), (ops, o, ln)
            held.discard(int(w[1]))
        elif o == "z":
            held, flying = set(), []
            assert st == fresh, (ops, ln)      # reset(): the constructor's state
        elif w[0] == "ok" and (o == "p" or (o == "y" and prev["pf"] == "-1")):
            # drained(): nothing to wait for, nothing ahead, the replay at buffer 0; tickets and counters as they were
            assert (st["ebr"], st["free"], st["parity"], st["pf"], st["active"], st["live"]) == ("0,0,0", "0,0,0", "0", "-1", "0", "0"), (ops, ln)
            assert all(st[k] == prev[k] for k in ("tk", "x_next", "fifo", "ext", "odo", "ebs")), (ops, ln, prev)
        assert {b for b, t in enumerate(st["tk"].split(",")) if t != "0"} == held, (ops, o, ln, held)
        assert (st["fifo"].split(",") if st["fifo"] != "-" else []) == [str(s) for s in flying], (ops, o, ln, flying)
        prev = st


def test_designed_scripts(exe):
    for flags in (1, 0):
        for ext in (0, NEAR_WRAP):
            for name, text, _ in ec.SCRIPTS:
                ops = [o.replace("s_", "s ") for o, _ in ec.script_ops(text)]
                begin, begun = start(flags, ext, ext)
                got = drive(exe, begin + ops)
                assert got[0] == begun[0], name
                assert [ln.split()[0] for ln in got[1:]] == [v for _, v in ec.script_ops(text)], (name, flags, ext)
                assert got[1:] == expected(flags, ops, ext, ext), (name, flags, ext)
                check_properties(ops, got[1:], ext, ext)


def test_every_sequence_up_to_depth(exe):
    """One driver process plays every sequence from a fresh EdgePipe; the restatement walks them as a tree, a node at a time."""
    lines, want = [], []
    begin, begun = start(1)

    def walk(m, ops, answers):
        for o in OPS:
            n = m.clone()
            v = n.op(o)
            here = answers + [v + " | " + n.state()]
            lines.extend(begin + ops + [o])
            want.extend(begun + here)
            if len(here) < DEPTH:
                walk(n, ops + [o], here)

    walk(ec.Model(1), [], [])
    assert len(want) == len(lines) and sum(1 for ln in lines if ln.startswith("new")) == sum(len(OPS) ** k for k in range(1, DEPTH + 1))
    got = drive(exe, lines)
    if got != want:
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        first = max(i for i in range(k + 1) if lines[i].startswith("new"))
        raise AssertionError((lines[first:k + 1], got[k], want[k]))
    # the properties, on every sequence up to length 4 (each is a prefix of the longer ones)
    seqs = [list(ops) for n in range(1, DEPTH) for ops in itertools.product(OPS, repeat=n)]
    got = drive(exe, [ln for ops in seqs for ln in begin + ops])
    at = 0
    for ops in seqs:
        check_properties(ops, got[at + 1:at + 1 + len(ops)])
        at += 1 + len(ops)
    assert at == len(got)


def random_ops(rng, n):
    m, ops = ec.Model(), []
    for _ in range(n):
        o = rng.choices(["x", "s", "c", "r", "ra", "y", "z", "p"], weights=[30, 30, 25, 3, 3, 4, 1, 4])[0]
        if o == "s":
            o = "s %d" % max(0, len(m.tickets) - 1 - rng.choice([0, 0, 0, 1, 1, 2, 3]))
        m.op(o)
        ops.append(o)
    return ops


def test_random_walks(exe):
    """Fixed seeds, 4000 operations each: the slot ring wraps several hundred times; from zero and from just below 2^32, so that the
    counters skip 0 with tickets outstanding."""
    for seed in (1, 2, 3, 4):
        ops = random_ops(random.Random(seed), 4000)
        for flags, ext, odo in ((1, 0, 0), (0, 0, 0), (1, NEAR_WRAP, NEAR_WRAP - 1)):
            begin, _ = start(flags, ext, odo)
            got = drive(exe, begin + ops)[1:]
            assert got == expected(flags, ops, ext, odo), (seed, flags, ext)
            check_properties(ops, got, ext, odo)
            wraps = sum(1 for o, ln in zip(ops, got) if o == "x" and ln.startswith("ok 0 "))
            assert wraps > 100, wraps


def test_the_counters_skip_zero_with_tickets_outstanding(exe):
    begin, _ = start(1, NEAR_WRAP, NEAR_WRAP)
    ops = ["x", "x", "x", "s 0", "s 1", "c", "c", "s 2", "c"]
    got = drive(exe, begin + ops)[1:]
    assert [ln.split(" | ")[0] for ln in got[:3]] == ["ok 0 4294967295", "ok 1 1", "ok 2 2"], got[:3]
    assert [fields(ln)[1]["odo"] for ln in got[3:5]] == ["4294967295", "1"] and fields(got[4])[1]["ebr"] == "4294967295,1,0", got[3:5]
    assert got == expected(1, ops, NEAR_WRAP, NEAR_WRAP)
    check_properties(ops, got, NEAR_WRAP, NEAR_WRAP)


def test_extraction_ahead_is_trusted_for_its_slot_and_list_only(exe):
    got = drive(exe, ["new flags=1", "ahead 2 4", "match 2 4", "match 1 4", "match 2 4 0,1", "ahead 3 4 1,3", "match 3 4 1,3", "match 3 4",
                      "match 3 4 1,2", "match 3 4 1", "match 2 4 1,3", "unahead", "match 3 4 1,3"])
    assert [ln for ln in got if len(ln) == 1] == ["1", "0", "0", "1", "0", "0", "0", "0", "0"], got
    assert fields(got[1])[1]["pf"] == "2" and fields(got[5])[1]["pf"] == "3" and fields(got[-2])[1]["pf"] == "-1"


# ---- the staging ring's cursor ----
def test_ring_owns_at_the_edges_of_every_slot(exe):
    for stride in (1, 16, 57600):
        lines, want = ["ring %d" % stride], [None]
        for k in range(ec.BUFS):
            lines += ["owns %d" % (k * stride), "owns %d" % ((k + 1) * stride - 1)]
            want += [k, k]
        lines += ["owns %d" % (ec.BUFS * stride), "owns -1", "owns -64"]
        want += [-1, -1, -1]
        got = drive(exe, lines)
        assert [int(ln.split()[0]) for ln in got[1:]] == want[1:], (stride, got)


def test_ring_rotation_after_every_order_of_sources(exe):
    """Own slot k: the upload reads it, and the next slot handed out is the one behind it; a registered buffer leaves the ring alone;
    pageable memory goes through slot `next`."""
    kinds = ["own 0", "own 1", "own 2", "reg", "page"]
    lines, want = [], []
    for order in itertools.product(kinds, repeat=4):
        nxt, valid = 0, [0, 0, 0]
        lines.append("ring 64")
        want.append("0 | next=0 valid=0,0,0")
        for k in order:
            used = int(k.split()[1]) if k.startswith("own") else (-1 if k == "reg" else nxt)
            if used >= 0:
                valid[used], nxt = 1, (used + 1) % ec.BUFS
            lines.append("src " + k)
            want.append("%d | next=%d valid=%s" % (used, nxt, ",".join(map(str, valid))))
        valid[nxt] = 0
        lines.append("hand")
        want.append("%d | next=%d valid=%s" % (nxt, nxt, ",".join(map(str, valid))))
    lines.append("left")
    want.append("0 | next=%d valid=0,0,0" % nxt)      # a reset keeps the cursor
    assert drive(exe, lines) == want
