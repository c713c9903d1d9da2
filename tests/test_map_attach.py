"""Which map is attached to which stream, as what (liodom_amd/csrc/map_attach.h), in a program of its own (tests/map_attach_main.cc),
built plain and under host sanitizers.  No GPU, nothing sanitized is loaded into Python.  The driver's verdict, effects and state
after every operation against the restatement of tests/map_attach_cases.py, on the designed scripts, on every sequence of operations
up to length 3 and on fixed-seed random walks; and the properties a caller relies on, read from the driver's output alone."""
import os
import random
import shutil
import subprocess

import pytest

import map_attach_cases as mc
from test_handle_plan import SAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}
STREAMS = [n + str(s) for n, S in mc.HANDLES for s in range(S)]
OPS = ([k + st + "." + str(m) for k in "wlr" for st in STREAMS for m in range(mc.N_MAPS)] + [k + st for k in "de" for st in STREAMS] +
       ["h" + st + sign for st in STREAMS for sign in "+-"] + ["X" + n for n, _ in mc.HANDLES])
# Every sequence of the 32 operations: 33 824 of them up to length 3, 134 208 driver lines in one process (the test takes 2 s with
# the plain driver and 3 s with the sanitized one on the machine this was written on; length 4 is thirty-two times that).
DEPTH = 3


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the driver"
    if request.param not in _EXE:
        out = str(tmp_path_factory.mktemp("attach") / ("map_attach_" + request.param))
        flags = ["-O2"] if request.param == "plain" else ["-O1", "-g"] + SAN
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                           ["-I", os.path.join(ROOT, "liodom_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "map_attach_main.cc")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _EXE[request.param] = out
    return _EXE[request.param]


def drive(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


NEW = "new - | " + mc.Model().state()


def expected(ops):
    m, out = mc.Model(), []
    for o in ops:
        v = m.op(o)
        out.append(v + " | " + m.state())
    return out


def fields(line):
    answer, st = line.split(" | ")
    w = answer.split()
    return w[0], [x for x in w[1:] if x != "-"], dict(kv.split("=") for kv in st.split())


def check_properties(ops, lines):
    """From the driver's lines alone."""
    prev, moved = fields(NEW)[2], set()
    for o, ln in zip(ops, lines):
        verdict, fx, st = fields(ln)
        ctx = (ops, o, ln)
        entries = {k: v.split(":") for k, v in st.items() if k[0] in "AB"}
        links = {int(k[1:]): v.split("/") for k, v in st.items() if k[0] == "m"}
        for m, (n_att, n_rd, holder) in links.items():
            n_att, n_rd = int(n_att), int(n_rd)
            # a map's counts are the streams of its holder that name it, per kind.  Once a map has been taken from a handle that held
            # it, that handle's stream names it still and is not counted, and if the map comes back that stream's detach takes
            # another stream's count away: from then on the counts say nothing (the defect DESIGN.md describes)
            named = [e[0] for k, e in entries.items() if k[0] == holder and e[0][1:].split("/")[0] == str(m) and e[0] != "-"]
            was = int(prev["m%d" % m].split("/")[0])
            if ("move=%d" % m) in fx and was > 0:
                moved.add(m)
            if m not in moved:
                assert n_att == len(named) and n_rd == sum(1 for a in named if a[0] == "r"), ctx
                assert n_rd in (0, n_att), ctx      # read or written, not both
            assert (holder == "-") == (n_att == 0), ctx
            # onto the handle's stream exactly when the handle attaches a map it does not hold; "a stream of its own again" exactly
            # when the count reaches 0 (within one call, where a stream that lost the map attaches it again: see above)
            mine = verdict == "ok" and o[0] in "wlr" and int(o[4]) == m
            assert (("move=%d" % m) in fx) == (mine and (was == 0 or prev["m%d" % m].split("/")[2] != o[1])), ctx
            assert (("own=%d" % m) in fx) == (n_att == 0 and (was > 0 or ("move=%d" % m) in fx)), ctx
        for hn, S in mc.HANDLES:
            mine = [entries["%s%d" % (hn, s)] for s in range(S)]
            tags = [] if st["tags" + hn] == "-" else st["tags" + hn].split(",")
            read = {e[0][1:].split("/")[0] for e in mine if e[0][0] == "r"}
            assert sorted(t for t in tags if t != ".") == sorted(read), ctx      # distinct places for distinct read maps, none for others
            for e in mine:
                tag, xy, z = (int(x) for x in e[2][1:].split(","))
                if e[0][0] == "r":
                    assert tag >= 1 and tags[tag - 1] == e[0][1:].split("/")[0] and [str(xy), str(z)] == e[0].split("/")[1:], ctx
                else:
                    assert (tag, xy, z) == (0, 0, 0), ctx
            want = (sum(1 for e in mine if e[0][0] == "w" and e[0].endswith("/1")), sum(1 for e in mine if e[0][0] == "r"),
                    sum(1 for e in mine if e[1] != "h-1"))
            assert st["cnt" + hn] == "%d,%d,%d" % want, ctx
        if verdict != "ok":
            assert st == prev and not fx, ctx      # a refusal touches nothing
        prev = st


def test_designed_scripts(exe):
    for name, text in mc.SCRIPTS:
        ops = [o for o, _ in mc.script_ops(text)]
        got = drive(exe, ["new"] + ops)
        assert got[0] == NEW, name
        assert [ln.split()[0] for ln in got[1:]] == [v for _, v in mc.script_ops(text)], name
        assert got[1:] == expected(ops), name
        check_properties(ops, got[1:])


def test_designed_scripts_reach_what_they_are_for():
    """Read from the restatement: the scripts do show the effects their names promise."""
    seen = set()
    for _, text in mc.SCRIPTS:
        m, moved_away = mc.Model(), False
        for o, _ in mc.script_ops(text):
            before = m.clone()
            answer = m.op(o).split()
            kind, hn = o[0], o[1]
            if "move=" in " ".join(answer) and any(mp.n_attached for mp in before.maps if mp.attached_to not in (None, before.handles[hn])):
                moved_away = True
            if kind in "de" and moved_away and len(answer) == 2 and before.handles[hn].mappers[int(o[2])] is not None:
                seen.add("the loser's detach is a no-op on the map")
            if kind in "wlr" and before.handles[hn].mappers[int(o[2])] == int(o[4]) and not any(a.startswith(("move", "own")) for a in answer):
                seen.add("held map re-attached as " + ("the other kind" if kind == "r" else "a writer"))
            if kind == "r" and before.handles[hn].readers and before.handles[hn].readers[int(o[2])] == int(o[4]):
                seen.add("held map re-attached as a reader")
            if kind == "X" and sum(1 for q in before.handles[hn].mappers + before.handles[hn].readers if q is not None) > len(answer) - 1:
                seen.add("destroy releases less than its streams name")
            if "clr=1" in answer and "." not in m.state().split("tags" + hn + "=")[1].split()[0] and kind in "de":
                seen.add("a reader leaves, the tag stays")
            if "." in m.state().split("tags" + hn + "=")[1].split()[0]:
                seen.add("a tag is freed")
            if kind == "r" and "." in before.state().split("tags" + hn + "=")[1].split()[0] and "sel=1," in " ".join(answer):
                seen.add("a freed tag is taken again")
            if "occ=1" in answer:
                seen.add("occupancy sized by " + ("the reader's attach" if kind == "r" else "the hits call"))
            if answer[0] != "ok":
                seen.add(answer[0])
            if kind in "de" and before.handles[hn].readers and before.handles[hn].readers[int(o[2])] is not None:
                seen.add("reader detached by " + kind)
            if kind in "de" and before.handles[hn].mappers[int(o[2])] is not None:
                seen.add("writer detached by " + kind)
    want = {"the loser's detach is a no-op on the map", "held map re-attached as a writer", "held map re-attached as the other kind",
            "held map re-attached as a reader", "destroy releases less than its streams name", "a reader leaves, the tag stays", "a tag is freed",
            "a freed tag is taken again", "occupancy sized by the reader's attach", "occupancy sized by the hits call", "is_read", "is_written",
            "other_handle", "reader detached by d", "reader detached by e", "writer detached by d", "writer detached by e"}
    assert want <= seen, want - seen


def test_every_sequence_up_to_depth(exe):
    """One driver process plays every sequence from a fresh universe; the restatement walks them as a tree, a node at a time."""
    lines, want, seqs = [], [], []

    def walk(m, ops, answers):
        for o in OPS:
            n = m.clone()
            v = n.op(o)
            here = answers + [v + " | " + n.state()]
            lines.extend(["new"] + ops + [o])
            want.extend([NEW] + here)
            seqs.append((ops + [o], here))
            if len(here) < DEPTH:
                walk(n, ops + [o], here)

    walk(mc.Model(), [], [])
    assert len(OPS) == 32 and len(seqs) == sum(len(OPS) ** k for k in range(1, DEPTH + 1)) == 33824 and len(lines) == 134208
    got = drive(exe, lines)
    if got != want:
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        first = max(i for i in range(k + 1) if lines[i] == "new")
        raise AssertionError((lines[first:k + 1], got[k], want[k]))
    for ops, here in seqs:      # (the driver's lines: got == want)
        if len(ops) == DEPTH:
            check_properties(ops, here)


def test_random_walks(exe):
    """Fixed seeds, 400 operations each; attaches are three times as likely as the rest, a destroy is rare."""
    weights = [6 if o[0] in "wlr" else 1 if o[0] == "X" else 3 for o in OPS]
    for seed in (1, 2, 3, 4, 5, 6):
        ops = random.Random(seed).choices(OPS, weights=weights, k=400)
        got = drive(exe, ["new"] + ops)[1:]
        assert got == expected(ops), seed
        check_properties(ops, got)
        assert {ln.split()[0] for ln in got} == {"ok", "is_read", "is_written", "other_handle"}, seed
