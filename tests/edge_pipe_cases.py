"""The bookkeeping of the three pipeline edge buffers (liodom_amd/csrc/edge_pipe.h), named once: the operations, designed scripts of
them, and an independent restatement of the rules written from the entry points of liodom_hip.hip as they stood before the header
existed.  tests/test_edge_pipe.py plays the scripts (and every short sequence, and random walks) through tests/edge_pipe_main.cc
without a device; tests/test_gpu_edge_pipe.py plays the scripts through the public API.

Operations (one per line for the driver):
  x     liodom_extract_edges_device: the next scan's extraction into the next hand-off slot, by ticket
  s k   liodom_odometry_submit_device of the k-th ticket this script was given (0-based; a ticket never given is {seq 0, slot 0})
  c     liodom_odometry_collect
  r     one step of the pipelined replay with readback, nothing issued ahead (liodom_process_resident_pipelined, next_slot -1)
  ra    ... with the next slot's extraction issued ahead
  y     liodom_sync
  z     liodom_reset
  p     liodom_process_scan (a plain entry point)
Verdicts: "ok" (x: "ok <slot> <seq>", c: "ok <slot> <lag>"), x: "ahead" / "replay_live" / "full", s: "stale" / "submitted" /
"two_in_flight", c: "none", r / ra / p: "tickets_out"."""

import copy

M32 = 0xFFFFFFFF
BUFS = 3

# name, operations with the verdict (first word) each must get, plays on a handle without resident scans (the polar handle)
SCRIPTS = [
    ("three slots, the fourth refused", "x:ok x:ok x:ok x:full s 0:ok x:full c:ok x:ok s 1:ok c:ok s 2:ok s 3:ok c:ok c:ok", True),
    ("submit twice", "x:ok s 0:ok s 0:submitted c:ok s 0:stale", True),
    ("three submits", "x:ok x:ok x:ok s 0:ok s 1:ok s 2:two_in_flight c:ok s 2:ok c:ok c:ok", True),
    ("collect with nothing submitted", "c:none x:ok c:none s 0:ok c:ok c:none", True),
    ("stale ticket after reset", "x:ok x:ok s 0:ok z:ok s 0:stale s 1:stale c:none x:ok s 1:stale s 2:ok c:ok", True),
    ("ticket after a replay: sync, not retry", "r:ok x:replay_live x:replay_live y:ok x:ok s 0:ok c:ok", False),
    ("ticket while an extraction is ahead", "ra:ok x:ahead y:ok x:ahead r:ok y:ok x:ok r:tickets_out ra:tickets_out s 0:ok c:ok y:ok r:ok", False),
    ("plain entry point while tickets are out", "p:ok x:ok p:tickets_out s 0:ok p:tickets_out c:ok p:ok x:ok s 1:ok c:ok", True),
    ("slot ring wrapped twice", "x:ok x:ok s 0:ok c:ok x:ok s 1:ok x:ok s 2:ok c:ok c:ok x:ok x:ok s 3:ok s 4:ok c:ok x:ok c:ok s 5:ok s 6:ok c:ok c:ok", True),
]


def script_ops(text):
    """[(operation, expected verdict)] of a SCRIPTS row."""
    return [tuple(w.rsplit(":", 1)) for w in text.replace("s ", "s_").split()]


def next_seq(v):
    v = (v + 1) & M32
    return v or 1      # 0 means "nothing to wait for"


class Model:
    """A three-slot ring, a FIFO of at most two, the two flags; flags: the handle orders its HIP streams by flags in device memory
    (sequence numbers), else by events."""

    def __init__(self, flags=True, ext_seq=0, odo_seq=0):
        self.flags, self.tickets, self.cur = flags, [], 0      # (tickets given and the replay's next slot: the script's, not the handle's)
        self.reset()
        self.ext, self.odo = ext_seq, odo_seq

    def clone(self):
        m = copy.copy(self)
        for k in ("tk", "fifo", "ebs", "ebr", "free", "tickets"):
            setattr(m, k, list(getattr(self, k)))
        return m

    def reset(self):
        self.tk, self.x_next, self.fifo, self.ext, self.odo = [0] * BUFS, 0, [], 0, 0
        self.ebs, self.ebr, self.free = [0] * BUFS, [0] * BUFS, [0] * BUFS
        self.parity, self.pf, self.active, self.live = 0, -1, False, False

    def drained(self):
        self.ebr, self.free, self.parity, self.pf, self.active, self.live = [0] * BUFS, [0] * BUFS, 0, -1, False, False

    def _extract(self, eb):
        if self.flags:
            self.ext = next_seq(self.ext)
            self.ebs[eb] = self.ext

    def _odometry(self, eb):
        if self.flags:
            self.odo = next_seq(self.odo)
            self.ebr[eb] = self.odo
        else:
            self.free[eb] = 1

    def op(self, o):
        o = o.replace("s_", "s ")
        if o == "x":
            if self.pf >= 0:
                return "ahead"
            if self.live:
                return "replay_live"
            eb = self.x_next
            if self.tk[eb]:
                return "full"
            self.ext = next_seq(self.ext)
            self.ebs[eb] = self.tk[eb] = self.ext
            self.active, self.x_next = True, (eb + 1) % BUFS
            self.tickets.append((self.ext, eb))
            return "ok %d %d" % (eb, self.ext)
        if o[0] == "s":
            k = int(o.split()[1])
            seq, eb = self.tickets[k] if k < len(self.tickets) else (0, 0)
            if seq == 0 or self.tk[eb] != seq:
                return "stale"
            if eb in self.fifo:
                return "submitted"
            if len(self.fifo) >= 2:
                return "two_in_flight"
            self._odometry(eb)
            self.active = True
            self.fifo.append(eb)
            return "ok"
        if o == "c":
            if not self.fifo:
                return "none"
            lag, eb = len(self.fifo) - 1, self.fifo.pop(0)
            self.tk[eb] = 0
            return "ok %d %d" % (eb, lag)
        if o in ("r", "ra", "p") and any(self.tk):
            return "tickets_out"
        if o in ("r", "ra"):
            self.live, eb = True, self.parity
            if self.pf != self.cur:
                self._extract(eb)
            self.pf = -1
            self._odometry(eb)
            self.parity, self.cur = (eb + 1) % BUFS, self.cur + 1
            if o == "ra":
                self._extract(self.parity)
                self.pf = self.cur
        elif o == "p" or (o == "y" and self.pf < 0):
            self.drained()
        elif o == "z":
            self.reset()
        else:
            assert o == "y", o
        return "ok"

    def state(self):
        j = lambda a: ",".join(str(int(v)) for v in a)      # noqa: E731
        return "tk=%s x_next=%d fifo=%s ext=%d odo=%d ebs=%s ebr=%s free=%s parity=%d pf=%d active=%d live=%d" % (
            j(self.tk), self.x_next, j(self.fifo) or "-", self.ext, self.odo, j(self.ebs), j(self.ebr), j(self.free), self.parity,
            self.pf, self.active, self.live)
