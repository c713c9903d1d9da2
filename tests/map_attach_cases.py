"""Which map is attached to which stream, as what (liodom_amd/csrc/map_attach.h), named once: the operations, designed scripts of
them, and an independent restatement of the rules written from liodom_hip.hip as it stood before the header existed (map_attachment,
other_attachments, detach_stream_map, the two attach entry points, liodom_set_map_hits, liodom_destroy).  tests/test_map_attach.py
plays the scripts (and every short sequence, and random walks) through tests/map_attach_main.cc without a device;
tests/test_gpu_map_attach.py plays the scripts through the public API.

The universe: handle A with two streams, handle B with one, maps 0 and 1.  Operations (one per line for the driver), H a handle,
s a stream, m a map:
  wHs.m         liodom_attach_mapper(H, s, m, 2, 1)                     (lag 0)
  lHs.m         liodom_attach_mapper_ex(H, s, m, {2, 1, lag = 1})
  rHs.m[/xy/z]  liodom_attach_map_reader(H, s, m, xy, z)                 (2, 1 unless given)
  dHs           liodom_attach_mapper(H, s, NULL, ...)                    detach, by the writers' entry point
  eHs           liodom_attach_map_reader(H, s, NULL, ...)                detach, by the readers' entry point
  hHs+ / hHs-   liodom_set_map_hits(H, s, 0 / -1)
  XH            liodom_destroy(H), and a fresh handle takes its name
Verdicts: "ok", w / l: "is_read", r: "is_written" / "other_handle".

After the verdict comes what the HIP half was told, in the order liodom_hip.hip did it: move=m (the map moves onto the handle's
stream), clr=1 (reader_sel[s] zeroed), own=m (the map gets a stream of its own again; X: every such map, in order), sel=tag,xy,z
(reader_sel[s] written), lag=v (lag_on[s] written where the handle has the word; -1: not touched), occ=1 (the map's kept occupancy
is sized: hits are on for the stream)."""

import copy

HANDLES = (("A", 2), ("B", 1))
N_MAPS = 2

# name, operations with the verdict each must get
SCRIPTS = [
    # 1: a reader refuses a map another handle holds, a writer takes it; the loser's detach is a no-op on the map
    ("a writer moves between handles, a reader does not",
     "wA0.0:ok rB0.0:is_written dA0:ok rA0.0:ok rB0.0:other_handle wB0.0:is_read lB0.0:is_read eA0:ok wA0.0:ok wB0.0:ok dA0:ok dB0:ok"),
    # ... and when the map comes back, the detach of the stream that lost it takes the count of the stream that holds it
    ("a moved map comes back", "lA1.1:ok wB0.1:ok wA0.1:ok dB0:ok dA1:ok rB0.1:ok dA0:ok eB0:ok"),
    # 2: attach first, detach second
    ("the held map again, as the same kind and as the other",
     "wA0.0:ok wA0.0:ok lA0.0:ok lA0.0:ok rA0.0:ok rA0.0:ok rA0.0/1/0:ok wA0.0:ok rA0.0/3/2:ok lA0.0:ok wA0.0:ok"),
    ("the held map again while another stream holds it too", "wA0.0:ok wA1.0:ok rA0.0:is_written wA0.0:ok dA1:ok rA0.0:ok rA1.0:ok wA1.0:is_read rA1.0/1/1:ok eA0:ok wA1.0:ok"),
    # read or written, not both: either order, across the streams of one handle
    ("read or written, not both", "wA0.0:ok rA1.0:is_written rA1.1:ok wA0.1:is_read lA0.1:is_read dA0:ok wA0.1:is_read rA0.1:ok wA1.0:ok rA0.0:is_written eA1:ok rA1.0:ok"),
    # 4: either entry point with NULL detaches either kind; a detach of nothing
    ("NULL detaches either kind", "dA0:ok eA0:ok wA0.0:ok eA0:ok rA0.0:ok dA0:ok lA1.1:ok eA1:ok rA1.1:ok eA1:ok rA1.1/1/0:ok"),
    # 5: the lagged count follows the options each writer was attached with
    ("lagged writers come and go", "lA0.0:ok lA1.0:ok wA0.0:ok rA1.1:ok lA1.1:ok lA0.1:ok dA1:ok wA0.0:ok dA0:ok wA0.0:ok lA1.0:ok"),
    # 6: the tag table
    ("two streams read one map, tags kept, freed and taken again", "rA0.0:ok rA1.0/1/0:ok eA0:ok rA0.1:ok dA1:ok rA1.1:ok eA0:ok eA1:ok rA0.1:ok rA1.0:ok rA0.0:ok"),
    ("the map read again gets the lowest free place", "rA0.0:ok rA1.1:ok rA1.1:ok eA0:ok rA1.1:ok rA0.0:ok"),
    # 7: hits on a stream size the map's kept occupancy before its reader is attached, and when switched on under a reader
    ("hits before and after the reader", "hA0+:ok rA0.0:ok hA1+:ok hA0-:ok rA1.1:ok hA1-:ok hA1-:ok rA0.0:ok hA0+:ok wA0.1:is_read eA0:ok lA0.1:is_read hA0-:ok hA1+:ok"),
    # 3: a destroyed handle lets go of what it still holds, each map once
    ("destroyed while two streams hold one map", "wA0.0:ok lA1.0:ok XA:ok rA0.0:ok rA1.0:ok hA1+:ok XA:ok wA0.0:ok rA1.1:ok XA:ok wA1.0:ok dA1:ok wA1.1:ok wA0.1:ok"),
    ("destroyed after its map has moved away", "wA0.0:ok rA1.1:ok wB0.0:ok XA:ok rA0.0:is_written dB0:ok wA0.0:ok wB0.0:ok XB:ok rB0.0:ok dA0:ok XB:ok"),
]


def script_ops(text):
    """[(operation, expected verdict)] of a SCRIPTS row."""
    return [tuple(w.rsplit(":", 1)) for w in text.split()]


def single_handle(text):
    """The script uses handle A alone: no map ever moves between handles."""
    return all(o[1] == "A" for o, _ in script_ops(text))


def parse(o):
    """(kind, handle, stream, map, xy, z) of an operation."""
    if o[0] == "X":
        return "X", o[1], None, None, None, None
    if o[0] == "h":
        return o[0] + o[3], o[1], int(o[2]), None, None, None
    if o[0] in "de":
        return o[0], o[1], int(o[2]), None, None, None
    parts = o[4:].split("/")
    xy, z = (int(parts[1]), int(parts[2])) if len(parts) == 3 else (2, 1)
    return o[0], o[1], int(o[2]), int(parts[0]), xy, z


class _Map:
    def __init__(self):
        self.n_attached, self.n_readers, self.attached_to, self.own_stream = 0, 0, None, True


class _Handle:
    def __init__(self, S):
        self.S = S
        self.mappers, self.opts = [None] * S, [None] * S      # opts: (xy, z, lag) the writer was attached with
        self.readers, self.reader_ext, self.read_maps = [], [], []      # empty until the first reader
        self.hit_radius = []      # empty until hits are first switched on
        self.n_lagged = self.n_readers = self.n_hits = 0
        self.sel, self.lag_on = [(0, 0, 0)] * S, [0] * S      # the device words


class Model:
    def __init__(self):
        self.maps = [_Map() for _ in range(N_MAPS)]
        self.handles = {n: _Handle(S) for n, S in HANDLES}

    def clone(self):
        return copy.deepcopy(self)

    # ---- the three helpers of the old liodom_hip.hip ----
    def _attachment(self, h, m, delta, reader, fx):
        mp = self.maps[m]
        if delta > 0:
            if mp.n_attached == 0 or mp.attached_to is not h:
                fx.append("move=%d" % m)
                mp.own_stream, mp.attached_to, mp.n_attached, mp.n_readers = False, h, 0, 0
            mp.n_attached += 1
            mp.n_readers += 1 if reader else 0
            return
        if mp.attached_to is not h:
            return
        if reader and mp.n_readers > 0:
            mp.n_readers -= 1
        if mp.n_attached > 0:
            mp.n_attached -= 1
        if mp.n_attached == 0:
            mp.n_readers, mp.attached_to, mp.own_stream = 0, None, True
            fx.append("own=%d" % m)

    def _others(self, h, s, m):
        own_w = 1 if h.mappers[s] == m else 0
        own_r = 1 if h.readers and h.readers[s] == m else 0
        mp = self.maps[m]
        if mp.attached_to is not h:
            own_w = own_r = 0
        return (mp.n_attached - mp.n_readers) - own_w, mp.n_readers - own_r      # writers, readers

    def _detach(self, h, s, fx):
        old = h.mappers[s]
        if old is not None:
            h.mappers[s] = None
            if h.opts[s][2] == 1:
                h.n_lagged -= 1
            self._attachment(h, old, -1, False, fx)
        if h.readers and h.readers[s] is not None:
            old = h.readers[s]
            h.readers[s] = None
            h.n_readers -= 1
            h.sel[s] = (0, 0, 0)
            fx.append("clr=1")
            if old not in h.readers:
                h.read_maps = [None if q == old else q for q in h.read_maps]
            self._attachment(h, old, -1, True, fx)

    # ---- the entry points ----
    def op(self, o):
        kind, hn, s, m, xy, z = parse(o)
        h, fx = self.handles[hn], []
        if kind == "X":
            for vec in (h.mappers, h.readers):
                for q in vec:
                    if q is None or self.maps[q].n_attached == 0 or self.maps[q].attached_to is not h:
                        continue
                    mp = self.maps[q]
                    mp.n_attached, mp.n_readers, mp.attached_to, mp.own_stream = 0, 0, None, True
                    fx.append("own=%d" % q)
            self.handles[hn] = _Handle(h.S)
            return "ok " + (" ".join(fx) or "-")
        if kind in ("h+", "h-"):
            radius = 0 if kind == "h+" else -1
            if not h.hit_radius:
                if radius < 0:
                    return "ok -"
                h.hit_radius = [-1] * h.S
            if radius >= 0 and h.readers and h.readers[s] is not None:
                fx.append("occ=1")
            h.n_hits += (1 if radius >= 0 else 0) - (1 if h.hit_radius[s] >= 0 else 0)
            h.hit_radius[s] = radius
            return "ok " + (" ".join(fx) or "-")
        if kind == "r":
            writers, _ = self._others(h, s, m)
            if writers > 0:
                return "is_written -"
            if self.maps[m].n_attached > 0 and self.maps[m].attached_to is not h:
                return "other_handle -"
            if not h.readers:
                h.readers, h.reader_ext = [None] * h.S, [(0, 0)] * h.S
            if h.n_hits > 0 and h.hit_radius[s] >= 0:
                fx.append("occ=1")
            self._attachment(h, m, +1, True, fx)
            self._detach(h, s, fx)
            if m not in h.read_maps:
                if None in h.read_maps:
                    h.read_maps[h.read_maps.index(None)] = m
                else:
                    h.read_maps.append(m)
            t = h.read_maps.index(m)
            h.readers[s], h.reader_ext[s] = m, (xy, z)
            h.n_readers += 1
            h.sel[s] = (t + 1, xy, z)
            fx.append("sel=%d,%d,%d" % h.sel[s])
            fx.append("lag=-1")
            return "ok " + " ".join(fx)
        lag = 1 if kind == "l" else 0
        if m is not None:
            _, readers = self._others(h, s, m)
            if readers > 0:
                return "is_read -"
            self._attachment(h, m, +1, False, fx)
        self._detach(h, s, fx)
        if m is not None:
            h.mappers[s], h.opts[s] = m, (xy, z, lag)
            h.n_lagged += lag
        h.lag_on[s] = lag if m is not None else 0
        fx.append("lag=%d" % h.lag_on[s])
        return "ok " + " ".join(fx)

    def state(self):
        out = []
        for hn, S in HANDLES:
            h = self.handles[hn]
            for s in range(S):
                w, r = h.mappers[s], h.readers[s] if h.readers else None
                assert w is None or r is None
                att = "w%d/%d/%d/%d" % ((w,) + h.opts[s]) if w is not None else "r%d/%d/%d" % ((r,) + h.reader_ext[s]) if r is not None else "-"
                out.append("%s%d=%s:h%d:t%d,%d,%d:g%d" % ((hn, s, att, h.hit_radius[s] if h.hit_radius else -1) + h.sel[s] + (h.lag_on[s],)))
        for hn, _ in HANDLES:
            h = self.handles[hn]
            out.append("tags%s=%s" % (hn, ",".join("." if q is None else str(q) for q in h.read_maps) or "-"))
            out.append("cnt%s=%d,%d,%d" % (hn, h.n_lagged, h.n_readers, h.n_hits))
        for k, mp in enumerate(self.maps):
            holder = "-" if mp.attached_to is None else next((n for n, h in self.handles.items() if h is mp.attached_to), "?")
            out.append("m%d=%d/%d/%s" % (k, mp.n_attached, mp.n_readers, holder))
        return " ".join(out)

    def attached(self, m):
        """What liodom_map_import_state / liodom_map_reset answer LIODOM_ERR_BUSY to."""
        return not self.maps[m].own_stream
