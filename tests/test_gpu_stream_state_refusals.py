"""liodom_import_stream_state refuses what stream_state_validate (csrc/stream_state_format.h) refuses, with its code, and a refusal
leaves the stream as it was: every refusal of stream_state_cases.py that can be made from a real export for the handle that made
it, each offered at an aligned and at an odd address.  (A received map above recv_capacity needs a mapping handle:
test_gpu_stream_state.py::test_round_trip_mapping.)  Run with -m gpu on an MI355X."""
import ctypes as C

import pytest

import stream_state_cases as ssc
from test_gpu_stream_state import DIMS, bits, clean_env, logs_of, open_handle

pytestmark = pytest.mark.gpu


def test_every_refusal_returns_its_code_and_leaves_the_stream_untouched(orc, synth, monkeypatch):
    clean_env(monkeypatch)
    H, W, P = DIMS[0], DIMS[1], DIMS[5]
    scans = logs_of(synth, DIMS, [3], 5)[0]
    _, g = open_handle(orc, DIMS)
    for x in scans[:4]:
        g.process_scan(x, H, W)
    want_next = bits(g.process_scan(scans[4], H, W)[0])          # the uninterrupted handle
    g.close()
    _, g = open_handle(orc, DIMS)
    for x in scans[:4]:
        g.process_scan(x, H, W)
    blob = g.export_stream_state(0)
    # the handle's capacities, from the size of its largest blob: points_offset + 16 * (local_map_size * edge_cap + recv_cap), recv_cap 0
    pts_off = ssc.COUNTS + 4 * ((P + 3) // 4 * 4)
    edge_cap, rest = divmod(g.stream_state_size() - pts_off, 16 * P)
    assert rest == 0 and edge_cap >= max(ssc.counts_of(blob))
    taker = ssc.Taker(ssc.fingerprint_of(blob), False, edge_cap, 0)
    assert taker.fingerprint[0] == P and taker.fingerprint[1] == 0
    refusals = [c for c in ssc.cases(blob, taker) if c.taker == taker and c.code != ssc.OK]
    assert len(refusals) >= 25 and {c.code for c in refusals} == {ssc.INVALID_ARG, ssc.CAPACITY}
    for c in refusals:
        n = len(c.blob)
        for odd in (0, 1):
            buf = (C.c_ubyte * (n + odd))()
            C.memmove(C.addressof(buf) + odd, c.blob, n)
            rc = g.L.liodom_import_stream_state(g.h, 0, C.c_void_p(C.addressof(buf) + odd), n)
            assert rc == c.code, (c.name, odd, rc, g.L.liodom_last_error())
    assert g.export_stream_state(0) == blob                       # nothing of them reached the stream
    assert bits(g.process_scan(scans[4], H, W)[0]) == want_next
    g.close()
