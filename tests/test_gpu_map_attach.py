"""Which map is attached to which stream, as what, through the C-ABI: the designed scripts of tests/map_attach_cases.py on a
two-stream and a one-stream mapping handle and two small maps.  After every call: the return code and the liodom_last_error() text
the verdict stands for, the three counters of liodom_get_modes, and for each map whether liodom_map_import_state of its own export
answers LIODOM_ERR_BUSY (attached) or succeeds with the same bytes.  A script that stays on one handle ends with one scan per
stream: a reader's received map is getLocalMap of the map it reads at the scan's pose, a lag-0 writer's that of its map after the
update, and a stream without a map keeps what it had.  Scripts in which a map moves between handles run no scan: a step of a
handle that has lost its map would enqueue onto the other handle's stream without ordering."""
import ctypes as C

import pytest

import liodom_amd as la
from liodom_amd import api
import map_attach_cases as mc
from mapper_lag_common import H, W, T_of, same, scans_of
from test_gpu_localize import CAPS, _handle

pytestmark = pytest.mark.gpu

# code and text of each refusal, as the library gave them before map_attach.h existed
REFUSALS = {
    "is_read": (api.ERR_INVALID_ARG, "liodom_attach_mapper: the map is attached reading (liodom_attach_map_reader): a map is read or written, not both"),
    "is_written": (api.ERR_INVALID_ARG, "liodom_attach_map_reader: the map is attached writing (liodom_attach_mapper): a map is read or written, not both"),
    "other_handle": (api.ERR_INVALID_ARG, "liodom_attach_map_reader: the map is attached to another handle"),
}


@pytest.fixture(scope="module")
def world(synth):
    """The scans, and two maps that differ, each filled by two updates."""
    scans = scans_of(synth, 0, 4)
    g = _handle()
    edges = [g.extract_edges(x, H, W)["edges"] for x in scans]
    g.close()
    maps = [la.Map(**CAPS) for _ in range(mc.N_MAPS)]
    for k, m in enumerate(maps):
        T = T_of([0.0, 0.0, 0.0, 1.0, 0.5 * k, 0.0, 0.0])
        m.update(edges[2 * k], T)
        m.update(edges[2 * k + 1], T)
        assert m.local(None, 2, 1).shape[0] > 0 and m.status() == 0
    assert maps[0].export_state() != maps[1].export_state()
    yield scans, maps
    for m in maps:
        m.close()


def call(g, o, maps):
    kind, _, s, m, xy, z = mc.parse(o)
    if kind in ("h+", "h-"):
        return g.L.liodom_set_map_hits(g.h, s, 0 if kind == "h+" else -1)
    if kind == "d":
        return g.L.liodom_attach_mapper(g.h, s, None, 2, 1)
    if kind == "e":
        return g.L.liodom_attach_map_reader(g.h, s, None, 2, 1)
    if kind == "r":
        return g.L.liodom_attach_map_reader(g.h, s, maps[m].h, xy, z)
    if kind == "w":
        return g.L.liodom_attach_mapper(g.h, s, maps[m].h, xy, z)
    return g.L.liodom_attach_mapper_ex(g.h, s, maps[m].h, C.byref(api.make_mapper_options(cells_xy=xy, cells_z=z, lag=1)))


@pytest.mark.parametrize("name,text", mc.SCRIPTS, ids=[n for n, _ in mc.SCRIPTS])
def test_script(world, name, text):
    scans, maps = world
    blobs = [m.export_state() for m in maps]
    hs = {n: _handle(S) for n, S in mc.HANDLES}
    model = mc.Model()
    try:
        for o, verdict in mc.script_ops(text):
            hn = o[1]
            if o[0] == "X":
                hs[hn].close()
                hs[hn] = _handle(dict(mc.HANDLES)[hn])
                rc = 0
            else:
                rc = call(hs[hn], o, maps)
            assert model.op(o).split()[0] == verdict, (o, verdict)
            if verdict == "ok":
                assert rc == 0, (o, rc, hs[hn].L.liodom_last_error())
            else:
                assert (rc, hs[hn].L.liodom_last_error().decode()) == REFUSALS[verdict], o
            for n, _ in mc.HANDLES:
                modes, mh = hs[n].modes(), model.handles[n]
                got = tuple(int(modes.get(k, "0")) for k in ("mapper_lag", "map_readers", "map_hits"))
                assert got == (mh.n_lagged, mh.n_readers, mh.n_hits), (o, n, modes)
            for k, m in enumerate(maps):
                if model.attached(k):
                    with pytest.raises(la.LiodomError) as err:
                        m.import_state(blobs[k])
                    assert err.value.code == api.ERR_BUSY, (o, k)
                else:
                    m.import_state(blobs[k])
                    assert m.export_state() == blobs[k], (o, k)
        if mc.single_handle(text):
            g, mh = hs["A"], model.handles["A"]
            for s in range(mh.S):
                before = g.received_map(stream=s)
                pose, _ = g.process_scan(scans[s], H, W, stream=s)
                got = g.received_map(stream=s)
                w, r = mh.mappers[s], mh.readers[s] if mh.readers else None
                if r is not None:
                    assert got.shape[0] > 0 and same(got, maps[r].local(T_of(pose), *mh.reader_ext[s])), (name, s)
                    assert maps[r].export_state() == blobs[r], (name, s)
                elif w is not None and mh.opts[s][2] == 0:
                    assert maps[w].export_state() != blobs[w], (name, s)
                    assert got.shape[0] > 0 and same(got, maps[w].local(T_of(pose), *mh.opts[s][:2])), (name, s)
                elif w is None:
                    assert same(got, before), (name, s)
    finally:
        for n, S in mc.HANDLES:
            for s in range(S):
                hs[n].L.liodom_attach_mapper(hs[n].h, s, None, 2, 1)
            hs[n].close()
        for k, m in enumerate(maps):      # the maps as they were, for the next script
            m.import_state(blobs[k])
