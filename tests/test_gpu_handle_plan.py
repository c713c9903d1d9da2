"""liodom_create against the decisions recorded before the plan moved into handle_plan.h (tests/handle_modes_mi355x.json,
tools/record_handle_modes.py): every handle of tests/handle_matrix.py is created with its switches set and the full text of
liodom_get_modes, taken right after creation, must be the recorded one.  The recording is of one device: on a GPU with another CU
count the whole file skips.  Run with -m gpu on an MI355X."""
import json
import os

import pytest

import handle_matrix as hm
import liodom_amd as la

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "handle_modes_mi355x.json")) as _f:
    FIXTURE = {e["name"]: e for e in json.load(_f)}


@pytest.fixture(scope="module")
def recorded_device():
    g = la.Liodom(la.make_params(scan_lines=4, scan_regions=4, edges_per_region=3), la.make_config(max_points=1024, max_width=256))
    _, cus = g.device_info()
    g.close()
    want = {e["cus"] for e in FIXTURE.values()}
    if want != {cus}:
        pytest.skip("the decisions were recorded on a device of %s CUs, this one has %d" % (sorted(want), cus))


def check_group(group, monkeypatch):
    for k in [k for k in os.environ if k.startswith("LIODOM_")]:
        monkeypatch.delenv(k)
    for entry in hm.MATRIX:
        if entry[0] != group:
            continue
        name, switches = entry[1], entry[4]
        for k, v in switches.items():
            monkeypatch.setenv(k, v)
        g = hm.create(la, entry)
        for k in switches:
            monkeypatch.delenv(k)
        got = hm.modes_string(g)
        g.close()
        want = FIXTURE[name]["modes"]
        m = hm.parse_modes(got)
        assert m[hm.PROBE_KEY] == hm.parse_modes(want)[hm.PROBE_KEY], \
            "%s: streams_concurrent=%s where the recording has 1: the concurrency probe failed (a busy GPU?)" % (name, m[hm.PROBE_KEY])
        assert got == want, (name, [(k, v, hm.parse_modes(want).get(k)) for k, v in m.items() if hm.parse_modes(want).get(k) != v])


@pytest.mark.parametrize("group", ["shape", "params", "switches"])
def test_create_decides_what_was_recorded(recorded_device, monkeypatch, group):
    assert {e[0] for e in hm.MATRIX} == {"shape", "params", "switches"} and set(hm.NAMES) == set(FIXTURE)
    check_group(group, monkeypatch)
