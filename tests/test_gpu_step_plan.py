"""The launches of a step against the counts recorded before they were planned in step_plan.h (tests/step_launches_mi355x.json,
tools/record_step_launches.py): every scenario of tests/step_scenarios.py runs with per-kernel profiling on from the start, and
liodom_get_kernel_stats must count per bucket what the recording counted.  The recording is of one device: on a GPU with another
CU count the whole file skips.  Run with -m gpu on an MI355X."""
import json
import os

import pytest

import liodom_amd as la
import step_scenarios as ss
from liodom_amd import synth

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_launches_mi355x.json")) as _f:
    FIXTURE = json.load(_f)["scenarios"]


@pytest.fixture(scope="module")
def recorded_device():
    g = la.Liodom(la.make_params(scan_lines=4, scan_regions=4, edges_per_region=3), la.make_config(max_points=1024, max_width=256))
    _, cus = g.device_info()
    g.close()
    want = {e["cus"] for e in FIXTURE.values()}
    if want != {cus}:
        pytest.skip("the launches were recorded on a device of %s CUs, this one has %d" % (sorted(want), cus))


@pytest.mark.parametrize("name", ss.NAMES)
def test_buckets_count_what_was_recorded(recorded_device, monkeypatch, name):
    assert set(ss.NAMES) == set(FIXTURE)
    sc = ss.SCENARIOS[ss.NAMES.index(name)]
    for k in [k for k in os.environ if k.startswith("LIODOM_")]:
        monkeypatch.delenv(k)
    for k, v in ss.entry_of(sc)[4].items():
        monkeypatch.setenv(k, v)
    g = ss.run(la, synth, sc, profiling=True)
    try:
        got = {k: v[0] for k, v in g.kernel_stats().items()}
    finally:
        g.close()
    assert got == FIXTURE[name]["counts"], (name, {k: (v, FIXTURE[name]["counts"].get(k)) for k, v in got.items() if FIXTURE[name]["counts"].get(k) != v})
