"""Short runs of API calls whose launches are recorded in tests/step_launches_mi355x.json (tools/record_step_launches.py) and
replayed by tests/test_step_plan.py (the plan of a scan's launches alone, liodom_amd/csrc/step_plan.h, no GPU) and
tests/test_gpu_step_plan.py (the library's per-bucket launch counts on the device).

A scenario is (name, handle, calls): a handle of tests/handle_matrix.py (its switches included) and a list of calls:
  ("profiling",)                       set_profiling(1)
  ("imu",)                             set_imu of a small rotation, stream 0
  ("mapper", lag, prune_period)        attach_mapper of a fresh map to stream 0
  ("reader",)                          attach_map_reader of a fresh, filled map to stream 0
  ("scan", stream)                     process_scan
  ("replay", first_slot, count)        replay_resident, depth 1
  ("step", slot, next_slot)            process_resident (pipelined, poses read back)
  ("subset", slot, streams, next_slot, next_streams)   process_resident_subset
  ("ticket",)                          extract_edges_device + odometry_submit_device
  ("collect",)                         odometry_collect
  ("sync",)
Every pose is collected before anything can flush the chain, so whether a repair launch is issued depends on the recorded
verdict alone (the fixture's "confirmed").

requests() states which plan requests each call issues: the glue of the entry points around launch_extract and
enqueue_odometry (edge-buffer parity, the extraction issued ahead), as lines for tests/step_plan_main.cc."""
import numpy as np

import handle_matrix as hm


def slots_of(calls):
    """Resident slots the calls name."""
    top = 0
    for c in calls:
        if c[0] == "replay":
            top = max(top, c[1] + c[2])
        elif c[0] == "step":
            top = max(top, c[1] + 1, c[2] + 1)
        elif c[0] == "subset":
            top = max(top, c[1] + 1, c[3] + 1)
    return top


def _one_stream(handle, replay=4):
    return (handle, handle, [("scan", 0), ("replay", 0, replay), ("scan", 0), ("sync",)])


def _lockstep(handle, steps=2):
    return (handle, handle, [("step", k, k + 1) for k in range(steps)] + [("sync",)])


SCENARIOS = [
    # two warm-up scans, overlapped / chain scans, a scan that leaves chain mode, two scans by ticket in flight together
    ("hdl64", "hdl64", [("scan", 0), ("replay", 0, 6), ("scan", 0), ("ticket",), ("ticket",), ("collect",), ("collect",), ("sync",)]),
    _one_stream("ouster128"),
    _one_stream("h128-epr12"),
    _one_stream("vlp16"),
    ("s4", "s4", [("step", 0, 1), ("step", 1, 2), ("step", 2, -1), ("scan", 1), ("sync",)]),
    _one_stream("hdl64 LIODOM_SPECULATE=0"),
    _one_stream("hdl64 LIODOM_EARLY_REBUILD=0", 3),
    _one_stream("hdl64 LIODOM_PIPE_FLAGS=0", 3),
    _one_stream("hdl64 LIODOM_SAFE_MODE=1", 3),
    _lockstep("s16 LIODOM_HASH_BUILD=global"),
    _one_stream("pose-cov"),
    _one_stream("filter", 3),
    ("imu", "imu", [("imu",), ("scan", 0), ("replay", 0, 3), ("sync",)]),
    ("mapping-lagged", "mapping", [("mapper", 1, 2), ("scan", 0), ("scan", 0), ("replay", 0, 2), ("sync",)]),
    ("mapping-reader", "mapping", [("reader",), ("scan", 0), ("replay", 0, 2), ("sync",)]),
    # nine steps cross kHbPeriod twice; a subset step with another list issued ahead; one stream of the batch alone
    ("s16", "s16", [("step", k, k + 1) for k in range(9)] +
     [("subset", 9, [1, 4, 7], 0, [2, 3]), ("subset", 0, [2, 3], -1, None), ("scan", 5), ("sync",)]),
    _lockstep("s256"),                      # 512 tiles: over k_ring_split's budget, k_ring_split_lb + k_ring_split_fix
    _lockstep("s16-window4"),
    _lockstep("s16-lidar1"),
    _lockstep("s16 LIODOM_KNN8=0"),
    ("hdl64-profiling", "hdl64", [("profiling",), ("scan", 0), ("replay", 0, 3), ("scan", 0), ("sync",)]),
]
NAMES = [s[0] for s in SCENARIOS]
assert len(set(NAMES)) == len(NAMES)


def entry_of(scenario):
    return hm.MATRIX[hm.NAMES.index(scenario[1])]


def shape_of(entry):
    """(H, W, points per scan, streams, lidar_type) of the handle's clouds."""
    _, _, p, c, _ = entry
    H = p["scan_lines"]
    W = c["max_width"]
    return H, W, H * W, c.get("n_streams", 1), p.get("lidar_type", 0)


def run(la, synth, scenario, profiling=False):
    """The scenario on the device.  The caller has set the handle's switches (and no other LIODOM_* variable).  Returns the
    handle, still open, after the last call."""
    _, _, calls = scenario
    entry = entry_of(scenario)
    H, W, n, S, lidar = shape_of(entry)
    g = hm.create(la, entry)
    if profiling:
        g.set_profiling(1)
    cfg = synth.make_cfg(H, W, lidar)
    clouds = {}

    def cloud(s, k):
        if (s, k) not in clouds:
            clouds[(s, k)] = synth.scan(cfg, s, k)[0]
        return clouds[(s, k)]

    if slots_of(calls):
        g.alloc_resident(slots_of(calls))
        for k in range(slots_of(calls)):
            for s in range(S):
                g.upload_scan(s, k, cloud(s, k))
    keep, tickets, nscan = [], [], 0
    for c in calls:
        if c[0] == "profiling":
            g.set_profiling(1)
        elif c[0] == "imu":
            g.set_imu(np.array([0.0, 0.0, 0.01, 1.0]) / np.sqrt(1.0001))
        elif c[0] == "mapper":
            m = la.Map(40.0, 50.0, 0.4, max_cells=256, cell_capacity=65536)
            keep.append(m)
            g.attach_mapper(m, lag=c[1], prune_period=c[2], keep_cells_xy=2, keep_cells_z=1)
        elif c[0] == "reader":
            m = la.Map(40.0, 50.0, 0.4, max_cells=256, cell_capacity=65536)
            keep.append(m)
            m.update(cloud(0, 0)[::16])
            g.attach_map_reader(m)
        elif c[0] == "scan":
            g.process_scan(cloud(c[1], 20 + nscan), H, W, stream=c[1])
            nscan += 1
        elif c[0] == "replay":
            g.replay_resident(c[1], c[2], n, H, W, depth=1)
        elif c[0] == "step":
            g.process_resident(c[1], n, H, W, next_slot=c[2])
        elif c[0] == "subset":
            g.process_resident_subset(c[1], c[2], n, H, W, next_slot=c[3], next_streams=c[4])
        elif c[0] == "ticket":
            t = g.extract_edges_device(cloud(0, 30 + nscan), H, W)
            nscan += 1
            assert t is not None and g.odometry_submit_device(t)
            tickets.append(t)
        elif c[0] == "collect":
            g.odometry_collect()
        elif c[0] == "sync":
            g.sync()
        else:
            raise ValueError(c)
    g._step_keep = keep
    return g


def requests(scenario, confirmed=True, profiling=False):
    """The scenario's plan requests, one line each, in the order the entry points issue them:
      x q=<o|x> s0= count= n= width=          launch_extract (s0 < 0: a stream list; q: the queue, for the stream's role)
      o s0= count= pipe=<0|1> [list=a,b,..]   launch_odometry; pipe: through enqueue_pipeline_odometry
      c lag= confirmed=                       wait_pose that includes stream 0 (it notes the scan's verdict)
      f                                       chain_flush (liodom_sync, drain_pipeline with scans in the pipeline)
      p                                       profiling on
      m lagged=<0|1>                          a mapper has been attached to stream 0
      set reader=1                            a map reader has been attached"""
    _, _, calls = scenario
    H, W, n, S, _ = shape_of(entry_of(scenario))
    out = ["p"] if profiling else []
    prof = profiling
    parity, pf_slot, pf_list, live, pending = 0, -1, None, False, 0
    conf = 1 if confirmed else 0
    full = list(range(S))

    def extract(s0, count, pipelined):
        out.append("x q=%s s0=%d count=%d n=%d width=%d" % ("x" if pipelined and not prof else "o", s0, count, n, W))

    def drain():
        nonlocal parity, pf_slot, pf_list, live
        if pf_slot >= 0 or parity != 0 or live:
            out.append("f")
            parity, pf_slot, pf_list, live = 0, -1, None, False

    def step(slot, streams, next_slot, next_streams, wait, lag=0):
        nonlocal parity, pf_slot, pf_list, live
        live = True
        eb = parity
        if streams:
            if not (pf_slot == slot and pf_list == streams):
                extract(0 if streams == full else -eb - 1, len(streams), True)
            pf_slot, pf_list = -1, None
            if streams == full:
                out.append("o s0=0 count=%d pipe=1" % S)
            else:
                out.append("o s0=%d count=%d pipe=1 list=%s" % (-(3 + eb) - 1, len(streams), ",".join(map(str, streams))))
            parity = (eb + 1) % 3
        if next_slot >= 0:
            nx = streams if next_streams is None else next_streams
            if nx:
                extract(0 if nx == full else -parity - 1, len(nx), True)
            pf_slot, pf_list = next_slot, nx
        if wait and streams and 0 in streams:
            out.append("c lag=%d confirmed=%d" % (lag, conf))

    for c in calls:
        if c[0] == "profiling":
            prof = True
            out.append("p")
        elif c[0] == "mapper":
            out.append("m lagged=%d" % c[1])
        elif c[0] == "reader":
            out.append("set reader=1")
        elif c[0] == "scan":
            drain()
            extract(c[1], 1, False)
            out.append("o s0=%d count=1 pipe=0" % c[1])
            if c[1] == 0:
                out.append("c lag=0 confirmed=%d" % conf)
        elif c[0] == "replay":
            for i in range(c[2]):
                step(c[1] + i, full, c[1] + i + 1 if i + 1 < c[2] else -1, None, False)
                if i > 0:
                    out.append("c lag=1 confirmed=%d" % conf)
            out.append("c lag=0 confirmed=%d" % conf)
        elif c[0] == "step":
            step(c[1], full, c[2], None, True)
        elif c[0] == "subset":
            step(c[1], list(c[2]), c[3], None if c[4] is None else list(c[4]), True)
        elif c[0] == "ticket":
            extract(0, 1, True)
            out.append("o s0=0 count=1 pipe=1")
            live = True
            pending += 1
        elif c[0] == "collect":
            pending -= 1
            out.append("c lag=%d confirmed=%d" % (pending, conf))
        elif c[0] == "sync":
            out.append("f")
            if pf_slot < 0:
                parity, live = 0, False
    return out
