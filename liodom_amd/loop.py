"""LoopCloser: key frames, their pose graph, and the correction of a detected revisit.

A host loop over existing calls, as MapPager is: PlacePolicy picks the key frames, a Places database finds the key frame a new one
was taken near, Map.search_pose measures the pose in the map, a PoseGraph holds the key frames with their odometry and loop edges,
and close() optimises it and applies the result — the map is rebuilt from the key frames' clouds at the corrected poses, the poses
in the place database are rewritten, the stream is seeded again.  Nothing is computed here but pose compositions.

A false loop edge — the descriptor has no roll, pitch or height term, and a site with repeated structure will produce one — bends
the whole graph under the plain quadratic cost.  close(loss=(name, scale), reject_below=r) is the answer to that: a first solve
with a robust loss on the loop edges (kind 1), the loop edges whose weight collapsed below r switched off, and a second, plain
quadratic solve over the survivors from the robust result, which takes the robust loss's bias off them.

A searched pose is a grid cell: x, y, yaw as fine as the last level's step, no roll, pitch or z.  LoopCloser(refine=dict(...))
registers it to the map in 6-DoF first (Map.register_poses, refine_loop) and measures the loop edge with the registered pose;
loop_info="solve" then weighs the edge by what that registration's solve knows, instead of a constant.

What close() cannot do: scans that were no key frames are not in the rebuilt map (their clouds are not kept); without refine a
loop measurement is as fine as the last search level's step.  The robust solve is only as good as its scale, which is in units of sqrt(chi2) of
a loop edge: it has to exceed what honest drift puts on a TRUE loop edge at the dead-reckoned poses, or the true edges are
down-weighted with the false one and the solve settles in the wrong minimum (DESIGN.md §3 "Closing loops" has a ring of 8 key
frames on which Geman-McClure with scale 3 rejects every true loop and scale 5 does not).  And it rejects by consensus: where
false loop edges agree with each other and outnumber the true ones, they win.  LoopCloser(gate=16.81) asks the graph first: a
loop candidate whose squared Mahalanobis distance from the relative pose the graph predicts — under the graph's own covariance,
PoseGraph.gate_edges — exceeds the gate is never added.  That needs no consensus, and is only as calibrated as odometry_info.
"""
import math

import numpy as np

from . import api

ODOMETRY_INFO = np.diag([400.0, 400.0, 400.0, 100.0, 100.0, 100.0])     # half-angle rotation first, then translation [1 / m^2]
LOOP_INFO = np.diag([400.0, 400.0, 400.0, 100.0, 100.0, 100.0])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _pose(p):
    p = np.array(p, np.float64).reshape(7)
    p[:4] /= math.sqrt(float(np.sum(p[:4] * p[:4])))
    return p


def compose(X, Y):
    """X o Y of two poses [qx qy qz qw tx ty tz]."""
    X, Y = _pose(X), _pose(Y)
    return np.concatenate([_qmul(X[:4], Y[:4]), api.pose_T34(X)[:, :3] @ Y[4:] + X[4:]])


def inverse(X):
    X = _pose(X)
    return np.concatenate([[-X[0], -X[1], -X[2], X[3]], -(api.pose_T34(X)[:, :3].T @ X[4:])])


def between(Xi, Xj):
    """X_i^-1 o X_j: what an edge (i, j) of the graph measures."""
    return compose(inverse(Xi), Xj)


def edge_jacobian_j(Xi, Xj, Z):
    """B = de / d(delta_j) of graph_edge_error (liodom_math.h) at (X_i, X_j, Z): [[Q, 0], [0, W]] with W = R_z^T R_i^T and
    Q[:, k] = s vec(conj(q_z) (x) conj(q_i) (x) [e_k, 0] (x) q_j), s the sign of the error quaternion's w."""
    Xi, Xj, Z = _pose(Xi), _pose(Xj), _pose(Z)
    conj = lambda q: np.array([-q[0], -q[1], -q[2], q[3]])
    a = _qmul(conj(Z[:4]), conj(Xi[:4]))
    s = 1.0 if _qmul(a, Xj[:4])[3] >= 0 else -1.0
    B = np.zeros((6, 6))
    for k in range(3):
        e = np.zeros(4)
        e[k] = 1.0
        B[:3, k] = s * _qmul(_qmul(a, e), Xj[:4])[:3]
    B[3:, 3:] = api.pose_T34(Z)[:, :3].T @ api.pose_T34(Xi)[:, :3].T
    return B


def solve_information(place_pose, registered_pose, Z, H, sigma2):
    """The information of the loop edge "X_place^-1 o X_registered was measured as Z" from the registration's solve: the pose's
    covariance is sigma2 H^-1 in the solver's tangent, which is the graph's, and the edge's error moves by e = B delta_j, so
    Omega = B^-T (H / sigma2) B^-1.  Symmetric by construction (the two halves are averaged against rounding)."""
    Binv = np.linalg.inv(edge_jacobian_j(place_pose, registered_pose, Z))
    om = Binv.T @ (np.asarray(H, np.float64).reshape(6, 6) / float(sigma2)) @ Binv
    return 0.5 * (om + om.T)


class LoopCloser:
    """LoopCloser(map, places, levels, ...): feed(pose, edges, scan=None) per scan, close() when loops have been found.

    map, places   the Map the loop measurements are searched in and the Places database of the key frames
    levels        the grids of Map.search_pose, coarse to fine, run around a match's pose (as Liodom.relocalize's)
    graph         a PoseGraph (made here with max_nodes / max_edges if None)
    min_dist, min_yaw   the key-frame policy (PlacePolicy)
    min_gap       a key frame enters `places` only when min_gap newer key frames exist: a query never returns the recent past
    k             matches asked of the database per key frame
    min_fraction  a match becomes a loop edge if its last level scores (hits_r + hits_0) / (2 n_edges) >= min_fraction
    odometry_info, loop_info   the information matrices (6 x 6, half-angle rotation first) of the two kinds of edge
                  odometry_info="solve" (needs odometry_source=(handle, stream), a handle created with pose_covariance = 1): the
                  information of an odometry edge is chained on the device from the covariance records of the scans between the
                  two key frames (Liodom.odometry_edges for the interval (the previous key frame's scan, this key frame's scan);
                  feed's `scan` is the scan index the handle gave the pose, info.scan_index), with odometry_options — inflation,
                  floor_rotation, floor_translation; tools/odometry_info_calibration.py measures the inflation a sensor and scene call
                  for.  Z stays between(the fed poses): Omega does not depend on the frame the log's poses are in.
                  ODOMETRY_INFO stands, and odometry_fallbacks counts it, where feed got no scan, the scan index did not
                  increase (the first key frame after close() has seeded the stream again), the call was refused, or the record's
                  flags are not exactly ODOM_EDGE_VALID (scans without a usable record: GAPS).
    refine        None, or dict(options of Map.register_poses, min_fraction=...): a searched pose is registered to the map in 6-DoF
                  (refine_loop) and the loop edge measures the registered pose; it is kept only if the registration ended CONVERGED
                  or MAX_PASSES with matches / n_edges >= refine's min_fraction (default 0.25)
                  loop_info="solve" (needs refine): the edge's information is solve_information of the registration; where that
                  is not defined (flags other than COV_VALID) LOOP_INFO stands
    max_update_points          points per Map.update call of the rebuild
    gate          None, or a threshold on d2 (PoseGraph.gate_edges): before feed() or add_loop() adds a loop edge, its squared
                  Mahalanobis distance d2 from the relative pose the graph predicts — under the graph's own covariance at the
                  current poses plus the edge's — is computed on the device, and the edge is added only if the status is "ok" and
                  d2 <= gate.  16.81 is the 0.99 quantile of chi-square with 6 degrees of freedom: a true loop is then refused one
                  time in a hundred — IF the information matrices are honest.  d2 is only as calibrated as odometry_info is: a
                  constant that understates the drift makes true loops look like outliers, one that overstates it lets false ones
                  pass.  gate_options: keywords of api.make_graph_cov_options for that call.  None: nothing is computed, every
                  candidate is added, as before the gate existed.

    `places` must be this LoopCloser's alone: empty when it is handed in, and filled by feed() only — a place's tag is its key
    frame's node index, and close() rewrites the poses by it (it raises ValueError, before anything is changed, if the database
    holds anything else).

    feed returns dict(key_frame, node, loops): loops = [dict(place, node, fraction, pose, match)] of the edges added; with a gate
    each carries d2.  gated: [(place, node, d2, status)] of the loop edges the gate refused (status one of api.GRAPH_COV_STATUSES).
    key_poses: the key frames' poses as fed (after close(): as corrected); clouds: their edge clouds (sensor frame)."""

    def __init__(self, map, places, levels, graph=None, min_dist=4.0, min_yaw=float("inf"), min_gap=10, k=3, min_fraction=0.5,
                 odometry_info=ODOMETRY_INFO, loop_info=LOOP_INFO, max_update_points=65536, max_nodes=4096, max_edges=16384, refine=None,
                 gate=None, gate_options=None, odometry_source=None, odometry_options=None):
        if min_gap < 1 or k < 1:
            raise ValueError("LoopCloser: needs min_gap >= 1 and k >= 1")
        self.info_from_solve = isinstance(loop_info, str)
        if self.info_from_solve:
            if loop_info != "solve" or refine is None:
                raise ValueError("LoopCloser: loop_info is a 6 x 6 matrix, or \"solve\" together with refine")
            loop_info = LOOP_INFO
        self.odometry_from_solve = isinstance(odometry_info, str)
        if self.odometry_from_solve:
            if odometry_info != "solve" or odometry_source is None:
                raise ValueError("LoopCloser: odometry_info is a 6 x 6 matrix, or \"solve\" together with odometry_source=(handle, stream)")
            odometry_info = ODOMETRY_INFO
        elif odometry_source is not None or odometry_options:
            raise ValueError("LoopCloser: odometry_source and odometry_options go with odometry_info=\"solve\"")
        self.odometry_source = None if odometry_source is None else (odometry_source[0], int(odometry_source[1]))
        self.odometry_options = dict(odometry_options or {})
        self.odometry_fallbacks = 0      # odometry edges that got the constant although odometry_info="solve"
        self.last_key_scan = None        # the scan index fed with the last key frame (None: none was)
        self.refine = None if refine is None else dict(refine)
        self.refine_min_fraction = float(self.refine.pop("min_fraction", 0.25)) if self.refine is not None else None
        self.map, self.places, self.levels = map, places, list(levels)
        self.graph = api.PoseGraph(max_nodes, max_edges) if graph is None else graph
        self.policy = api.PlacePolicy(min_dist, min_yaw)
        self.min_gap, self.k, self.min_fraction = int(min_gap), int(k), float(min_fraction)
        self.odometry_info = np.array(odometry_info, np.float64).reshape(6, 6)
        self.loop_info = np.array(loop_info, np.float64).reshape(6, 6)
        self.max_update_points = int(max_update_points)
        self.key_poses, self.clouds = [], []
        self.inserted = 0                # key frames 0 .. inserted - 1 are in `places`
        self.loops = []                  # (place node, node) of every active loop edge, in the graph's edge order
        self.rejected = []               # (place node, node, weight) of the loop edges close() has switched off
        self.last_pose = None            # the last pose fed, key frame or not
        self.gate = None if gate is None else float(gate)
        self.gate_options = dict(gate_options or {})
        self.gated = []                  # (place node, node, d2, status) of the loop edges the gate refused

    def odometry_information(self, scan):
        """The information of the odometry edge from the last key frame to a key frame taken at scan index `scan`: with
        odometry_info="solve" the chained one (see the class), else — and wherever that is not to be had, counted in
        odometry_fallbacks — the constant."""
        if not self.odometry_from_solve:
            return self.odometry_info
        if scan is not None and self.last_key_scan is not None and int(scan) > self.last_key_scan:
            handle, stream = self.odometry_source
            try:
                rec = handle.odometry_edges(stream, [self.last_key_scan], [int(scan)], **self.odometry_options)[0]
            except api.LiodomError:
                rec = None
            if rec is not None and int(rec["flags"]) == api.ODOM_EDGE_VALID:
                return np.array(rec["information"], np.float64).reshape(6, 6)
        self.odometry_fallbacks += 1
        return self.odometry_info

    def feed(self, pose, edges, scan=None):
        pose = _pose(pose)
        self.last_pose = pose
        if not self.policy.feed(pose):
            return dict(key_frame=False, node=None, loops=[])
        edges = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        node = self.graph.add_nodes(pose[None], [1 if not self.key_poses else 0])
        if self.key_poses:
            self.graph.add_edges(api.graph_edges([node - 1], [node], [between(self.key_poses[-1], pose)], self.odometry_information(scan), kind=0))
        self.last_key_scan = None if scan is None else int(scan)
        self.key_poses.append(pose)
        self.clouds.append(edges.copy())
        # lagged insertion: only key frames with min_gap newer ones behind them are places
        while self.inserted + self.min_gap <= node:
            self.places.add(self.clouds[self.inserted], self.key_poses[self.inserted], id=self.inserted)
            self.inserted += 1
        loops = []
        if self.inserted > 0 and edges.shape[0] > 0 and self.levels:
            seen = set()
            for m in self.places.query([edges], self.k)[0]:
                place = int(m["id"])
                if m["index"] < 0 or place in seen:
                    continue
                seen.add(place)
                found, results = api.Liodom._search_levels(self.map, edges, m["pose"], self.levels)
                fraction = (results[-1]["hits_r"] + results[-1]["hits_0"]) / (2.0 * edges.shape[0])
                if not fraction >= self.min_fraction:
                    continue
                if self.refine is None:
                    added, extra = self._add_gated(place, node, between(m["place_pose"], found), self.loop_info)
                    if added:
                        loops.append(dict(place=place, node=node, fraction=fraction, pose=np.array(found, np.float64), match=m, **extra))
                    continue
                Z, info, record = self.refine_loop(edges, m["place_pose"], found)
                if Z is None:
                    continue
                added, extra = self._add_gated(place, node, Z, info)
                if added:
                    loops.append(dict(place=place, node=node, fraction=fraction, pose=record["pose"].copy(), match=m,
                                      searched_pose=np.array(found, np.float64), registration=record, **extra))
        return dict(key_frame=True, node=node, loops=loops)

    def refine_loop(self, edges, place_pose, found):
        """Registers the searched pose `found` of the edge cloud `edges` to the map (Map.register_poses with refine's options) ->
        (Z, info, record): Z = between(place_pose, registered pose) and its information — loop_info, or with loop_info="solve"
        solve_information of the registration —, record = the registration's dict.  (None, None, record) if the registration did
        not end CONVERGED or MAX_PASSES, or with matches / n_edges below refine's min_fraction: no loop edge."""
        if self.refine is None:
            raise ValueError("LoopCloser.refine_loop: the LoopCloser was made without refine")
        edges = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1, 4)
        record = self.map.register_poses(edges, np.asarray(found, np.float64).reshape(1, 7), **self.refine)[0]
        taken = record["termination"] in (api.REG_CONVERGED, api.REG_MAX_PASSES)
        if not taken or edges.shape[0] == 0 or not record["matches"] / float(edges.shape[0]) >= self.refine_min_fraction:
            return None, None, record
        Z = between(place_pose, record["pose"])
        info = self.loop_info
        if self.info_from_solve and record["cov_flags"] == api.COV_VALID and record["sigma2"] > 0.0 and np.isfinite(record["information"]).all():
            info = solve_information(place_pose, record["pose"], Z, record["information"], record["sigma2"])
        return Z, info, record

    def _add_gated(self, place, node, Z, info):
        """Adds the loop edge (place, node, Z, info) unless the gate refuses it -> (added, dict(d2=...) with a gate, else {})."""
        edge = api.graph_edges([place], [node], [Z], info, kind=1)
        extra = {}
        if self.gate is not None:
            d2, status = self.graph.gate_edges(edge, **self.gate_options)
            if int(status[0]) != api.GRAPH_COV_OK or not float(d2[0]) <= self.gate:
                self.gated.append((place, node, float(d2[0]), api.GRAPH_COV_STATUSES[int(status[0])]))
                return False, extra
            extra = dict(d2=float(d2[0]))
        self.graph.add_edges(edge)
        self.loops.append((place, node))
        return True, extra

    def add_loop(self, place, node, Z, info=None):
        """A loop edge from another source — a surveyed tie, a user's hint, a test —: "X_place^-1 o X_node was measured as Z", the
        edge feed() would add (kind 1, info None: loop_info).  place and node are key frames' node indices, place < node.
        -> whether the edge was added: always True without a gate; with one, False where the gate refused it (it is then the
        last entry of self.gated)."""
        place, node = int(place), int(node)
        if not (0 <= place < node < len(self.key_poses)):
            raise ValueError("LoopCloser.add_loop: place and node must be key frames with place < node")
        info = self.loop_info if info is None else np.array(info, np.float64).reshape(6, 6)
        return self._add_gated(place, node, _pose(Z), info)[0]

    def _loop_edges(self):
        """Edge indices of the active loop edges: one per entry of self.loops, in its order."""
        ed, act = self.graph.edges(), self.graph.edge_active()
        idx = [e for e in range(ed.shape[0]) if int(ed["kind"][e]) == 1 and act[e]]
        if [(int(ed["i"][e]), int(ed["j"][e])) for e in idx] != [tuple(l) for l in self.loops]:
            raise ValueError("LoopCloser.close: the graph's loop edges are not the ones feed() and add_loop() added")
        return idx

    def close(self, handle=None, stream=0, reader_cells=None, loss=None, reject_below=None, **options):
        """Optimises the graph (the first key frame is fixed; **options: make_graph_options) and applies the result:
          map      reset and rebuilt from the key frames' clouds at the corrected poses; with reader_cells = (cells_xy, cells_z) the
                   handle's stream is detached from it before (attach_mapper(None)) and attached as its reader again after
          places   the poses of the database rewritten (export_state -> parse_place_state -> build_place_state -> import_state)
          stream   with a handle: seeded (seed_stream) at the corrected pose of the last scan fed — the last key frame's corrected
                   pose composed with the odometry since
        Returns dict(report, before [K, 7], after [K, 7], pose = the corrected current pose).

        loss = (name, scale): the solve runs with that robust loss (api.GRAPH_LOSSES) on the loop edges — kind 1; the odometry
        edges, kind 0, are never touched — and kind 1 is set back to "none" whatever happens.  The return gains robust_report (=
        report) and weights, the loop edges' weights in the order of self.loops.
        reject_below = r (needs loss): after the robust solve every loop edge with weight < r is switched off (it stays in the
        graph's edges, inactive), and the graph is optimised again from the robust result with the plain quadratic cost; that
        second result is what is applied, and `report` is its report.  The return gains rejected = [(place, node, weight)],
        kept = [(place, node, weight)] and applied = True; self.loops keeps the survivors, self.rejected accumulates.  If EVERY
        loop edge is rejected nothing is applied and nothing is switched off: the map, the places, the stream, self.loops and
        the graph — its poses are set back — stay as they were, and the return is dict(applied=False, rejected, kept=[],
        robust_report, report=None, before, after=before, pose=the last pose fed)."""
        if reject_below is not None and loss is None:
            raise ValueError("LoopCloser.close: reject_below needs a loss")
        if not self.key_poses:
            raise ValueError("LoopCloser.close: no key frame yet")
        before = np.stack(self.key_poses)
        st = api.parse_place_state(self.places.export_state()) if self.inserted else None
        if (st["count"] if st else self.places.count()) != self.inserted or (st and list(st["ids"]) != list(range(self.inserted))):
            raise ValueError("LoopCloser.close: the place database holds places that feed() did not add")
        extra = {}
        if loss is None:
            report = self.graph.optimize(**options)
        else:
            idx = self._loop_edges()
            start = self.graph.poses()
            self.graph.set_loss(1, loss[0], loss[1])
            try:
                report = self.graph.optimize(**options)
                weights = self.graph.edge_weights()[1][idx] if idx else np.zeros(0)
            finally:
                self.graph.set_loss(1, "none")
            extra = dict(robust_report=report, weights=weights)
            if reject_below is not None:
                both = [(l[0], l[1], float(w)) for l, w in zip(self.loops, weights)]
                rejected = [b for b in both if b[2] < reject_below]
                kept = [b for b in both if not b[2] < reject_below]
                if rejected and not kept:
                    self.graph.set_poses(0, start)
                    return dict(applied=False, rejected=rejected, kept=[], robust_report=report, weights=weights, report=None,
                                before=before, after=before.copy(), pose=self.last_pose.copy())
                for e, b in zip(idx, both):
                    if b[2] < reject_below:
                        self.graph.set_edge_active(e, [0])
                self.loops = [(b[0], b[1]) for b in kept]
                self.rejected += rejected
                report = self.graph.optimize(**options)
                extra.update(rejected=rejected, kept=kept, applied=True)
        after = self.graph.poses()
        current = compose(after[-1], between(before[-1], self.last_pose))
        if handle is not None and reader_cells is not None:
            handle.attach_mapper(None, stream=stream)
        self.map.reset()
        chunk = max(1, min(self.max_update_points, int(getattr(self.map, "max_update_points", self.max_update_points))))
        for cloud, pose in zip(self.clouds, after):
            T = api.pose_T34(pose)
            for at in range(0, cloud.shape[0], chunk):
                self.map.update(cloud[at:at + chunk], T)
        if handle is not None and reader_cells is not None:
            handle.attach_map_reader(self.map, reader_cells[0], reader_cells[1], stream=stream)
        if self.inserted:
            poses = np.stack([after[int(i)] for i in st["ids"]])
            self.places.import_state(api.build_place_state(st["geometry"], st["desc"], st["ids"], poses, st["bits"]))
        if handle is not None:
            handle.seed_stream(current, stream=stream)
            self.last_key_scan = None      # the stream's scan indices start over: the next key frame's interval would span two lives
        self.key_poses = [p.copy() for p in after]
        self.last_pose = current
        self.policy.last = [float(v) for v in after[-1]]
        return dict(report=report, before=before, after=after, pose=current, **extra)
