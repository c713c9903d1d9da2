"""A pure-Python model of liodom_map_evict and liodom_map_merge_state on parsed blobs (api.parse_map_state), and a fake Map built
on it for running liodom_amd.pager.MapPager without a device.  Independent of the kernels: the GPU tests compare against it.

A model state is a dict with keys (list of (kx, ky, kz) tuples), corner_leaf (list of 3-tuples), cells (list of [n, 4] float32
arrays) and status, all in creation order."""
import numpy as np

from liodom_amd import api


def state_of(blob, sizes=None):
    st = api.parse_map_state(blob, sizes=sizes)
    return dict(keys=[tuple(int(q) for q in k) for k in st["keys"]], corner_leaf=[tuple(int(q) for q in c) for c in st["corner_leaf"]],
                cells=[c.copy() for c in st["cells"]], status=int(st["status"]))


def blob_of(state, sizes, status=None):
    xy, z, res = sizes
    return api.join_map_state(xy, z, res, state["keys"], state["corner_leaf"], state["cells"], status=state["status"] if status is None else status)


def empty_state():
    return dict(keys=[], corner_leaf=[], cells=[], status=0)


def centre_cell(T34, sizes):
    """Map::getLocalMap's centre (map.cc:144-151): the translation truncated to int first, then the cell key."""
    T = np.asarray(T34, np.float64).reshape(3, 4)
    return api.map_cell_key([float(int(T[0, 3])), float(int(T[1, 3])), float(int(T[2, 3]))], sizes[0], sizes[1])


def keeps(key, centre, sizes, keep_xy, keep_z):
    """The keep rule of liodom_map_prune: a plain box in double."""
    lim = (keep_xy * sizes[0], keep_xy * sizes[0], keep_z * sizes[1])
    return all(abs(float(key[a]) - float(centre[a])) <= lim[a] for a in range(3))


def _pick(state, idx, status):
    return dict(keys=[state["keys"][i] for i in idx], corner_leaf=[state["corner_leaf"][i] for i in idx],
                cells=[state["cells"][i] for i in idx], status=status)


def evict(state, T34, sizes, keep_xy, keep_z):
    """-> (kept, removed): both in relative creation order; the kept part has the map's status, the removed tile status 0."""
    c = centre_cell(T34, sizes)
    flags = [keeps(k, c, sizes, keep_xy, keep_z) for k in state["keys"]]
    kept = _pick(state, [i for i, f in enumerate(flags) if f], state["status"])
    removed = _pick(state, [i for i, f in enumerate(flags) if not f], 0)
    return kept, removed


def merge(state, tile, max_cells=None):
    """-> (merged, taken): the tile's cells whose key the state lacks, appended in tile order; status ORed.  None, taken when the
    taken cells do not fit max_cells (the map stays untouched)."""
    have = set(state["keys"])
    taken = np.array([0 if k in have else 1 for k in tile["keys"]], np.int32)
    idx = [i for i, t in enumerate(taken) if t]
    if max_cells is not None and len(state["keys"]) + len(idx) > max_cells:
        return None, taken
    if not tile["keys"]:
        return state, taken
    add = _pick(tile, idx, 0)
    return dict(keys=state["keys"] + add["keys"], corner_leaf=state["corner_leaf"] + add["corner_leaf"], cells=state["cells"] + add["cells"],
                status=state["status"] | tile["status"]), taken


def by_key(state):
    """{key: (corner_leaf, bytes of the points)}: two maps hold the same cells iff these are equal, whatever the ids."""
    return {k: (c, p.tobytes()) for k, c, p in zip(state["keys"], state["corner_leaf"], state["cells"])}


class FakeMap:
    """What MapPager needs of liodom_amd.Map, on the model.  update() appends the transformed points to their cells without any
    voxel filter (new cells in first-appearance order): enough for the pager's bookkeeping, not a model of Map::updateMap."""

    def __init__(self, xy, z, res, max_cells=1 << 20, max_update_points=64):
        self.sizes = (float(xy), float(z), float(res))
        self.max_cells, self.max_update_points = max_cells, max_update_points
        self.state = empty_state()
        self.calls = []

    def num_cells(self):
        return len(self.state["keys"])

    def export_state(self):
        return blob_of(self.state, self.sizes)

    def import_state(self, blob):
        self.state = state_of(blob, self.sizes)

    def evict(self, T34, keep_xy, keep_z):
        self.state, removed = evict(self.state, T34, self.sizes, keep_xy, keep_z)
        self.calls.append(("evict", len(removed["keys"])))
        return blob_of(removed, self.sizes), len(removed["keys"])

    def merge_state(self, blob):
        merged, taken = merge(self.state, state_of(blob, self.sizes), self.max_cells)
        if merged is None:
            raise RuntimeError("FakeMap: not enough free cells")
        self.state = merged
        self.calls.append(("merge", int(taken.sum()), len(taken)))
        return taken

    def update(self, xyzi, T34=None):
        x = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        assert x.shape[0] <= self.max_update_points
        T = np.eye(4)[:3] if T34 is None else np.asarray(T34, np.float64).reshape(3, 4)
        p = x.copy()
        p[:, :3] = (x[:, :3].astype(np.float64) @ T[:, :3].T + T[:, 3]).astype(np.float32)
        xy, z, res = self.sizes
        self.calls.append(("update", x.shape[0]))
        for q in p:
            key = tuple(api.map_cell_key(q[:3], xy, z))
            if key not in self.state["keys"]:
                self.state["keys"].append(key)
                self.state["corner_leaf"].append(tuple(api.map_cell_corner_leaf(q[:3], xy, z, res)))
                self.state["cells"].append(np.zeros((0, 4), np.float32))
            i = self.state["keys"].index(key)
            self.state["cells"][i] = np.concatenate([self.state["cells"][i], q[None]])
