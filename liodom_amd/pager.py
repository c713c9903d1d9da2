"""MapPager: the device map (liodom_amd.Map) as a window onto a larger map that lives on the host.

Between scans the pager evicts the cells outside a keep box around the pose (Map.evict: they come out as a blob, nothing is
lost), keeps them in `store`, and puts the stored cells inside a load box around the same pose back (Map.merge_state).  Device
memory stays bounded by the keep box, a revisit sees exactly the cells it left, and export_all() is the whole map.
No library, no GPU of its own: everything goes through the Map handed in.
"""
import numpy as np

from . import api


def identity_pose():
    return np.ascontiguousarray(np.eye(4)[:3], np.float64)


class MapPager:
    """MapPager(map, keep_xy, keep_z, load_xy, load_z): step(T34) after a scan (or every n-th scan) with that scan's pose.

    store: dict from cell key (kx, ky, kz) to (corner_leaf, points), in the order the cells were evicted.
    Counters: evicted, loaded (cells, over the pager's life) and conflicts.  last_evicted / last_loaded: the keys of the last step.

    A CONFLICT is a stored cell whose key is a cell of the device map as well: a merge that reports taken = 0, or an evicted key
    that is in the store already.  The device created that cell anew because the stored one was not there when the sensor touched
    it.  Both are resolved by one rule: the device keeps (for an evicted key: gets back) its cell, the stored cell's points go
    through Map.update(points, identity) in chunks of max_update_points — the map treats them as re-observed points — and the
    stored cell is dropped.  The result is a sound map, but not the map of an unbounded run (the voxel filter saw the points in
    another order).

    No conflict happens, and a paged run equals the unbounded run bit for bit, while the device holds everything the sensor can
    touch before it touches it:
      load_xy * voxel_xysize >= max_range + (window travel of the lagged frame) + (travel per pager period + 1 m for the int
                                truncation of the centre) + voxel_xysize,
      the same on z — for getLocalMap's z column with the reference's quirk that its extent comes from the xy size:
                                load_z * voxel_zsize >= cells_z * voxel_xysize as well —,
      load_xy >= cells_xy + 1,
    and keep >= load on both axes (checked: ValueError).  keep > load gives hysteresis: a cell loaded at the rim of the load box
    is not evicted by the next small step back.  max_cells of the map must hold the keep box plus the cells one period creates.
    """

    def __init__(self, map, keep_xy, keep_z, load_xy, load_z):
        if min(keep_xy, keep_z, load_xy, load_z) < 0 or keep_xy < load_xy or keep_z < load_z:
            raise ValueError("MapPager: needs keep >= load >= 0 on both axes (keep %r, %r; load %r, %r)" % (keep_xy, keep_z, load_xy, load_z))
        self.map = map
        self.keep_xy, self.keep_z, self.load_xy, self.load_z = int(keep_xy), int(keep_z), int(load_xy), int(load_z)
        self.store = {}
        self.evicted = self.loaded = self.conflicts = 0
        self.last_evicted, self.last_loaded = [], []

    def centre(self, T34):
        """The centre cell of a pose as liodom_map_prune / Map::getLocalMap compute it: the translation truncated to int first."""
        T = np.asarray(T34, np.float64).reshape(3, 4)
        xy, z, _ = self.map.sizes
        return api.map_cell_key([float(int(T[0, 3])), float(int(T[1, 3])), float(int(T[2, 3]))], xy, z)

    def in_box(self, key, centre, n_xy, n_z):
        """The keep rule of liodom_map_prune, compared in double."""
        xy, z, _ = self.map.sizes
        lim = (n_xy * xy, n_xy * xy, n_z * z)
        return all(abs(float(key[a]) - float(centre[a])) <= lim[a] for a in range(3))

    def _reobserve(self, points):
        cap = int(self.map.max_update_points)
        for lo in range(0, len(points), cap):
            self.map.update(points[lo:lo + cap], identity_pose())

    def _blob(self, keys, status=0):
        xy, z, res = self.map.sizes
        return api.join_map_state(xy, z, res, np.array(keys, np.int64).reshape(-1, 3), np.array([self.store[k][0] for k in keys], np.int64).reshape(-1, 3),
                                  [self.store[k][1] for k in keys], status=status)

    def store_state(self, blob):
        """Puts the cells of a saved map (a blob of this map's sizes, e.g. a site map larger than the device map) into the store;
        the device is not touched, the next step loads what its load box holds.  ValueError for a key that is stored already."""
        st = api.parse_map_state(blob, sizes=self.map.sizes)
        keys = [tuple(int(q) for q in k) for k in st["keys"]]
        if any(k in self.store for k in keys):
            raise ValueError("MapPager.store_state: a cell of the blob is in the store already")
        for key, corner, pts in zip(keys, st["corner_leaf"], st["cells"]):
            self.store[key] = (corner.copy(), pts.copy())

    def step(self, T34):
        """Evict outside the keep box, store; load the stored cells inside the load box.  Returns (evicted, loaded) of this step."""
        xy, z, res = self.map.sizes
        blob, n = self.map.evict(T34, self.keep_xy, self.keep_z)
        st = api.parse_map_state(blob, sizes=self.map.sizes)
        assert len(st["keys"]) == n
        self.last_evicted, self.last_loaded = [], []
        back = []                              # evicted cells whose key is in the store already
        for k, corner, pts in zip(st["keys"], st["corner_leaf"], st["cells"]):
            key = tuple(int(q) for q in k)
            self.last_evicted.append(key)
            if key in self.store:
                back.append((key, corner.copy(), pts.copy()))
            else:
                self.store[key] = (corner.copy(), pts.copy())
        self.evicted += n
        if back:                               # the device gets its cell back, the stored one is re-observed into it
            taken = self.map.merge_state(api.join_map_state(xy, z, res, [b[0] for b in back], [b[1] for b in back], [b[2] for b in back]))
            assert taken.all()
            for key, _, _ in back:
                self.conflicts += 1
                self._reobserve(self.store.pop(key)[1])
        centre = self.centre(T34)
        want = [k for k in self.store if self.in_box(k, centre, self.load_xy, self.load_z)]
        if want:
            taken = self.map.merge_state(self._blob(want))
            for k, t in zip(want, taken):
                pts = self.store.pop(k)[1]
                if t:
                    self.loaded += 1
                    self.last_loaded.append(k)
                else:
                    self.conflicts += 1
                    self._reobserve(pts)
        return n, len(self.last_loaded)

    def export_all(self):
        """The blob of device map U store: the device's cells first (creation order), then the stored ones (eviction order)."""
        xy, z, res = self.map.sizes
        st = api.parse_map_state(self.map.export_state(), sizes=self.map.sizes)
        keys = [tuple(int(q) for q in k) for k in st["keys"]] + list(self.store)
        corner = [c for c in st["corner_leaf"]] + [self.store[k][0] for k in self.store]
        cells = list(st["cells"]) + [self.store[k][1] for k in self.store]
        return api.join_map_state(xy, z, res, keys, corner, cells, status=st["status"])
