"""NumPy restatement of branch-and-bound relocalisation (include/liodom_hip.h "relocalising over a wide window",
csrc/kernels_reloc_bnb.h, csrc/reloc_bnb.h): the block sets, the bound of a node, the level of a node and the round-based driver.
The exact score and the candidate grid come from tests/reloc_model.py, unchanged.  Nothing here touches the library's compute entry
points.

  leaf        floor(p * leaf_inv) in float32; in range iff in [-2^20, 2^20)
  block set   B_h = {(lx >> h, ly >> h, lz)} over the finite points of every cell whose three leaves are in range
  node        T_lo [12] the lowest child's matrix, t_hi [2] = T[3], T[7] of the highest child
  ub_0, ub_r  per edge, see BlockSets.bound; an edge with a non-finite coordinate counts in neither, a finite edge with a leaf out of
              range or a range over more than three blocks counts in both
  driver      search(): rounds of `batch` nodes, ordered by (bound descending, lowest candidate index ascending)"""
import numpy as np

import reloc_model as rm

LEVEL_MAX = 21
LEAF_LIMIT = 1 << 20
BATCH_DEFAULT = 1024


def level_of(width, step_xy, resolution, radius):
    """reloc_bnb_level: the smallest h >= 1 with 2^h >= (width - 1) * step / leaf + 2 radius + 2, at most LEVEL_MAX."""
    leaf = float(np.float32(resolution))
    span = (float(width - 1) * step_xy / leaf if width > 1 else 0.0) + 2.0 * radius + 2.0
    h = 1
    while h < LEVEL_MAX and 2.0 ** h < span:
        h += 1
    return h


def _leaf(p32, leaf_inv):
    """(leaf as int64, in range) of float32 coordinates."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(p32, np.float32) * leaf_inv)
        ok = (f >= -LEAF_LIMIT) & (f < LEAF_LIMIT)
    return np.where(ok, f, np.float32(0)).astype(np.int64), ok


def _pack(bx, by, lz):
    return ((bx + LEAF_LIMIT) << 42) | ((by + LEAF_LIMIT) << 21) | (lz + LEAF_LIMIT)


class BlockSets:
    def __init__(self, state):
        self.leaf = np.float32(state["resolution"])
        self.leaf_inv = np.float32(1.0) / np.float32(state["resolution"])
        pts = [np.asarray(c, np.float32).reshape(-1, 4)[:, :3] for c in state["cells"]]
        p = np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)
        p = p[np.isfinite(p).all(axis=1)]
        leaves, ok = _leaf(p, self.leaf_inv)
        self.leaves = leaves[ok.all(axis=1)]
        self._sets = {}

    def keys(self, h):
        if h not in self._sets:
            l = self.leaves
            self._sets[h] = np.unique(_pack(l[:, 0] >> h, l[:, 1] >> h, l[:, 2]))
        return self._sets[h]

    def _has(self, h, key, where):
        s = self.keys(h)
        if s.size == 0:
            return np.zeros(key.shape, bool)
        at = np.minimum(np.searchsorted(s, key), s.size - 1)
        return where & (s[at] == key)

    def _range(self, q_lo, q_hi, radius):
        lo_0, a = _leaf(q_lo, self.leaf_inv)
        hi_0, b = _leaf(q_hi, self.leaf_inv)
        ok = a & b
        lo_r, hi_r = lo_0, hi_0
        if radius:
            with np.errstate(invalid="ignore", over="ignore"):
                lo_r, a = _leaf(q_lo + np.float32(-1.0) * self.leaf, self.leaf_inv)
                hi_r, b = _leaf(q_hi + np.float32(1.0) * self.leaf, self.leaf_inv)
            ok = ok & a & b
        return lo_r, hi_r, lo_0, hi_0, ok

    def bound(self, edges, T_lo, t_hi, level, radius=1):
        """int32 [n, 2] (sum of ub_r, sum of ub_0) of the nodes T_lo [n, 12], t_hi [n, 2] at block level `level` (an int, or one per node)."""
        e32 = np.asarray(edges, np.float32).reshape(-1, 4)[:, :3]
        e = e32.astype(np.float64)
        T = np.asarray(T_lo, np.float64).reshape(-1, 12)
        th = np.asarray(t_hi, np.float64).reshape(-1, 2)
        n = T.shape[0]
        out = np.zeros((n, 2), np.int32)
        if n == 0 or e.shape[0] == 0:
            return out
        h = np.broadcast_to(np.asarray(level, np.int64).reshape(-1, 1), (n, 1))
        fin = np.isfinite(e32).all(axis=1)[None, :]
        Tc = T[:, :, None]

        def q(r, t3):
            with np.errstate(invalid="ignore", over="ignore"):
                return (Tc[:, 4 * r + 0] * e[:, 0] + Tc[:, 4 * r + 1] * e[:, 1] + Tc[:, 4 * r + 2] * e[:, 2] + t3).astype(np.float32)

        x = self._range(q(0, Tc[:, 3]), q(0, th[:, 0:1]), radius)
        y = self._range(q(1, Tc[:, 7]), q(1, th[:, 1:2]), radius)
        qz = q(2, Tc[:, 11])
        with np.errstate(invalid="ignore", over="ignore"):
            z = [_leaf(qz + np.float32(j - 1) * self.leaf, self.leaf_inv) for j in range(3)]
        ok = x[4] & y[4] & z[1][1]
        if radius:
            ok = ok & z[0][1] & z[2][1]
        ok = ok & ((x[1] >> h) - (x[0] >> h) <= 2) & ((y[1] >> h) - (y[0] >> h) <= 2)

        def any_block(xlo, xhi, ylo, yhi, lz):
            hit = np.zeros(ok.shape, bool)
            for dy in range(3):
                for dx in range(3):
                    bx, by = (xlo >> h) + dx, (ylo >> h) + dy
                    hit |= self._level_has(h, _pack(bx, by, lz), ok & (bx <= (xhi >> h)) & (by <= (yhi >> h)))
            return hit

        h0 = any_block(x[2], x[3], y[2], y[3], z[1][0])
        hr = h0.copy()
        if radius:
            for j in range(3):
                hr |= any_block(x[0], x[1], y[0], y[1], z[j][0])
        esc = fin & ~ok
        out[:, 0] = (fin & (hr | esc)).sum(axis=1)
        out[:, 1] = (fin & (h0 | esc)).sum(axis=1)
        return out

    def _level_has(self, h, key, where):
        hit = np.zeros(key.shape, bool)
        for lv in np.unique(h):
            rows = (h[:, 0] == lv)
            if 1 <= lv <= LEVEL_MAX:
                hit[rows] = self._has(int(lv), key[rows], where[rows])
        return hit


# ---- the driver (reloc_bnb_search) ----
def search(wx, wy, slabs, max_score, batch, bound_fn, exact_fn):
    """bound_fn(nodes) -> [n, 2] for nodes = [(slab, x0, y0, k)]; exact_fn(indices) -> [n, 2].  -> dict(best_index, hits_r, hits_0,
    rounds, nodes_bounded, candidates_scored)."""
    K = 0
    while (1 << K) < max(wx, wy):
        K += 1
    lowest = lambda n: (n[0] * wy + n[2]) * wx + n[1]
    open_ = [(s, 0, 0, K, max_score) for s in range(slabs)]
    best_index, best_score, best = -1, -1, (0, 0)
    st = dict(rounds=0, nodes_bounded=0, candidates_scored=0)
    while True:
        open_ = [n for n in open_ if not (best_index >= 0 and (n[4] < best_score or (n[4] == best_score and lowest(n) > best_index)))]
        if not open_:
            break
        st["rounds"] += 1
        open_.sort(key=lambda n: (-n[4], lowest(n)))
        take, open_ = open_[:batch], open_[batch:]
        kids, leaves = [], []
        for s, x0, y0, k, b in take:
            if k == 0:
                leaves.append(lowest((s, x0, y0)))
                continue
            half = 1 << (k - 1)
            for q in range(4):
                x, y = x0 + (q & 1) * half, y0 + (q >> 1) * half
                if x < wx and y < wy:
                    kids.append((s, x, y, k - 1, b))
        if kids:
            ub = np.asarray(bound_fn([n[:4] for n in kids]), np.int64).reshape(-1, 2)
            st["nodes_bounded"] += len(kids)
            open_ += [n[:4] + (min(n[4], int(u[0] + u[1])),) for n, u in zip(kids, ub)]
        if leaves:
            hits = np.asarray(exact_fn(leaves), np.int64).reshape(-1, 2)
            st["candidates_scored"] += len(leaves)
            for i, hh in zip(leaves, hits):
                score = int(hh[0] + hh[1])
                if score > best_score or (score == best_score and i < best_index):
                    best_score, best_index, best = score, i, (int(hh[0]), int(hh[1]))
    return dict(best_index=max(best_index, 0), hits_r=best[0], hits_0=best[1], **st)


def node_extremes(T_all, wx, wy, nodes):
    """(T_lo [n, 12], t_hi [n, 2], lowest [n], highest [n]) of nodes (slab, x0, y0, k) of a grid whose matrices are T_all [n, 12]."""
    lo = np.array([(s * wy + y0) * wx + x0 for s, x0, y0, k in nodes], np.int64)
    hi = np.array([(s * wy + min(y0 + (1 << k), wy) - 1) * wx + min(x0 + (1 << k), wx) - 1 for s, x0, y0, k in nodes], np.int64)
    return T_all[lo], T_all[hi][:, [3, 7]], lo, hi


def search_grid(occ, blocks, edges, centre, batch=BATCH_DEFAULT, resolution=0.4, **grid):
    """The model of liodom_map_search_pose_bnb on a grid small enough to tabulate its matrices: search()'s dict plus n_candidates and
    levels_built.  occ: rm.Occupancy, blocks: BlockSets of the same state."""
    T_all, _, _ = rm.candidate_grid(centre, **grid)
    radius = grid.get("radius", 1)
    wx, wy = 2 * grid.get("nx", 0) + 1, 2 * grid.get("ny", 0) + 1
    slabs = T_all.shape[0] // (wx * wy)
    n_edges = np.asarray(edges).reshape(-1, 4).shape[0]
    level = lambda k: level_of(1 << k, grid.get("step_xy", 0.4), resolution, radius)

    def bound_fn(nodes):
        T_lo, t_hi, _, _ = node_extremes(T_all, wx, wy, nodes)
        return blocks.bound(edges, T_lo, t_hi, [level(n[3]) for n in nodes], radius)

    if n_edges == 0 or blocks.leaves.shape[0] == 0:
        r = dict(best_index=0, hits_r=0, hits_0=0, rounds=0, nodes_bounded=0, candidates_scored=0, levels_built=0)
    else:
        r = search(wx, wy, slabs, 2 * n_edges, batch, bound_fn, lambda idx: occ.hits(edges, T_all[np.asarray(idx)], radius=radius))
        K = 0
        while (1 << K) < max(wx, wy):
            K += 1
        r["levels_built"] = len({level(k) for k in range(K)})
    r["n_candidates"] = T_all.shape[0]
    return r
