// reloc_bnb.h — branch-and-bound over the candidate grid of liodom_map_search_pose_bnb (include/liodom_hip.h): the
// level of a node, a node's two extreme children, and the round-based driver, with the scoring behind two callbacks.
// Plain C++, no HIP include: tests/reloc_bnb_main.cc compiles it for the host alone under sanitizers; tests/reloc_bnb_model.py
// restates it in NumPy and the counts are held equal.
//
// A node is a tile of one (ia, iz) slab of the grid (reloc_candidates.h): the candidates x0 .. x0 + 2^k - 1 by y0 .. y0 + 2^k - 1
// (x = ix + nx, y = iy + ny), clipped to the grid.  Its bound is computed from its two extreme children — (x0, y0) and the clipped
// (x1, y1) — at the block level reloc_bnb_level gives for the unclipped width 2^k.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "reloc_candidates.h"

namespace liodom_dev {

constexpr int64_t kRelocBnbCandidatesMax = 0x7fffffff;      // per axis and in all: best_index and n_candidates are int32
constexpr int kRelocBnbLevelMax = 21;      // blocks of 2^21 leaves: the leaf coordinates of a table, +-2^20, fall into two of them
constexpr int kRelocBnbLeafLimit = 1 << 20;      // leaf coordinates in [-2^20, 2^20) have a place in a block key, others are escapes
constexpr int kRelocBnbBatchDefault = 1024;
constexpr int kRelocBnbBatchMax = 65536;

// The block level of a node `width` candidates wide: the smallest h >= 1 with 2^h >= (width - 1) * step / leaf + 2 radius + 2.
// The probes of the node's children span (width - 1) * step / leaf + 2 radius leaves on an axis, plus a leaf for the floor at
// either end; a run of at most 2^h + 1 leaves touches at most two blocks of 2^h, so a range has a block to spare of the three the
// bound looks up per axis (and one that needs more is an escape: the bound never depends on this choice for being admissible).
inline int reloc_bnb_level(int64_t width, double step_xy, double resolution, int radius) {
  const double leaf = (double)(float)resolution;
  const double span = (width > 1 ? (double)(width - 1) * step_xy / leaf : 0.0) + 2.0 * radius + 2.0;
  int h = 1;
  while (h < kRelocBnbLevelMax && ldexp(1.0, h) < span) h++;
  return h;
}

struct RelocBnbGrid {
  int64_t wx, wy, slabs;      // candidates in x and y, (ia, iz) pairs: slab = (iz + nz) * (2 nyaw + 1) + (ia + nyaw)
  int K;                      // a root is 2^K wide: the smallest K with 2^K >= max(wx, wy)
};
inline RelocBnbGrid reloc_bnb_grid(const liodom_pose_search_t* s) {
  RelocBnbGrid g;
  g.wx = 2 * (int64_t)s->nx + 1; g.wy = 2 * (int64_t)s->ny + 1;
  g.slabs = (2 * (int64_t)s->nyaw + 1) * (2 * (int64_t)s->nz + 1);
  g.K = 0;
  while (((int64_t)1 << g.K) < std::max(g.wx, g.wy)) g.K++;
  return g;
}

struct RelocBnbNode {
  int64_t slab;
  int32_t x0, y0, k, bound;
};
inline int64_t reloc_bnb_lowest(const RelocBnbGrid& g, const RelocBnbNode& n) { return (n.slab * g.wy + n.y0) * g.wx + n.x0; }
inline int64_t reloc_bnb_highest(const RelocBnbGrid& g, const RelocBnbNode& n) {
  const int64_t x1 = std::min<int64_t>((int64_t)n.x0 + ((int64_t)1 << n.k), g.wx) - 1, y1 = std::min<int64_t>((int64_t)n.y0 + ((int64_t)1 << n.k), g.wy) - 1;
  return (n.slab * g.wy + y1) * g.wx + x1;
}

// The two extreme children of a node as k_map_bound_nodes takes them: T_lo = the matrix of (x0, y0), t_hi = T[3], T[7] of (x1, y1).
inline void reloc_bnb_extremes(const liodom_pose_search_t* s, const RelocCentre& c, const RelocBnbGrid& g, const RelocBnbNode& n, double* T_lo, double* t_hi) {
  double t[3];
  int ix, iy, ia, iz;
  reloc_candidate_matrix(s, c, reloc_bnb_lowest(g, n), T_lo);
  reloc_candidate_indices(s, reloc_bnb_highest(g, n), &ix, &iy, &ia, &iz);
  reloc_candidate_translation(s, c, ix, iy, iz, t);
  t_hi[0] = t[0]; t_hi[1] = t[1];
}

struct RelocBnbResult {
  int64_t best_index;
  int32_t hits_r, hits_0;
  int64_t rounds, nodes_bounded, candidates_scored;
};

// The search.  max_score: no candidate scores more (2 * n_edges) — the bound of a root, which is never bounded itself.
//   bound_fn(const RelocBnbNode* nodes, size_t n, int32_t* ub)      ub[2 i], ub[2 i + 1] = ub_r, ub_0 of node i; returns 0 or an error
//   exact_fn(const int64_t* index, size_t n, int32_t* hits)         hits[2 i], hits[2 i + 1] = hits_r, hits_0 of candidate index[i]
// Order: a node comes before another if its bound is larger, or equal and its lowest candidate index lower (open nodes are disjoint
// tiles: the order is total).  A node cannot win if its bound is below the incumbent's score, or equal with its lowest index above
// the incumbent's.  Each round drops those, takes the first `batch` of the rest, scores the width-1 nodes among them exactly and
// bounds the children (up to four, clipped to the grid) of the others; a child's bound is min(its own, its parent's).  The roots
// are not materialised (there may be 2^31 of them): they all have the bound max_score and come in slab order, so a counter stands
// for the ones not taken yet.  Ends when nothing is left; the incumbent is then the exhaustive ranking's best: the largest score,
// ties to the lowest index.  Returns 0, or the first error of a callback.
template <class BoundFn, class ExactFn>
inline int reloc_bnb_search(const RelocBnbGrid& g, int32_t max_score, int batch, BoundFn&& bound_fn, ExactFn&& exact_fn, RelocBnbResult* res) {
  std::vector<RelocBnbNode> open, take, kids;
  std::vector<int64_t> leaves;
  std::vector<int32_t> vals;
  int64_t next_root = 0, best_index = -1;
  int32_t best_score = -1;
  *res = RelocBnbResult{0, 0, 0, 0, 0, 0};
  const size_t nb = (size_t)std::max(1, batch);
  auto hopeless = [&](int32_t bound, int64_t lowest) { return best_index >= 0 && (bound < best_score || (bound == best_score && lowest > best_index)); };
  auto before = [&](const RelocBnbNode& a, const RelocBnbNode& b) { return a.bound != b.bound ? a.bound > b.bound : reloc_bnb_lowest(g, a) < reloc_bnb_lowest(g, b); };
  for (;;) {
    open.erase(std::remove_if(open.begin(), open.end(), [&](const RelocBnbNode& n) { return hopeless(n.bound, reloc_bnb_lowest(g, n)); }), open.end());
    // (every candidate scored so far lies in a root taken already: the roots left all have a lowest index above the incumbent's)
    if (next_root < g.slabs && hopeless(max_score, next_root * g.wy * g.wx)) next_root = g.slabs;
    if (open.empty() && next_root >= g.slabs) break;
    res->rounds++;
    const size_t n_open = std::min(nb, open.size());
    std::partial_sort(open.begin(), open.begin() + (std::ptrdiff_t)n_open, open.end(), before);
    take.clear();
    size_t io = 0;
    while (take.size() < nb) {
      const bool has_open = io < n_open, has_root = next_root < g.slabs;
      if (!has_open && !has_root) break;
      const RelocBnbNode root{next_root, 0, 0, g.K, max_score};
      if (has_open && (!has_root || before(open[io], root))) take.push_back(open[io++]);
      else { take.push_back(root); next_root++; }
    }
    open.erase(open.begin(), open.begin() + (std::ptrdiff_t)io);
    kids.clear(); leaves.clear();
    for (const RelocBnbNode& n : take) {
      if (n.k == 0) { leaves.push_back(reloc_bnb_lowest(g, n)); continue; }
      const int64_t half = (int64_t)1 << (n.k - 1);
      for (int q = 0; q < 4; q++) {
        const int64_t x = n.x0 + (q & 1) * half, y = n.y0 + (q >> 1) * half;
        if (x < g.wx && y < g.wy) kids.push_back(RelocBnbNode{n.slab, (int32_t)x, (int32_t)y, n.k - 1, n.bound});
      }
    }
    if (!kids.empty()) {
      vals.assign(2 * kids.size(), 0);
      const int rc = bound_fn((const RelocBnbNode*)kids.data(), kids.size(), vals.data());
      if (rc) return rc;
      res->nodes_bounded += (int64_t)kids.size();
      for (size_t i = 0; i < kids.size(); i++) kids[i].bound = std::min(kids[i].bound, vals[2 * i] + vals[2 * i + 1]);
      open.insert(open.end(), kids.begin(), kids.end());
    }
    if (!leaves.empty()) {
      vals.assign(2 * leaves.size(), 0);
      const int rc = exact_fn((const int64_t*)leaves.data(), leaves.size(), vals.data());
      if (rc) return rc;
      res->candidates_scored += (int64_t)leaves.size();
      for (size_t i = 0; i < leaves.size(); i++) {
        const int32_t score = vals[2 * i] + vals[2 * i + 1];
        if (score > best_score || (score == best_score && leaves[i] < best_index)) {
          best_score = score; best_index = leaves[i];
          res->hits_r = vals[2 * i]; res->hits_0 = vals[2 * i + 1];
        }
      }
    }
  }
  res->best_index = best_index < 0 ? 0 : best_index;
  return 0;
}

}  // namespace liodom_dev
