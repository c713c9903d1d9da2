// Relocalising over a wide window (liodom_map_search_pose_bnb / liodom_map_bound_nodes; no counterpart in the reference): upper
// bounds on the score of every candidate of a node, from block sets of the map's occupied leaves.  Included at the end of
// liodom_map.h, after kernels_reloc.h.
//
// The contract (include/liodom_hip.h; tests/reloc_bnb_model.py restates it in NumPy and the counts are held equal):
//   leaf        of a float coordinate p: floorf(p * leaf_inv) — map_leaf_bit's, a global integer lattice — "in range" iff it lies in
//               [-2^20, 2^20) (tested in float, before the cast)
//   block set   B_h, h = 1 .. 21: the keys (lx >> h, ly >> h, lz) of every finite point of every cell's current slab whose three
//               leaves are in range (arithmetic shift; blocks in x and y only).  An open-addressing table of 64-bit keys, 0 = empty.
//   node        T_lo: the matrix of its lowest child; t_hi: T[3], T[7] of its highest (the other entries are the same)
//   ranges      q_lo = transform_point(T_lo, e), q_hi likewise with t_hi.  Centre range of x: [leaf(q_lo.x), leaf(q_hi.x)]; radius 1:
//               [leaf(q_lo.x + (-1.f) * leaf), leaf(q_hi.x + 1.f * leaf)]; y likewise; z: the leaves of q.z + (j - 1) * leaf, j = 0, 1, 2
//   ub_r, ub_0  per edge 1 iff a key (bx, by, lz) is in B_h with bx, by in the (shifted) ranges and lz among the z leaves (ub_0: the
//               centre ranges and the centre's lz; radius 0: ub_r = ub_0)
//   escapes     an edge with a non-finite coordinate never counts (every probe of every child is non-finite).  A finite edge counts
//               in both sums without a lookup if a leaf it would use is not in range (this takes in non-finite extremes), or a range
//               spans more than three blocks, or the level's table has not been built.
// Every operation between a candidate's ix and a probe's leaf is monotone non-decreasing (the double add of the translation, the
// add of T[3], the rounding to float, the float add of d * leaf, the multiply by leaf_inv > 0, floorf), so the children's probes
// reach exactly the leaves between the two extremes': the bound is >= hits_r + hits_0 of every child (reloc_bit only removes hits).
// Nothing of the map is written.
#pragma once

#include "reloc_bnb.h"

namespace liodom_dev {

struct BlockTables {
  unsigned long long* base;      // table of level h: base + slot[h] * (mask + 1)
  unsigned int mask;             // entries of one table - 1 (a power of two >= 2 * the map's points)
  int slot[kRelocBnbLevelMax + 1];      // -1: not built
};

__device__ __forceinline__ bool bnb_leaf(float p, float leaf_inv, int* l) {
  const float f = floorf(p * leaf_inv);
  if (!(f >= -(float)kRelocBnbLeafLimit && f < (float)kRelocBnbLeafLimit)) return false;      // (false for NaN)
  *l = (int)f;
  return true;
}
__device__ __forceinline__ unsigned long long bnb_key(int bx, int by, int lz) {
  const int B = kRelocBnbLeafLimit;
  return (1ull << 63) | ((unsigned long long)(unsigned int)(bx + B) << 42) | ((unsigned long long)(unsigned int)(by + B) << 21) |
         (unsigned long long)(unsigned int)(lz + B);
}
__device__ __forceinline__ bool bnb_has(const unsigned long long* __restrict__ tab, unsigned int mask, unsigned long long key) {
  unsigned int h = map_hash(key, mask);
  for (unsigned int probe = 0; probe <= mask; probe++) {
    const unsigned long long k = tab[h];
    if (k == key) return true;
    if (k == 0ull) return false;
    h = (h + 1u) & mask;
  }
  return false;
}

// block sets, step 1: zeroes `total` 8-byte entries (a multiple of 2: tables are powers of two >= 64), 16 bytes per store
__global__ __launch_bounds__(256) void k_map_blocks_clear(unsigned long long* tab, size_t total) {
  const size_t n2 = total / 2, t = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  uint4* o4 = reinterpret_cast<uint4*>(tab);
  for (size_t i = t; i < n2; i += step) o4[i] = make_uint4(0u, 0u, 0u, 0u);
}

// block sets, step 2, grid (x, y) as k_map_occ_build: one insert (atomicCAS on the 64-bit key) per map point and built level
__global__ __launch_bounds__(256) void k_map_blocks_build(MapView m, BlockTables bt) {
  const int nc = max(0, min(m.st->n_cells, m.max_cells));
  for (int c = blockIdx.y; c < nc; c += gridDim.y) {
    const int cnt = max(0, min(m.cell_n[c], m.cell_cap));
    const float4* src = map_cell_cur(m, c);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
      const float4 p = src[i];
      if (!(ld_isfinite((double)p.x) && ld_isfinite((double)p.y) && ld_isfinite((double)p.z))) continue;
      int lx, ly, lz;
      if (!(bnb_leaf(p.x, m.leaf_inv, &lx) && bnb_leaf(p.y, m.leaf_inv, &ly) && bnb_leaf(p.z, m.leaf_inv, &lz))) continue;
      for (int h = 1; h <= kRelocBnbLevelMax; h++) {
        if (bt.slot[h] < 0) continue;
        unsigned long long* tab = bt.base + (size_t)bt.slot[h] * ((size_t)bt.mask + 1);
        const unsigned long long key = bnb_key(lx >> h, ly >> h, lz);
        unsigned int at = map_hash(key, bt.mask);
        for (unsigned int probe = 0; probe <= bt.mask; probe++) {      // (the table has a free entry for every point: this ends)
          unsigned long long prev = __hip_atomic_load(&tab[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (prev == 0ull) prev = atomicCAS(&tab[at], 0ull, key);
          if (prev == 0ull || prev == key) break;
          at = (at + 1u) & bt.mask;
        }
      }
    }
  }
}

// the leaf range of one axis over a node's children: [lo_r, hi_r] of the displaced probes, [lo_0, hi_0] of the centre
struct BnbRange { int lo_r, hi_r, lo_0, hi_0; bool ok; };
__device__ __forceinline__ BnbRange bnb_range(float q_lo, float q_hi, int radius, float leaf, float leaf_inv) {
  BnbRange r;
  r.lo_0 = r.hi_0 = 0;
  r.ok = bnb_leaf(q_lo, leaf_inv, &r.lo_0) && bnb_leaf(q_hi, leaf_inv, &r.hi_0);
  r.lo_r = r.lo_0; r.hi_r = r.hi_0;
  if (radius) r.ok = r.ok && bnb_leaf(q_lo + -1.0f * leaf, leaf_inv, &r.lo_r) && bnb_leaf(q_hi + 1.0f * leaf, leaf_inv, &r.hi_r);
  return r;
}

// One wave per node, lanes over the edges; a workgroup takes kRelocWaves contiguous nodes — the shape of k_map_score_poses.
//   node       wave-uniform (readfirstlane of the wave's number): its 12 + 2 doubles and its level are scalar loads
//   edges      read through the cache, one 16-byte load per lane and edge
//   lookups    at most 3 x 3 blocks for the centre, then 3 x 3 x 3 for the radius; an edge stops at its first hit
//   counts     ballot + popcount per round of 64 edges; lane 0 stores both with one 8-byte store.  No LDS, no atomics, no barrier.
// node_level: the level of each node, or null: every node at `level`.
__global__ __launch_bounds__(kRelocThreads) void k_map_bound_nodes(MapView m, BlockTables bt, const float4* __restrict__ edges, int n_edges,
                                                                   const double* __restrict__ T_lo, const double* __restrict__ t_hi,
                                                                   const int* __restrict__ node_level, int level, int n, int radius, float leaf,
                                                                   int* __restrict__ ub) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int node = (int)blockIdx.x * kRelocWaves + wave;
  if (node >= n) return;
  const double* Tp = T_lo + 12 * (size_t)node;
  double T[12], Th[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = Th[i] = Tp[i];
  Th[3] = t_hi[2 * (size_t)node]; Th[7] = t_hi[2 * (size_t)node + 1];
  const int h = node_level ? node_level[node] : level;
  const int slot = (h >= 1 && h <= kRelocBnbLevelMax) ? bt.slot[h] : -1;
  const unsigned long long* tab = bt.base + (size_t)max(slot, 0) * ((size_t)bt.mask + 1);
  int n_r = 0, n_0 = 0;
  for (int base = 0; base < n_edges; base += 64) {
    const int i = base + lane;
    bool h0 = false, hr = false;
    if (i < n_edges) {
      const float4 e = edges[i];
      if (ld_isfinite((double)e.x) && ld_isfinite((double)e.y) && ld_isfinite((double)e.z)) {
        float lx, ly, lz, hx, hy, hz;
        transform_point(T, e.x, e.y, e.z, &lx, &ly, &lz);
        transform_point(Th, e.x, e.y, e.z, &hx, &hy, &hz);
        const BnbRange rx = bnb_range(lx, hx, radius, leaf, m.leaf_inv), ry = bnb_range(ly, hy, radius, leaf, m.leaf_inv);
        int z[3] = {0, 0, 0};
        bool ok = slot >= 0 && rx.ok && ry.ok && bnb_leaf(lz, m.leaf_inv, &z[1]);
        if (radius) ok = ok && bnb_leaf(lz + -1.0f * leaf, m.leaf_inv, &z[0]) && bnb_leaf(lz + 1.0f * leaf, m.leaf_inv, &z[2]);
        // (valid leaves shifted by h >= 1 differ by less than 2^20: the subtractions cannot overflow)
        ok = ok && (rx.hi_r >> h) - (rx.lo_r >> h) <= 2 && (ry.hi_r >> h) - (ry.lo_r >> h) <= 2;
        if (!ok) {
          h0 = hr = true;
        } else {
          for (int by = ry.lo_0 >> h; by <= (ry.hi_0 >> h) && !h0; by++)
            for (int bx = rx.lo_0 >> h; bx <= (rx.hi_0 >> h) && !h0; bx++) h0 = bnb_has(tab, bt.mask, bnb_key(bx, by, z[1]));
          hr = h0;
          if (radius && !hr) {
            for (int j = 0; j < 3 && !hr; j++)
              for (int by = ry.lo_r >> h; by <= (ry.hi_r >> h) && !hr; by++)
                for (int bx = rx.lo_r >> h; bx <= (rx.hi_r >> h) && !hr; bx++) hr = bnb_has(tab, bt.mask, bnb_key(bx, by, z[j]));
          }
        }
      }
    }
    n_r += __popcll(__ballot(hr));
    n_0 += __popcll(__ballot(h0));
  }
  if (lane == 0) reinterpret_cast<int2*>(ub)[node] = make_int2(n_r, n_0);
}

}  // namespace liodom_dev
