// Relocalising in a saved map (liodom_map_score_poses / liodom_map_search_pose; no counterpart in the reference): candidate poses
// of one scan's edge cloud scored against the map's leaf occupancy.  Included at the end of liodom_map.h.
//
// The contract (include/liodom_hip.h; tests/reloc_model.py restates it in NumPy and the counts are held equal):
//   occupancy  bit map_leaf_bit(m, c, p) of row c for every finite point p of cell c's current slab, if it is >= 0
//   query      q = transform_point(T, e) (FP64 multiply-adds, rounded to float: what k_map_assign does to an inserted point)
//   probe p    hits iff p is finite, its three map_cell_key pack, map_find_cell finds their cell, and p's leaf bit there is set
//   probes     the centre q; radius = 1: q + d * leaf, d in {-1, 0, 1}^3, leaf = (float)resolution (a kernel argument: MapView
//              holds its reciprocal only), float multiply then float add per axis, every probe keyed as a point in its own right
//   counts     hits_r = edges with a hitting probe, hits_0 = edges whose centre probe hits
// Nothing of the map is written: no MapState field, no entries, no status bit — the kernels run on a read-attached map between
// steps as k_map_local_rows does.  The occupancy is a buffer of the map's own ([cells][m.words], not m.bitmap: that one belongs to
// an update in flight and has mod_cap rows) and is rebuilt by every call.
#pragma once

namespace liodom_dev {

constexpr int kRelocThreads = 256;
constexpr int kRelocWaves = kRelocThreads / 64;       // candidates of one workgroup: one wave each, contiguous
constexpr int kRelocBestThreads = 1024;

__device__ __forceinline__ int reloc_cells(const MapView& m, int occ_cells) { return max(0, min(min(m.st->n_cells, m.max_cells), occ_cells)); }

// occupancy, step 1: zeroes the rows of the cells the map holds, 16 bytes per store (the buffer is a hipMalloc of its own)
__global__ __launch_bounds__(256) void k_map_occ_clear(MapView m, unsigned int* occ, int occ_cells) {
  const size_t total = (size_t)reloc_cells(m, occ_cells) * (size_t)m.words, n4 = total / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
  uint4* o4 = reinterpret_cast<uint4*>(occ);
  for (size_t i = t; i < n4; i += step) o4[i] = make_uint4(0u, 0u, 0u, 0u);
  for (size_t i = n4 * 4 + t; i < total; i += step) occ[i] = 0u;
}

// occupancy, step 2, grid (x, y): one atomicOr per map point
__global__ __launch_bounds__(256) void k_map_occ_build(MapView m, unsigned int* occ, int occ_cells) {
  const int nc = reloc_cells(m, occ_cells);
  for (int c = blockIdx.y; c < nc; c += gridDim.y) {
    const int cnt = max(0, min(m.cell_n[c], m.cell_cap));
    const float4* src = map_cell_cur(m, c);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
      const float4 p = src[i];
      if (!(ld_isfinite((double)p.x) && ld_isfinite((double)p.y) && ld_isfinite((double)p.z))) continue;
      const int bit = map_leaf_bit(m, c, p);        // < gx * gy * gz <= 32 * words
      if (bit >= 0) atomicOr(&occ[(size_t)c * m.words + (bit >> 5)], 1u << (bit & 31));
    }
  }
}

// the three probes of one axis: coordinate, finiteness, coarse-cell key and leaf coordinate (map_leaf_bit's floorf(p * leaf_inv))
struct RelocAxis { int key[3], leaf[3]; bool fin[3]; };
__device__ __forceinline__ RelocAxis reloc_axis(float q, float leaf, float leaf_inv, double inv, double size, double half) {
  RelocAxis a;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float p = q + (float)(j - 1) * leaf;
    a.fin[j] = ld_isfinite((double)p);
    a.key[j] = map_cell_key((double)p, inv, size, half);
    a.leaf[j] = (int)floorf(p * leaf_inv);
  }
  return a;
}
template <typename V> __device__ __forceinline__ V reloc_sel3(int j, V a, V b, V c) { return j == 0 ? a : (j == 1 ? b : c); }

// the cell of a key, -1 if the map holds none (or one the occupancy has no row for)
__device__ __forceinline__ int reloc_find(const MapView& m, int occ_cells, int kx, int ky, int kz) {
  const int c = map_find_cell(m, kx, ky, kz);
  return (c >= 0 && c < m.max_cells && c < occ_cells) ? c : -1;
}
// the hit test: one 4-byte load of the occupancy word
__device__ __forceinline__ bool reloc_bit(const MapView& m, const unsigned int* occ, int cell, int lx, int ly, int lz) {
  const int rx = lx - m.cell_org[cell * 3 + 0], ry = ly - m.cell_org[cell * 3 + 1], rz = lz - m.cell_org[cell * 3 + 2];
  if (rx < 0 || rx >= m.gx || ry < 0 || ry >= m.gy || rz < 0 || rz >= m.gz) return false;
  const int bit = rx + ry * m.gx + rz * m.gx * m.gy;
  return ((occ[(size_t)cell * m.words + (bit >> 5)] >> (bit & 31)) & 1u) != 0u;
}

// One wave per candidate, lanes over the edges; a workgroup takes kRelocWaves contiguous candidates.
//   edges      read through the cache, one 16-byte load per lane and edge, consecutive lanes on consecutive edges — not staged in
//              the LDS: a scan's edge cloud (684 x 16 B = 11 KiB here) sits in the CU's 32 KiB L1 after the workgroup's first
//              wave has read it and in the L2 for every other workgroup, the load is one instruction per 27 probes, and the call
//              takes clouds up to max_update_points (16384 x 16 B = 256 KiB by default), which no LDS staging holds in one piece
//   T          the candidate is wave-uniform (readfirstlane of the wave's number): its 12 doubles are scalar loads
//   lookup     the dependent chain hash probe -> cell id -> cell_org -> occupancy row is walked once for the centre's key; a
//              displaced probe whose key equals the centre's reuses that cell, only one across a coarse-cell face looks up again
//   counts     ballot + popcount per round of 64 edges, summed in scalar registers; lane 0 stores both counts with one 8-byte
//              store.  No LDS, no atomics, no barrier.
__global__ __launch_bounds__(kRelocThreads) void k_map_score_poses(MapView m, const unsigned int* __restrict__ occ, int occ_cells,
                                                                   const float4* __restrict__ edges, int n_edges,
                                                                   const double* __restrict__ T_all, int n, int radius, float leaf, int* __restrict__ hits) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const int cand = (int)blockIdx.x * kRelocWaves + wave;
  if (cand >= n) return;
  const double* Tp = T_all + 12 * (size_t)cand;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; i++) T[i] = Tp[i];
  int n_r = 0, n_0 = 0;
  for (int base = 0; base < n_edges; base += 64) {
    const int i = base + lane;
    bool h0 = false, hr = false;
    if (i < n_edges) {
      const float4 e = edges[i];
      float qx, qy, qz;
      transform_point(T, e.x, e.y, e.z, &qx, &qy, &qz);
      const RelocAxis ax = reloc_axis(qx, leaf, m.leaf_inv, m.inv_xy, m.xy, m.half_xy);
      const RelocAxis ay = reloc_axis(qy, leaf, m.leaf_inv, m.inv_xy, m.xy, m.half_xy);
      const RelocAxis az = reloc_axis(qz, leaf, m.leaf_inv, m.inv_z, m.z, m.half_z);
      int c0 = -1;
      if (ax.fin[1] && ay.fin[1] && az.fin[1]) c0 = reloc_find(m, occ_cells, ax.key[1], ay.key[1], az.key[1]);
      if (c0 >= 0) h0 = reloc_bit(m, occ, c0, ax.leaf[1], ay.leaf[1], az.leaf[1]);
      hr = h0;
      if (radius && !hr) {
        for (int k = 0; k < 27 && !hr; k++) {
          if (k == 13) continue;                    // the centre
          const int jx = k % 3, jy = (k / 3) % 3, jz = k / 9;
          if (!(reloc_sel3(jx, ax.fin[0], ax.fin[1], ax.fin[2]) && reloc_sel3(jy, ay.fin[0], ay.fin[1], ay.fin[2]) &&
                reloc_sel3(jz, az.fin[0], az.fin[1], az.fin[2]))) continue;
          const int kx = reloc_sel3(jx, ax.key[0], ax.key[1], ax.key[2]), ky = reloc_sel3(jy, ay.key[0], ay.key[1], ay.key[2]),
                    kz = reloc_sel3(jz, az.key[0], az.key[1], az.key[2]);
          // (a finite displaced probe has a finite centre: c0 is the looked-up cell of the centre's key)
          const int cell = (kx == ax.key[1] && ky == ay.key[1] && kz == az.key[1]) ? c0 : reloc_find(m, occ_cells, kx, ky, kz);
          if (cell < 0) continue;
          hr = reloc_bit(m, occ, cell, reloc_sel3(jx, ax.leaf[0], ax.leaf[1], ax.leaf[2]), reloc_sel3(jy, ay.leaf[0], ay.leaf[1], ay.leaf[2]),
                         reloc_sel3(jz, az.leaf[0], az.leaf[1], az.leaf[2]));
        }
      }
    }
    n_r += __popcll(__ballot(hr));
    n_0 += __popcll(__ballot(h0));
  }
  if (lane == 0) reinterpret_cast<int2*>(hits)[cand] = make_int2(n_r, n_0);
}

// One workgroup: the maximum of the 64-bit keys (score << 32) | ~index over the n candidates — the largest score, ties to the lowest
// index — by shuffles inside a wave and one LDS word per wave.  out = {best index, its hits_r, its hits_0, n}; n = 0: {0, 0, 0, 0}.
__global__ __launch_bounds__(kRelocBestThreads) void k_map_score_best(const int* __restrict__ hits, int n, int* __restrict__ out) {
  __shared__ unsigned long long sh_best[kRelocBestThreads / 64];
  const int tid = threadIdx.x;
  unsigned long long best = 0ull;                   // below every candidate's key: ~index != 0 for index < 2^32 - 1
  for (int i = tid; i < n; i += kRelocBestThreads) {
    const int2 h = reinterpret_cast<const int2*>(hits)[i];
    const unsigned long long key = ((unsigned long long)(unsigned int)(h.x + h.y) << 32) | (unsigned long long)(~(unsigned int)i);
    best = key > best ? key : best;
  }
  for (int off = 32; off >= 1; off >>= 1) { const unsigned long long o = __shfl_xor(best, off); best = o > best ? o : best; }
  if ((tid & 63) == 0) sh_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kRelocBestThreads / 64; w++) best = sh_best[w] > best ? sh_best[w] : best;
    int4 r = make_int4(0, 0, 0, n);
    if (n > 0) {
      const int idx = (int)(~(unsigned int)best);
      const int2 h = reinterpret_cast<const int2*>(hits)[idx];
      r.x = idx; r.y = h.x; r.z = h.y;
    }
    *reinterpret_cast<int4*>(out) = r;
  }
}

}  // namespace liodom_dev
