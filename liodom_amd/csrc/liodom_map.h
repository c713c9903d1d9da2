// Device-side liodom::Map (rows A12-A14 of SURVEY.md §8): the mapping node's coarse-cell map,
// src/map.cc:70-189 and include/liodom/map.h:58-116 of the reference, rebuilt for MI355X.
//
//   Map::updateMap   (map.cc:90-129)  transform the edge cloud by the pose (FP64 -> float), key each
//                    point to a coarse cell int(floor(x / size) * size + size / 2) (:103-105), create
//                    missing cells in first-appearance order (cells_vector_, :110-114), append, then
//                    re-filter every modified cell with PCL VoxelGrid(resolution) (:124-128).
//   Map::getLocalMap (map.cc:141-189) and Map::getMap (:131-139): concatenations of cell clouds.
//
// PCL's VoxelGrid output is one centroid per occupied leaf, ordered by ascending leaf index, each
// centroid a float sum taken in cloud order divided by the count.  A modified cell's cloud is
// [previous centroids (ascending leaf), new points (input order)].  Instead of sorting, every
// modified cell gets a DENSE leaf-occupancy bitmap for the update (a 40 x 40 x 50 m cell at 0.4 m
// is 105 x 105 x 130 leaves = 175 KiB of bits incl. margins; HBM is plentiful), so that
//   output position of a leaf = number of occupied leaves before it = word prefix + popcount,
// which is exactly PCL's order (lexicographic z, y, x of the leaf coordinates).  Leaves holding one
// point (the common case: an old centroid nobody touched) are copied straight to their new
// position; leaves with several points collect the members' cloud-order indices and a half-wave
// sums them in ascending order — the same float additions in the same order as PCL.  Nothing here
// assumes that an old centroid still falls into the leaf it came from.
//
// Cells are slabs of fixed capacity, double-buffered (an update writes the other buffer of every
// modified cell and flips it at commit).  All counts live on the device: an update can be enqueued
// behind the odometry kernels with the edge cloud, its size and the pose read from device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "liodom_math.h"
#include "map_state_format.h"
#include "liodom_sizes.h"      // kMapRowsThreads

namespace liodom_dev {

constexpr int kMapLeafMargin = 2;       // leaves of slack around a cell for float rounding at its faces
constexpr int kMapNewCellsMax = 256;    // cells created by one update (LDS list)
constexpr int kMapLocalEntriesMax = 4096;
constexpr unsigned long long kMapEmptyKey = 0xFFFFFFFFFFFFFFFFull;

enum MapStatusBits {
  MAP_STATUS_UPDATE_OVERFLOW = 1,   // more points in one update than max_update_points
  MAP_STATUS_CELLS_FULL = 2,        // more coarse cells than max_cells / more new cells than the LDS list
  MAP_STATUS_MODIFIED_FULL = 4,     // more cells touched by one update than max_modified_cells
  MAP_STATUS_CELL_OVERFLOW = 8,     // a cell cloud outgrew cell_capacity
  MAP_STATUS_LEAF_RANGE = 16,       // a point's leaf fell outside its cell's dense grid (sizes not multiples?)
  MAP_STATUS_KEY_RANGE = 32,        // cell key beyond +-2^20
  MAP_STATUS_LOCAL_OVERFLOW = 64,   // getLocalMap / getMap result larger than the output buffer
};

struct MapState {
  int n_cells;       // cells_vector_.size()
  int n_mod;         // cells modified by the update in flight
  int n_new;         // points of the update in flight
  int n_multi;       // leaves with more than one point (update in flight)
  int cursor;        // allocation cursor of the member lists
  int status;
  int n_entries;     // getLocalMap / getMap plan
  int n_result;      // points of the last getLocalMap / getMap
};

struct MapEntry { int cell, offset, count, pad; };

struct MapView {
  // Map::Map (map.cc:70-81)
  double xy, inv_xy, half_xy, z, inv_z, half_z;
  float leaf_inv;                // PCL inverse_leaf_size_ = 1.0f / (float)resolution
  int gx, gy, gz, words;         // dense leaf grid of one cell (with margins), 32-bit words of its bitmap
  int max_cells, cell_cap, upd_cap, mod_cap, ctable;
  MapState* st;
  unsigned long long* ckey;      // [ctable] packed cell key or kMapEmptyKey   (HashMap cells_, map.h:91)
  int* cslot_cell;               // [ctable] cell id, -1 while the slot is being created
  int* cfirst;                   // [ctable] first input index that touched a slot under creation
  int* cell_key;                 // [max_cells][3] voxel_x, voxel_y, voxel_z as the reference computes them
  int* cell_org;                 // [max_cells][3] leaf coordinates of the dense grid's origin
  int* cell_n;                   // [max_cells] points in the cell
  int* cell_buf;                 // [max_cells] current slab (0 / 1)
  float4* slab;                  // [2][max_cells][cell_cap]
  // scratch of the update in flight
  float4* new_pts;               // [upd_cap] transformed input points
  int* new_cell;                 // [upd_cap] hash slot, then cell id
  int* new_mi;                   // [upd_cap] index of the point's cell in mod_list
  int* new_pos;                  // [upd_cap] leaf bit, then output position
  int* new_rank;                 // [upd_cap]
  int* mod_list;                 // [mod_cap] cell ids
  int* mod_of_cell;              // [max_cells] index in mod_list or -1
  int* mod_out_n;                // [mod_cap] points after filtering
  unsigned int* bitmap;          // [mod_cap][words]
  unsigned int* wprefix;         // [mod_cap][words]
  int* old_pos;                  // [mod_cap][cell_cap] leaf bit, then output position of the old points
  int* old_rank;                 // [mod_cap][cell_cap]
  unsigned int* leaf_cnt;        // [mod_cap][cell_cap] points per output leaf
  unsigned int* leaf_start;      // [mod_cap][cell_cap] member list start (leaves with > 1 point)
  int* members;                  // [mod_cap * cell_cap + upd_cap] cloud-order indices grouped by leaf (bound: map_build)
  int2* multi;                   // [(mod_cap * cell_cap + upd_cap + 1) / 2] (mod index, output position) of the multi-point leaves
  MapEntry* entries;             // [kMapLocalEntriesMax] plan of a getLocalMap
};

__device__ __forceinline__ unsigned int map_hash(unsigned long long k, unsigned int mask) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return (unsigned int)k & mask;
}
// HashKey (map.h:58-72): three ints.  Packed with 21 bits each (+-2^20 m).
__device__ __forceinline__ bool map_pack_key(int kx, int ky, int kz, unsigned long long* out) {
  const int B = 1 << 20;
  if (kx < -B || kx >= B || ky < -B || ky >= B || kz < -B || kz >= B) return false;
  *out = ((unsigned long long)(unsigned int)(kx + B) << 42) | ((unsigned long long)(unsigned int)(ky + B) << 21) |
         (unsigned long long)(unsigned int)(kz + B);
  return true;
}
// map.cc:103-105 (also :145,148,151 with an int argument)
__device__ __forceinline__ int map_cell_key(double x, double inv, double size, double half) {
  return (int)(floor(x * inv) * size + half);
}
// read-only lookup (no update in flight)
__device__ __forceinline__ int map_find_cell(const MapView& m, int kx, int ky, int kz) {
  unsigned long long key;
  if (!map_pack_key(kx, ky, kz, &key)) return -1;
  const unsigned int mask = (unsigned int)m.ctable - 1u;
  unsigned int h = map_hash(key, mask);
  for (int probe = 0; probe < m.ctable; probe++) {
    const unsigned long long k = m.ckey[h];
    if (k == key) return m.cslot_cell[h];
    if (k == kMapEmptyKey) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}
__device__ __forceinline__ const float4* map_cell_cur(const MapView& m, int cell) {
  return m.slab + ((size_t)m.cell_buf[cell] * m.max_cells + cell) * m.cell_cap;
}
__device__ __forceinline__ float4* map_cell_next(const MapView& m, int cell) {
  return m.slab + ((size_t)(m.cell_buf[cell] ^ 1) * m.max_cells + cell) * m.cell_cap;
}
// leaf bit of a point inside its cell's dense grid, -1 if outside
__device__ __forceinline__ int map_leaf_bit(const MapView& m, int cell, const float4& p) {
  const int rx = (int)floorf(p.x * m.leaf_inv) - m.cell_org[cell * 3 + 0];
  const int ry = (int)floorf(p.y * m.leaf_inv) - m.cell_org[cell * 3 + 1];
  const int rz = (int)floorf(p.z * m.leaf_inv) - m.cell_org[cell * 3 + 2];
  if (rx < 0 || rx >= m.gx || ry < 0 || ry >= m.gy || rz < 0 || rz >= m.gz) return -1;
  return rx + ry * m.gx + rz * m.gx * m.gy;
}

// ---------------------------------------------------------------------------------------------
// updateMap, step 1 (one workgroup): transform, cell keys, creation of missing cells in
// first-appearance order, list of modified cells.
// ---------------------------------------------------------------------------------------------
// kTransform = false (the lagged mapper, liodom_attach_mapper_ex with lag = 1): the input is in the world frame already — a frame
// that left a sliding window — and enters the map bit for bit; T_ptr is not read.
template <bool kTransform = true>
__global__ __launch_bounds__(1024) void k_map_assign(MapView m, const float4* in, const int* n_ptr, const double* T_ptr) {
  __shared__ double T[12];
  __shared__ int sh_newslot[kMapNewCellsMax];
  __shared__ int sh_nnew, sh_nmod, sh_n;
  const int tid = threadIdx.x;
  MapState& st = *m.st;
  if (kTransform && tid < 12) T[tid] = T_ptr[tid];
  if (tid == 0) {
    int n = *n_ptr;
    if (n > m.upd_cap) { n = m.upd_cap; atomicOr(&st.status, MAP_STATUS_UPDATE_OVERFLOW); }
    if (n < 0) n = 0;
    sh_n = n; sh_nnew = 0; sh_nmod = 0;
  }
  __syncthreads();
  const int n = sh_n;
  const unsigned int mask = (unsigned int)m.ctable - 1u;
  // phase A: claim / find the hash slot of every point's cell
  for (int i = tid; i < n; i += 1024) {
    const float4 e = in[i];
    float4 p = e;
    if (kTransform) transform_point(T, e.x, e.y, e.z, &p.x, &p.y, &p.z);        // map.cc:93-94
    m.new_pts[i] = p;
    const int kx = map_cell_key((double)p.x, m.inv_xy, m.xy, m.half_xy);      // :103
    const int ky = map_cell_key((double)p.y, m.inv_xy, m.xy, m.half_xy);      // :104
    const int kz = map_cell_key((double)p.z, m.inv_z, m.z, m.half_z);         // :105
    unsigned long long key;
    int slot = -1;
    if (map_pack_key(kx, ky, kz, &key)) {
      unsigned int h = map_hash(key, mask);
      for (int probe = 0; probe < m.ctable; probe++) {
        const unsigned long long prev = atomicCAS(&m.ckey[h], kMapEmptyKey, key);
        if (prev == kMapEmptyKey) {
          const int u = atomicAdd(&sh_nnew, 1);
          if (u < kMapNewCellsMax) sh_newslot[u] = (int)h;
          slot = (int)h;
          break;
        }
        if (prev == key) { slot = (int)h; break; }
        h = (h + 1) & mask;
      }
      if (slot >= 0 && *(volatile int*)&m.cslot_cell[slot] < 0) atomicMin(&m.cfirst[slot], i);
    } else {
      atomicOr(&st.status, MAP_STATUS_KEY_RANGE);
    }
    m.new_cell[i] = slot;
  }
  __threadfence();
  __syncthreads();
  // phase B: new cells get their ids in the order of the first point that touched them (:110-114)
  int nn = sh_nnew;
  if (nn > kMapNewCellsMax) { nn = kMapNewCellsMax; if (tid == 0) atomicOr(&st.status, MAP_STATUS_CELLS_FULL); }
  const int base_cells = st.n_cells;
  if (tid < nn) {
    const int hs = sh_newslot[tid];
    const int f = *(volatile int*)&m.cfirst[hs];
    int rank = 0;
    for (int u = 0; u < nn; u++) rank += (*(volatile int*)&m.cfirst[sh_newslot[u]] < f) ? 1 : 0;
    const int id = base_cells + rank;
    if (id < m.max_cells) {
      const float4 p = m.new_pts[f];
      m.cell_key[id * 3 + 0] = map_cell_key((double)p.x, m.inv_xy, m.xy, m.half_xy);
      m.cell_key[id * 3 + 1] = map_cell_key((double)p.y, m.inv_xy, m.xy, m.half_xy);
      m.cell_key[id * 3 + 2] = map_cell_key((double)p.z, m.inv_z, m.z, m.half_z);
      // dense leaf grid: origin = leaf of the cell's lower corner minus the margin
      m.cell_org[id * 3 + 0] = (int)floorf((float)(floor((double)p.x * m.inv_xy) * m.xy) * m.leaf_inv) - kMapLeafMargin;
      m.cell_org[id * 3 + 1] = (int)floorf((float)(floor((double)p.y * m.inv_xy) * m.xy) * m.leaf_inv) - kMapLeafMargin;
      m.cell_org[id * 3 + 2] = (int)floorf((float)(floor((double)p.z * m.inv_z) * m.z) * m.leaf_inv) - kMapLeafMargin;
      m.cell_n[id] = 0;
      m.cell_buf[id] = 0;
      m.cslot_cell[hs] = id;
    } else {
      m.cslot_cell[hs] = m.max_cells;       // marker: no room (points of this cell are dropped)
      atomicOr(&st.status, MAP_STATUS_CELLS_FULL);
    }
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) st.n_cells = min(base_cells + nn, m.max_cells);
  // phase C1: resolve ids, claim a place in the list of modified cells
  for (int i = tid; i < n; i += 1024) {
    const int slot = m.new_cell[i];
    int id = slot >= 0 ? *(volatile int*)&m.cslot_cell[slot] : -1;
    if (id >= m.max_cells) id = -1;
    m.new_cell[i] = id;
    if (id >= 0 && atomicCAS(&m.mod_of_cell[id], -1, -2) == -1) {
      const int mi = atomicAdd(&sh_nmod, 1);
      if (mi < m.mod_cap) { m.mod_list[mi] = id; atomicExch(&m.mod_of_cell[id], mi); }
      else { atomicExch(&m.mod_of_cell[id], -3); atomicOr(&st.status, MAP_STATUS_MODIFIED_FULL); }
    }
  }
  __threadfence();
  __syncthreads();
  // phase C2
  for (int i = tid; i < n; i += 1024) {
    const int id = m.new_cell[i];
    int mi = id >= 0 ? *(volatile int*)&m.mod_of_cell[id] : -1;
    if (mi < 0) mi = -1;
    m.new_mi[i] = mi;
  }
  if (tid == 0) { st.n_new = n; st.n_mod = min(sh_nmod, m.mod_cap); st.n_multi = 0; st.cursor = 0; }
}

// step 2: clear the bitmap and the leaf counters of every modified cell.  grid (x, mod_cap)
__global__ __launch_bounds__(256) void k_map_clear(MapView m) {
  const MapState& st = *m.st;
  const int mi = blockIdx.y;
  if (mi >= st.n_mod) return;
  const int cell = m.mod_list[mi];
  const int lim = min(m.cell_cap, m.cell_n[cell] + st.n_new);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < m.words || i < lim; i += gridDim.x * 256) {
    if (i < m.words) m.bitmap[(size_t)mi * m.words + i] = 0u;
    if (i < lim) m.leaf_cnt[(size_t)mi * m.cell_cap + i] = 0u;
  }
}

// Items of an update: row blockIdx.y < mod_cap = old points of modified cell y; row mod_cap = new points.
struct MapItem { int mi, cell, order; float4 p; bool valid, is_new; int idx; };
__device__ __forceinline__ MapItem map_item(const MapView& m) {
  MapItem it;
  it.valid = false;
  const MapState& st = *m.st;
  const int i = blockIdx.x * 256 + threadIdx.x;
  it.idx = i;
  if ((int)blockIdx.y == m.mod_cap) {
    it.is_new = true;
    if (i >= st.n_new) return it;
    it.mi = m.new_mi[i];
    if (it.mi < 0) return it;
    it.cell = m.new_cell[i];
    it.order = m.cell_n[it.cell] + i;          // after every old point, ascending in input order
    it.p = m.new_pts[i];
  } else {
    it.is_new = false;
    it.mi = blockIdx.y;
    if (it.mi >= st.n_mod) return it;
    it.cell = m.mod_list[it.mi];
    if (i >= m.cell_n[it.cell]) return it;
    it.order = i;
    it.p = map_cell_cur(m, it.cell)[i];
  }
  it.valid = true;
  return it;
}
__device__ __forceinline__ int* map_item_pos(const MapView& m, const MapItem& it) {
  return it.is_new ? &m.new_pos[it.idx] : &m.old_pos[(size_t)it.mi * m.cell_cap + it.idx];
}
__device__ __forceinline__ int* map_item_rank(const MapView& m, const MapItem& it) {
  return it.is_new ? &m.new_rank[it.idx] : &m.old_rank[(size_t)it.mi * m.cell_cap + it.idx];
}

// step 3: leaf occupancy.  grid (x, mod_cap + 1)
__global__ __launch_bounds__(256) void k_map_setbits(MapView m) {
  const MapItem it = map_item(m);
  if (!it.valid) return;
  // PCL skips non-finite points (is_dense == false path); transformed edges are always finite
  int bit = -1;
  if (ld_isfinite((double)it.p.x) && ld_isfinite((double)it.p.y) && ld_isfinite((double)it.p.z)) {
    bit = map_leaf_bit(m, it.cell, it.p);
    if (bit < 0) atomicOr(&m.st->status, MAP_STATUS_LEAF_RANGE);
  }
  *map_item_pos(m, it) = bit;
  if (bit >= 0) atomicOr(&m.bitmap[(size_t)it.mi * m.words + (bit >> 5)], 1u << (bit & 31));
}

// step 4: exclusive prefix of the popcounts of a modified cell's bitmap words.  grid (mod_cap)
__global__ __launch_bounds__(1024) void k_map_prefix(MapView m) {
  __shared__ int sh_w[16];
  __shared__ int sh_carry;
  MapState& st = *m.st;
  const int mi = blockIdx.x;
  if (mi >= st.n_mod) return;
  const int tid = threadIdx.x;
  const unsigned int* bm = m.bitmap + (size_t)mi * m.words;
  unsigned int* wp = m.wprefix + (size_t)mi * m.words;
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < m.words; base += 1024 * 4) {
    const int i0 = base + tid * 4;
    int c[4];
    int sum = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { c[k] = (i0 + k < m.words) ? __popc(bm[i0 + k]) : 0; sum += c[k]; }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if ((tid & 63) >= off) incl += t; }
    if ((tid & 63) == 63) sh_w[tid >> 6] = incl;
    __syncthreads();
    int run = sh_carry + incl - sum;
    for (int q = 0; q < (tid >> 6); q++) run += sh_w[q];
#pragma unroll
    for (int k = 0; k < 4; k++) { if (i0 + k < m.words) wp[i0 + k] = (unsigned int)run; run += c[k]; }
    __syncthreads();
    if (tid == 1023) sh_carry = run;
    __syncthreads();
  }
  if (tid == 0) {
    int total = sh_carry;
    if (total > m.cell_cap) { total = m.cell_cap; atomicOr(&st.status, MAP_STATUS_CELL_OVERFLOW); }
    m.mod_out_n[mi] = total;
  }
}

// step 5: output position of every point and points per output leaf.  grid (x, mod_cap + 1)
__global__ __launch_bounds__(256) void k_map_count(MapView m) {
  const MapItem it = map_item(m);
  if (!it.valid) return;
  int* pp = map_item_pos(m, it);
  const int bit = *pp;
  if (bit < 0) return;
  const size_t w = (size_t)it.mi * m.words + (bit >> 5);
  const int pos = (int)m.wprefix[w] + __popc(m.bitmap[w] & ((1u << (bit & 31)) - 1u));
  if (pos >= m.cell_cap) { *pp = -1; return; }
  *pp = pos;
  *map_item_rank(m, it) = (int)atomicAdd(&m.leaf_cnt[(size_t)it.mi * m.cell_cap + pos], 1u);
}

// step 6: member-list allocation for the leaves with more than one point.  grid (x, mod_cap)
__global__ __launch_bounds__(256) void k_map_alloc(MapView m) {
  MapState& st = *m.st;
  const int mi = blockIdx.y;
  if (mi >= st.n_mod) return;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= m.mod_out_n[mi]) return;
  const unsigned int c = m.leaf_cnt[(size_t)mi * m.cell_cap + pos];
  if (c > 1u) {
    m.leaf_start[(size_t)mi * m.cell_cap + pos] = (unsigned int)atomicAdd(&st.cursor, (int)c);
    m.multi[atomicAdd(&st.n_multi, 1)] = make_int2(mi, pos);
  }
}

// step 7: single-point leaves are written to their new position; the others list their members.
__global__ __launch_bounds__(256) void k_map_emit(MapView m) {
  const MapItem it = map_item(m);
  if (!it.valid) return;
  const int pos = *map_item_pos(m, it);
  if (pos < 0) return;
  const size_t li = (size_t)it.mi * m.cell_cap + pos;
  const unsigned int c = m.leaf_cnt[li];
  if (c == 1u) {
    // PCL: centroid = 0 + p, then / 1
    float4 o;
    o.x = (0.0f + it.p.x) / 1.0f; o.y = (0.0f + it.p.y) / 1.0f; o.z = (0.0f + it.p.z) / 1.0f; o.w = (0.0f + it.p.w) / 1.0f;
    map_cell_next(m, it.cell)[pos] = o;
  } else {
    m.members[m.leaf_start[li] + (unsigned int)*map_item_rank(m, it)] = it.order;
  }
}

// step 8: centroid of a multi-point leaf, members summed in cloud order.  32 lanes per leaf.
__global__ __launch_bounds__(256) void k_map_centroid(MapView m) {
  const MapState& st = *m.st;
  const int q = blockIdx.x * 8 + (threadIdx.x >> 5);
  const int hl = threadIdx.x & 31;
  for (int leaf = q; leaf < st.n_multi; leaf += gridDim.x * 8) {
    const int2 mp = m.multi[leaf];
    const int cell = m.mod_list[mp.x];
    const size_t li = (size_t)mp.x * m.cell_cap + mp.y;
    const int cnt = (int)m.leaf_cnt[li];
    const int* list = m.members + m.leaf_start[li];
    const int n_old = m.cell_n[cell];
    const float4* cur = map_cell_cur(m, cell);
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    int last = -1;
    for (int k = 0; k < cnt; k++) {
      int best = 0x7fffffff;                      // smallest cloud-order index above `last`
      for (int j = hl; j < cnt; j += 32) { const int o = list[j]; if (o > last && o < best) best = o; }
      for (int off = 16; off >= 1; off >>= 1) best = min(best, __shfl_xor(best, off));
      const float4 p = best < n_old ? cur[best] : m.new_pts[best - n_old];
      sx += p.x; sy += p.y; sz += p.z; si += p.w;
      last = best;
    }
    if (hl == 0) {
      const float c = (float)cnt;
      map_cell_next(m, cell)[mp.y] = make_float4(sx / c, sy / c, sz / c, si / c);
    }
  }
}

// step 9: flip the slabs of the modified cells.
__global__ __launch_bounds__(256) void k_map_commit(MapView m) {
  MapState& st = *m.st;
  const int nm = st.n_mod;
  for (int mi = threadIdx.x; mi < nm; mi += 256) {
    const int cell = m.mod_list[mi];
    m.cell_n[cell] = m.mod_out_n[mi];
    m.cell_buf[cell] ^= 1;
    m.mod_of_cell[cell] = -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) { st.n_mod = 0; st.n_new = 0; }
}

// ---------------------------------------------------------------------------------------------
// getLocalMap (map.cc:141-189): the cells of a (2*cells_xy+1)^2 square at the pose's z layer, x outer
// and y inner, then a z column through the centre cell.  Reproduced as written: the translation is
// truncated to int first (:144,147,150); the z column's extent uses voxel_xysize_ but steps by
// voxel_zsize_ (:175-178); the centre cell is visited by both loops; int loop variables advance by
// `i += double`.  One thread plans (<= a few dozen lookups), k_map_gather copies.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void map_plan_add(const MapView& m, int kx, int ky, int kz, int* ne, int* total) {
  const int cell = map_find_cell(m, kx, ky, kz);
  if (cell < 0 || cell >= m.max_cells) return;
  if (*ne >= kMapLocalEntriesMax) { atomicOr(&m.st->status, MAP_STATUS_LOCAL_OVERFLOW); return; }
  MapEntry e; e.cell = cell; e.offset = *total; e.count = m.cell_n[cell]; e.pad = 0;
  m.entries[*ne] = e;
  *ne += 1;
  *total += e.count;
}
// The loop guard of the planners: a visit is cut after kMapVisitMax loop iterations (inner and outer together), so that no sizes
// or extents can keep the planning lane busy without end.  A loop that ends on it has left keys out: the planner raises
// MAP_STATUS_LOCAL_OVERFLOW, whatever `sticky` is (as for more than kMapLocalEntriesMax found cells).  `cut = map_visit_cut(guard)`
// stands behind the loop's own condition, so it is evaluated — and 1 — only while the loop would still go on.
constexpr int kMapVisitMax = 65536;
__device__ __forceinline__ int map_visit_cut(int guard) { return guard >= kMapVisitMax ? 1 : 0; }

__global__ void k_map_local_plan(MapView m, const double* T_ptr, int cells_xy, int cells_z, int out_cap, int* n_out, int sticky) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  MapState& st = *m.st;
  const int x = (int)T_ptr[3];                                                       // :144
  const int voxel_x = map_cell_key((double)x, m.inv_xy, m.xy, m.half_xy);
  const int y = (int)T_ptr[7];                                                       // :147
  const int voxel_y = map_cell_key((double)y, m.inv_xy, m.xy, m.half_xy);
  const int z = (int)T_ptr[11];                                                      // :150
  const int voxel_z = map_cell_key((double)z, m.inv_z, m.z, m.half_z);
  const int init_x = (int)(voxel_x - cells_xy * m.xy);                               // :157-160
  const int end_x = (int)(voxel_x + cells_xy * m.xy);
  const int init_y = (int)(voxel_y - cells_xy * m.xy);
  const int end_y = (int)(voxel_y + cells_xy * m.xy);
  int ne = 0, total = 0, guard = 0, cut = 0;
  for (int i = init_x; i <= end_x && !(cut = map_visit_cut(guard)); i = (int)(i + m.xy), guard++) {          // :162
    for (int j = init_y; j <= end_y && !(cut = map_visit_cut(guard)); j = (int)(j + m.xy), guard++) {        // :163
      map_plan_add(m, i, j, voxel_z, &ne, &total);
    }
  }
  const int init_z = (int)(voxel_z - cells_z * m.xy);                                // :175 (xy size)
  const int end_z = (int)(voxel_z + cells_z * m.xy);                                 // :176
  for (int i = init_z; i <= end_z && !(cut = map_visit_cut(guard)); i = (int)(i + m.z), guard++) {   // :178
    map_plan_add(m, voxel_x, voxel_y, i, &ne, &total);
  }
  if (cut) atomicOr(&st.status, MAP_STATUS_LOCAL_OVERFLOW);                         // keys were left out: whatever `sticky` is
  if (total > out_cap && sticky) atomicOr(&st.status, MAP_STATUS_LOCAL_OVERFLOW);   // host callers get LIODOM_ERR_CAPACITY instead
  st.n_entries = ne;
  st.n_result = total;
  if (n_out) *n_out = total > out_cap ? out_cap : total;
}

// getMap (map.cc:131-139), every cell in cells_vector_ order, has no plan of its own: liodom_map_get_all plans with k_map_pack_plan
// and copies with k_map_pack (below), which hold any number of cells.  The entries above are getLocalMap's alone.

// grid (x, entries): copies the planned cells to the output
__global__ __launch_bounds__(256) void k_map_gather(MapView m, float4* out, int out_cap) {
  const MapState& st = *m.st;
  for (int e = blockIdx.y; e < st.n_entries; e += gridDim.y) {
    const MapEntry en = m.entries[e];
    const float4* src = map_cell_cur(m, en.cell);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < en.count; i += gridDim.x * 256) {
      const int o = en.offset + i;
      if (o < out_cap) out[o] = src[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// getLocalMap for a batch of poses against ONE map in one launch (liodom_map_get_local_batch, and the per-scan path of the map
// readers of liodom_attach_map_reader; no counterpart in the reference, which asks one pose at a time).  grid (x, rows).  Every
// workgroup plans its row in LDS — no MapView::entries, no MapState::n_entries / n_result: nothing of the map is written, so
// any number of rows, of this launch or of others, can share a map — and copies its slice of the row's result.
//   plan    one lane enumerates the keys with the loops of k_map_local_plan as they stand (translation truncated to int first,
//           i = (int)(i + m.xy), the z column's extent from the xy size, the centre cell visited twice); the lanes look the keys
//           up in parallel; a scan over (found, count) in key order gives the entries k_map_local_plan would have written and
//           their offsets.
//   copy    the row's n = min(total, cap) output points are dealt to the row's workgroups in contiguous slices (the x extent is
//           capped by the host; a slice is walked 256 points at a time); one 16-byte load and one 16-byte store per point,
//           consecutive lanes on consecutive points.
// Output of a row: what k_map_local_plan + k_map_gather leave for the same pose and capacity, bit for bit — order, duplicates,
// truncation at cap, n = min(total, cap), the sticky MAP_STATUS_LOCAL_OVERFLOW (sticky != 0 only).
// The LDS plan holds kMapRowsKeysMax keys.  The host launches this kernel only for extents whose visit cannot exceed that
// (map_rows_fit in liodom_map_host.h: a bound over every pose) and runs the two old launches per row otherwise; should a row
// get here with more keys all the same, the plan stops at the cap and raises MAP_STATUS_LOCAL_OVERFLOW.
// ---------------------------------------------------------------------------------------------
constexpr int kMapRowsKeysMax = 1024;
constexpr int kMapRowsGridX = 16;       // most workgroups a row is dealt to
constexpr int kMapRowsGridMax = 2048;   // most workgroups of a launch

// Where the rows of a launch live.  Row `row` works for index idx = s0 + row, or list[row] (kList: a subset step's stream list).
// sel != nullptr (step path): idx is a stream; it takes part iff sel[idx].x == tag (it reads THIS map), with the extents
// sel[idx].y / .z it was attached with.  sel == nullptr (batch call): every row takes part with cells_xy / cells_z.
struct MapRows {
  const double* T;  long long T_stride;      // pose of idx: T + idx * T_stride, 12 doubles (row-major 3 x 4)
  float4* out;      long long out_stride;    // result of idx: out + idx * out_stride, room for `cap` points
  int* n_out;       long long n_stride;      // points written: n_out[idx * n_stride]
  int* total;                                // (optional) [idx] size of the full result, whatever cap is
  const int4* sel;
  const int* list;
  int tag, s0, cap, cells_xy, cells_z, sticky;
};

template <bool kList = false>
__global__ __launch_bounds__(kMapRowsThreads) void k_map_local_rows(MapView m, MapRows r) {
  __shared__ int sh_key[3][kMapRowsKeysMax];
  __shared__ int sh_cell[kMapRowsKeysMax];          // the entries, compacted: cell id
  __shared__ int sh_off[kMapRowsKeysMax + 1];       // ... and offset; [ne] = total
  __shared__ int sh_wf[kMapRowsThreads / 64], sh_wc[kMapRowsThreads / 64];
  __shared__ int sh_nk, sh_over, sh_ne, sh_total;
  const int tid = threadIdx.x;
  const int row = blockIdx.y;
  const int idx = kList ? r.list[row] : r.s0 + row;
  int cells_xy = r.cells_xy, cells_z = r.cells_z;
  if (r.sel) {
    const int4 sl = r.sel[idx];
    if (sl.x != r.tag) return;                      // (uniform) not a reader of this map
    cells_xy = sl.y; cells_z = sl.z;
  }
  if (tid == 0) {
    const double* T_ptr = r.T + (long long)idx * r.T_stride;
    int nk = 0, over = 0;
    auto add = [&](int kx, int ky, int kz) {
      if (nk < kMapRowsKeysMax) { sh_key[0][nk] = kx; sh_key[1][nk] = ky; sh_key[2][nk] = kz; nk++; }
      else over = 1;
    };
    const int x = (int)T_ptr[3];                                                       // :144
    const int voxel_x = map_cell_key((double)x, m.inv_xy, m.xy, m.half_xy);
    const int y = (int)T_ptr[7];                                                       // :147
    const int voxel_y = map_cell_key((double)y, m.inv_xy, m.xy, m.half_xy);
    const int z = (int)T_ptr[11];                                                      // :150
    const int voxel_z = map_cell_key((double)z, m.inv_z, m.z, m.half_z);
    const int init_x = (int)(voxel_x - cells_xy * m.xy);                               // :157-160
    const int end_x = (int)(voxel_x + cells_xy * m.xy);
    const int init_y = (int)(voxel_y - cells_xy * m.xy);
    const int end_y = (int)(voxel_y + cells_xy * m.xy);
    int guard = 0, cut = 0;
    for (int i = init_x; i <= end_x && !over && !(cut = map_visit_cut(guard)); i = (int)(i + m.xy), guard++) {          // :162
      for (int j = init_y; j <= end_y && !over && !(cut = map_visit_cut(guard)); j = (int)(j + m.xy), guard++) {        // :163
        add(i, j, voxel_z);
      }
    }
    const int init_z = (int)(voxel_z - cells_z * m.xy);                                // :175 (xy size)
    const int end_z = (int)(voxel_z + cells_z * m.xy);                                 // :176
    for (int i = init_z; i <= end_z && !over && !(cut = map_visit_cut(guard)); i = (int)(i + m.z), guard++) {   // :178
      add(voxel_x, voxel_y, i);
    }
    sh_nk = nk; sh_over = over | cut; sh_ne = 0; sh_total = 0;          // either way keys were left out
  }
  __syncthreads();
  const int nk = sh_nk;
  // lookups in parallel, then the scan of k_map_evict_plan over (found, count) in key order, chunk after chunk
  for (int base = 0; base < nk; base += kMapRowsThreads) {
    const int k = base + tid;
    int cell = -1, cnt = 0;
    if (k < nk) {
      const int c = map_find_cell(m, sh_key[0][k], sh_key[1][k], sh_key[2][k]);
      if (c >= 0 && c < m.max_cells) { cell = c; cnt = m.cell_n[c]; }
    }
    const int f = cell >= 0 ? 1 : 0;
    int inf = f, inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      const int tf = __shfl_up(inf, off), tc = __shfl_up(inc, off);
      if ((tid & 63) >= off) { inf += tf; inc += tc; }
    }
    if ((tid & 63) == 63) { sh_wf[tid >> 6] = inf; sh_wc[tid >> 6] = inc; }
    __syncthreads();
    int j = sh_ne + inf - f, o = sh_total + inc - cnt;
    for (int q = 0; q < (tid >> 6); q++) { j += sh_wf[q]; o += sh_wc[q]; }
    if (f) { sh_cell[j] = cell; sh_off[j] = o; }      // j < nk <= kMapRowsKeysMax
    __syncthreads();
    if (tid == kMapRowsThreads - 1) { sh_ne = j + f; sh_total = o + cnt; }
    __syncthreads();
  }
  const int ne = sh_ne, total = sh_total;
  if (tid == 0) sh_off[ne] = total;
  __syncthreads();
  const int n = total > r.cap ? r.cap : total;
  if (blockIdx.x == 0 && tid == 0) {
    if ((total > r.cap && r.sticky) || sh_over) atomicOr(&m.st->status, MAP_STATUS_LOCAL_OVERFLOW);
    r.n_out[(long long)idx * r.n_stride] = n;
    if (r.total) r.total[idx] = total;
  }
  // this workgroup's slice [lo, hi) of the row's n output points
  const int per = (n + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = min(n, (int)blockIdx.x * per), hi = min(n, lo + per);
  if (lo >= hi) return;
  int e = 0;
  {                                                   // first entry that reaches past lo (entries of 0 points share an offset)
    int a = 0, b = ne;                                // invariant: sh_off[a] <= lo < sh_off[b]
    while (b - a > 1) { const int mid = (a + b) >> 1; if (sh_off[mid] <= lo) a = mid; else b = mid; }
    e = a;
  }
  float4* out = r.out + (long long)idx * r.out_stride;
  for (; e < ne && sh_off[e] < hi; e++) {
    const int o0 = sh_off[e];
    const int a = max(o0, lo), b = min(sh_off[e + 1], hi);
    const float4* src = map_cell_cur(m, sh_cell[e]);
    for (int o = a + tid; o < b; o += kMapRowsThreads) out[o] = src[o - o0];
  }
}

// fills the bookkeeping arrays at creation
__global__ __launch_bounds__(256) void k_map_init(MapView m) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m.ctable) { m.ckey[i] = kMapEmptyKey; m.cslot_cell[i] = -1; m.cfirst[i] = 0x7fffffff; }
  if (i < m.max_cells) { m.mod_of_cell[i] = -1; m.cell_n[i] = 0; m.cell_buf[i] = 0; }
  if (i == 0) { MapState z = {}; *m.st = z; }
}

// ---------------------------------------------------------------------------------------------
// The map as a blob (map_state_format.h): liodom_map_export_state / liodom_map_import_state / liodom_map_reset.  None of this is
// on the per-scan path: a map that never calls those entry points launches none of these kernels and allocates nothing for them.
// The blob's head (header + cell records) and its point section are two device buffers; the host writes the rest of the header.
// ---------------------------------------------------------------------------------------------
// Export, step 1 (one workgroup): exclusive prefix over cell_n in creation order, chunk after chunk with a carry, for any number of
// cells (no plan entries: the records are the plan); liodom_map_get_all plans with it too.  Writes the cell records behind the
// header and n_cells, status and n_points into the header, where the host reads them.  `head` holds kMapStateHeaderBytes +
// max_cells records.
__global__ __launch_bounds__(1024) void k_map_pack_plan(MapView m, unsigned char* head) {
  __shared__ int sh_w[16];
  __shared__ long long sh_carry;
  const MapState& st = *m.st;
  const int tid = threadIdx.x;
  const int nc = max(0, min(st.n_cells, m.max_cells));
  MapStateRecord* rec = reinterpret_cast<MapStateRecord*>(head + kMapStateHeaderBytes);
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < nc; base += 1024) {
    const int c = base + tid;
    const int cnt = c < nc ? max(0, min(m.cell_n[c], m.cell_cap)) : 0;
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if ((tid & 63) >= off) incl += t; }
    if ((tid & 63) == 63) sh_w[tid >> 6] = incl;
    __syncthreads();
    long long run = sh_carry + (incl - cnt);
    for (int q = 0; q < (tid >> 6); q++) run += sh_w[q];
    if (c < nc) {
      MapStateRecord r;
      for (int a = 0; a < 3; a++) { r.key[a] = m.cell_key[c * 3 + a]; r.corner_leaf[a] = m.cell_org[c * 3 + a] + kMapLeafMargin; }
      r.count = cnt;
      r.first = (int)run;
      rec[c] = r;
    }
    __syncthreads();
    if (tid == 1023) sh_carry = run + cnt;
    __syncthreads();
  }
  if (tid == 0) {
    MapStateHeader* hd = reinterpret_cast<MapStateHeader*>(head);
    hd->n_cells = nc;
    hd->status = (uint32_t)st.status;
    hd->n_points = sh_carry;
  }
}

// Export, step 2, grid (x, y): gathers every cell's current slab into the point section — one 16-byte load and one 16-byte store
// per point, consecutive lanes on consecutive points.  Reads the plan from the records k_map_pack_plan wrote.
__global__ __launch_bounds__(256) void k_map_pack(MapView m, const unsigned char* head, float4* pts, int pts_cap) {
  const MapStateHeader* hd = reinterpret_cast<const MapStateHeader*>(head);
  const MapStateRecord* rec = reinterpret_cast<const MapStateRecord*>(head + kMapStateHeaderBytes);
  const int nc = max(0, min(hd->n_cells, m.max_cells));
  for (int c = blockIdx.y; c < nc; c += gridDim.y) {
    const int first = rec[c].first, cnt = min(rec[c].count, m.cell_cap);
    const float4* src = map_cell_cur(m, c);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
      const long long o = (long long)first + i;
      if (o >= 0 && o < pts_cap) pts[o] = src[i];
    }
  }
}

// Import, grid (x, y), launched behind k_map_init (which leaves the map empty: hash, cell_n, cell_buf, mod_of_cell = -1, every
// counter 0; liodom_map_reset is that launch alone).  For every record: the key goes into the hash with the map_hash / linear
// probe map_find_cell and k_map_assign read (keys are distinct — the host's map_state_validate has seen to it — so the slots are
// claimed in parallel; which slot a key lands in is invisible to every later lookup), then cslot_cell, cell_key, cell_org =
// corner_leaf - kMapLeafMargin, cell_n; cell_buf stays 0 and the points go into slab 0.  Any number of cells: nothing here is
// sized by kMapNewCellsMax.  The host has validated the blob against this map's capacities; counts are clamped all the same.
__global__ __launch_bounds__(256) void k_map_unpack(MapView m, const unsigned char* head, const float4* pts, int n_cells, int n_points,
                                                    int status) {
  const MapStateRecord* rec = reinterpret_cast<const MapStateRecord*>(head + kMapStateHeaderBytes);
  const int nc = max(0, min(n_cells, m.max_cells));
  const unsigned int mask = (unsigned int)m.ctable - 1u;
  const int nthreads = gridDim.x * gridDim.y * 256;
  for (int c = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; c < nc; c += nthreads) {
    const MapStateRecord r = rec[c];
    unsigned long long key;
    if (map_pack_key(r.key[0], r.key[1], r.key[2], &key)) {
      unsigned int h = map_hash(key, mask);
      for (int probe = 0; probe < m.ctable; probe++) {
        if (atomicCAS(&m.ckey[h], kMapEmptyKey, key) == kMapEmptyKey) { m.cslot_cell[h] = c; break; }
        h = (h + 1) & mask;
      }
    }
    for (int a = 0; a < 3; a++) {
      m.cell_key[c * 3 + a] = r.key[a];
      m.cell_org[c * 3 + a] = (int)((unsigned int)r.corner_leaf[a] - (unsigned int)kMapLeafMargin);
    }
    m.cell_n[c] = max(0, min(r.count, m.cell_cap));
  }
  for (int c = blockIdx.y; c < nc; c += gridDim.y) {
    const int first = rec[c].first, cnt = min(rec[c].count, m.cell_cap);
    float4* dst = m.slab + (size_t)c * m.cell_cap;          // slab 0
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
      const long long o = (long long)first + i;
      if (o >= 0 && o < n_points) dst[i] = pts[o];
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { m.st->n_cells = nc; m.st->status = status; }
}

// ---------------------------------------------------------------------------------------------
// Pruning (liodom_map_prune, the auto-prune of liodom_attach_mapper_ex; no counterpart in the reference, whose map only grows):
// every cell outside a box of cells around a pose is dropped.  Afterwards the map is what liodom_map_import_state would make of
// its own blob with the dropped cells' records and points taken out: the survivors keep their relative creation order and are
// renumbered densely, the cell hash (open addressing, no tombstones: nothing can be deleted in place) is rebuilt from them — which
// also drops the "no room" slots an earlier CELLS_FULL left —, sticky status bits stay.  A map that never prunes launches none of
// this and allocates nothing for it.
//
// Moving the slabs without a hazard: survivor c -> new id j <= c.  Its points are copied from its CURRENT slab (cell_buf[c], c) to
// the NON-current slab of id j, (cell_buf[j] ^ 1, j), and cell_buf[j] is flipped.  Every source of the move is a current slab
// (b_c, c); a destination (b_j ^ 1, j) could only be a source if c' = j and b_j = b_j ^ 1.  So the move is one grid, in any order.
// A survivor whose id does not change (j = c) stays where it is.
// ---------------------------------------------------------------------------------------------
constexpr int kMapPruneThreads = 1024;
// One entry per survivor (16 bytes, one load in the move grid): old id, slab it is read from, slab of id j it goes to, points.
// Entry [max_cells] is the host's: {cells removed, cells before, cells after, 0}.
struct __attribute__((aligned(16))) MapPruneMove { int src, src_buf, dst_buf, count; };

// The keep box, shared by k_map_prune_plan and k_map_evict_plan so that the two cannot drift: centre cell from T exactly as
// k_map_local_plan (translation truncated to int first, map.cc:144-151), extents in double.
struct MapKeepBox { int vx, vy, vz; double lim_xy, lim_z; };
__device__ __forceinline__ MapKeepBox map_keep_box(const MapView& m, const double* T_ptr, int keep_xy, int keep_z) {
  const int x = (int)T_ptr[3], y = (int)T_ptr[7], z = (int)T_ptr[11];                 // map.cc:144,147,150
  MapKeepBox b;
  b.vx = map_cell_key((double)x, m.inv_xy, m.xy, m.half_xy);
  b.vy = map_cell_key((double)y, m.inv_xy, m.xy, m.half_xy);
  b.vz = map_cell_key((double)z, m.inv_z, m.z, m.half_z);
  b.lim_xy = (double)keep_xy * m.xy; b.lim_z = (double)keep_z * m.z;
  return b;
}
__device__ __forceinline__ int map_keep_cell(const MapKeepBox& b, const int* key) {
  return (fabs((double)key[0] - (double)b.vx) <= b.lim_xy && fabs((double)key[1] - (double)b.vy) <= b.lim_xy &&
          fabs((double)key[2] - (double)b.vz) <= b.lim_z) ? 1 : 0;
}

// Step 1.  Workgroup 0 plans: centre cell from T exactly as k_map_local_plan (translation truncated to int first, map.cc:144-151),
// keep flags, exclusive scan over creation order (the scan of k_map_pack_plan, any number of cells), and the bookkeeping arrays
// compacted in place, chunk after chunk: a chunk's threads hold their cells' records in registers across the scan's barrier and
// write to ids j <= c, i.e. to places of this chunk or of earlier ones, all read already; no place is written twice.
// Workgroups 1 .. : the cell hash back to the state k_map_init leaves (independent of the plan; the move grid re-inserts).
__global__ __launch_bounds__(kMapPruneThreads) void k_map_prune_plan(MapView m, const double* T_ptr, int keep_xy, int keep_z, MapPruneMove* mv) {
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    for (int i = ((int)blockIdx.x - 1) * kMapPruneThreads + tid; i < m.ctable; i += ((int)gridDim.x - 1) * kMapPruneThreads) {
      m.ckey[i] = kMapEmptyKey; m.cslot_cell[i] = -1; m.cfirst[i] = 0x7fffffff;
    }
    return;
  }
  __shared__ int sh_w[16];
  __shared__ int sh_carry;
  MapState& st = *m.st;
  const int nc = max(0, min(st.n_cells, m.max_cells));
  const MapKeepBox box = map_keep_box(m, T_ptr, keep_xy, keep_z);
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < nc; base += kMapPruneThreads) {
    const int c = base + tid;
    int key[3] = {0, 0, 0}, org[3] = {0, 0, 0}, cnt = 0, buf = 0, keep = 0;
    if (c < nc) {
      for (int a = 0; a < 3; a++) { key[a] = m.cell_key[c * 3 + a]; org[a] = m.cell_org[c * 3 + a]; }
      cnt = max(0, min(m.cell_n[c], m.cell_cap));
      buf = m.cell_buf[c] & 1;
      keep = map_keep_cell(box, key);
    }
    int incl = keep;
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if ((tid & 63) >= off) incl += t; }
    if ((tid & 63) == 63) sh_w[tid >> 6] = incl;
    __syncthreads();                      // (every record of the chunk is in registers from here on)
    int j = sh_carry + incl - keep;
    for (int q = 0; q < (tid >> 6); q++) j += sh_w[q];
    if (keep) {
      for (int a = 0; a < 3; a++) { m.cell_key[j * 3 + a] = key[a]; m.cell_org[j * 3 + a] = org[a]; }
      m.cell_n[j] = cnt;
      MapPruneMove e;
      e.src = c; e.src_buf = buf; e.count = cnt;
      e.dst_buf = (j == c) ? buf : ((m.cell_buf[j] & 1) ^ 1);      // (cell_buf[j] is written by id j's survivor alone: this thread)
      m.cell_buf[j] = e.dst_buf;
      mv[j] = e;
    }
    __syncthreads();
    if (tid == kMapPruneThreads - 1) sh_carry = j + keep;
    __syncthreads();
  }
  if (tid == 0) {
    const int kept = sh_carry;
    MapPruneMove info; info.src = nc - kept; info.src_buf = nc; info.dst_buf = kept; info.count = 0;
    mv[m.max_cells] = info;
    st.n_cells = kept;
  }
}

// Step 2, grid (chunk, survivor): the survivors' keys into the cleared hash (distinct keys, slots claimed in parallel as in
// k_map_unpack), and the slabs of those whose id changed — one 16-byte load and one 16-byte store per point, consecutive lanes on
// consecutive points, only cell_n points of a cell.
__global__ __launch_bounds__(256) void k_map_prune_move(MapView m, const MapPruneMove* mv) {
  const int nc = max(0, min(m.st->n_cells, m.max_cells));
  const unsigned int mask = (unsigned int)m.ctable - 1u;
  const int nthreads = gridDim.x * gridDim.y * 256;
  for (int c = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; c < nc; c += nthreads) {
    unsigned long long key;
    if (map_pack_key(m.cell_key[c * 3 + 0], m.cell_key[c * 3 + 1], m.cell_key[c * 3 + 2], &key)) {
      unsigned int h = map_hash(key, mask);
      for (int probe = 0; probe < m.ctable; probe++) {
        if (atomicCAS(&m.ckey[h], kMapEmptyKey, key) == kMapEmptyKey) { m.cslot_cell[h] = c; break; }
        h = (h + 1) & mask;
      }
    }
  }
  for (int j = blockIdx.y; j < nc; j += gridDim.y) {
    const MapPruneMove e = mv[j];
    if (e.src == j || e.src < 0 || e.src >= m.max_cells) continue;
    const int cnt = min(e.count, m.cell_cap);
    const float4* src = m.slab + ((size_t)(e.src_buf & 1) * m.max_cells + e.src) * m.cell_cap;
    float4* dst = m.slab + ((size_t)(e.dst_buf & 1) * m.max_cells + j) * m.cell_cap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) dst[i] = src[i];
  }
}

// ---------------------------------------------------------------------------------------------
// Paging (liodom_map_evict / liodom_map_merge_state; no counterpart in the reference): the device map as a window onto a larger
// map the caller keeps on the host.  Evict = prune whose dropped cells come out as a blob first; merge = import that appends to
// the cells already there.  Not on the per-scan path: a map that never calls those entry points launches none of this and
// allocates nothing for it.  Order is stream order, as for prune.
// ---------------------------------------------------------------------------------------------
// Evict, step 1 (one workgroup, read-only on the map): keep flags with the keep box of k_map_prune_plan, then the chunked scan of
// k_map_pack_plan over the DROPPED cells — rank among the dropped and exclusive prefix of their counts — so any number of cells.
// Writes the dropped cells' records behind the header in `head` (relative creation order, `first` recomputed), the header counts
// where the host reads them (status 0: a tile has no history), and each record's source cell id into `src` (the prune scratch,
// which the prune that follows overwrites only after the pack has read it: stream order).
__global__ __launch_bounds__(1024) void k_map_evict_plan(MapView m, const double* T_ptr, int keep_xy, int keep_z, unsigned char* head, int* src) {
  __shared__ int sh_wr[16];
  __shared__ int sh_wc[16];
  __shared__ int sh_rank;
  __shared__ long long sh_carry;
  const MapState& st = *m.st;
  const int tid = threadIdx.x;
  const int nc = max(0, min(st.n_cells, m.max_cells));
  const MapKeepBox box = map_keep_box(m, T_ptr, keep_xy, keep_z);
  MapStateRecord* rec = reinterpret_cast<MapStateRecord*>(head + kMapStateHeaderBytes);
  if (tid == 0) { sh_carry = 0; sh_rank = 0; }
  __syncthreads();
  for (int base = 0; base < nc; base += 1024) {
    const int c = base + tid;
    int key[3] = {0, 0, 0}, drop = 0, cnt = 0;
    if (c < nc) {
      for (int a = 0; a < 3; a++) key[a] = m.cell_key[c * 3 + a];
      drop = map_keep_cell(box, key) ^ 1;
      cnt = drop ? max(0, min(m.cell_n[c], m.cell_cap)) : 0;
    }
    int ir = drop, ic = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      const int tr = __shfl_up(ir, off), tc = __shfl_up(ic, off);
      if ((tid & 63) >= off) { ir += tr; ic += tc; }
    }
    if ((tid & 63) == 63) { sh_wr[tid >> 6] = ir; sh_wc[tid >> 6] = ic; }
    __syncthreads();
    int j = sh_rank + ir - drop;
    long long run = sh_carry + (ic - cnt);
    for (int q = 0; q < (tid >> 6); q++) { j += sh_wr[q]; run += sh_wc[q]; }
    if (drop) {                       // j < nc <= max_cells: inside `head` and `src`
      MapStateRecord r;
      for (int a = 0; a < 3; a++) { r.key[a] = key[a]; r.corner_leaf[a] = m.cell_org[c * 3 + a] + kMapLeafMargin; }
      r.count = cnt;
      r.first = (int)run;
      rec[j] = r;
      src[j] = c;
    }
    __syncthreads();
    if (tid == 1023) { sh_rank = j + drop; sh_carry = run + cnt; }
    __syncthreads();
  }
  if (tid == 0) {
    MapStateHeader* hd = reinterpret_cast<MapStateHeader*>(head);
    hd->n_cells = sh_rank;
    hd->status = 0u;
    hd->n_points = sh_carry;
  }
}

// Evict, step 2, grid (chunk, record): k_map_pack for records that name their source cell — gathers each dropped cell's CURRENT
// slab into the point section, one 16-byte load and one 16-byte store per point, consecutive lanes on consecutive points.
__global__ __launch_bounds__(256) void k_map_evict_pack(MapView m, const unsigned char* head, const int* src, float4* pts, int pts_cap) {
  const MapStateHeader* hd = reinterpret_cast<const MapStateHeader*>(head);
  const MapStateRecord* rec = reinterpret_cast<const MapStateRecord*>(head + kMapStateHeaderBytes);
  const int nr = max(0, min(hd->n_cells, m.max_cells));
  for (int j = blockIdx.y; j < nr; j += gridDim.y) {
    const int c = src[j];
    if (c < 0 || c >= m.max_cells) continue;
    const int first = rec[j].first, cnt = min(rec[j].count, m.cell_cap);
    const float4* from = map_cell_cur(m, c);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
      const long long o = (long long)first + i;
      if (o >= 0 && o < pts_cap) pts[o] = from[i];
    }
  }
}

// Entry [0] of the merge scratch is the host's; the blob cells' ranks follow from entry [4] on.
struct MapMergeInfo { int n_taken, n_before, pad0, pad1; };

// Merge, step 1 (one workgroup, read-only on the map).  Every blob key is looked up through map_hash / the linear probe; a key
// that is a cell of the map (a slot whose cslot_cell is an id in [0, n_cells)) is skipped, every other one is taken.  rank[i] =
// rank among the taken cells, or -1; the chunked scan again, so any number of blob cells.  info = {taken, cells of the map}.
__global__ __launch_bounds__(1024) void k_map_merge_plan(MapView m, const unsigned char* head, int n_blob, MapMergeInfo* info, int* rank) {
  __shared__ int sh_w[16];
  __shared__ int sh_carry;
  const int tid = threadIdx.x;
  const int nc = max(0, min(m.st->n_cells, m.max_cells));
  const MapStateRecord* rec = reinterpret_cast<const MapStateRecord*>(head + kMapStateHeaderBytes);
  const int nb = max(0, min(n_blob, m.max_cells));
  if (tid == 0) sh_carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + tid;
    int take = 0;
    if (i < nb) {
      const int id = map_find_cell(m, rec[i].key[0], rec[i].key[1], rec[i].key[2]);
      take = (id >= 0 && id < nc) ? 0 : 1;
    }
    int incl = take;
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if ((tid & 63) >= off) incl += t; }
    if ((tid & 63) == 63) sh_w[tid >> 6] = incl;
    __syncthreads();
    int j = sh_carry + incl - take;
    for (int q = 0; q < (tid >> 6); q++) j += sh_w[q];
    if (i < nb) rank[i] = take ? j : -1;
    __syncthreads();
    if (tid == 1023) sh_carry = j + take;
    __syncthreads();
  }
  if (tid == 0) { MapMergeInfo o; o.n_taken = sh_carry; o.n_before = nc; o.pad0 = 0; o.pad1 = 0; *info = o; }
}

// Merge, step 2, grid (chunk, blob cell), launched only when the taken cells fit (the host has read `info`).  Taken cell i gets id
// n_before + rank[i].  Its key claims a hash slot as in k_map_unpack — the taken keys are distinct among themselves (the host's
// map_state_validate) and none is a cell of the map, so the slots are claimed in parallel.  A taken key can already SIT in the
// hash without being a cell: k_map_assign leaves such slots behind when one update creates more than kMapNewCellsMax cells
// (cslot_cell stays -1) or when the map is full (cslot_cell = max_cells, "no room").  The probe stops at that slot and takes it
// over, so every later lookup finds the merged cell.  ("No room" while the map has free ids is unreachable — the marker is only
// written when n_cells reaches max_cells, and everything that lowers n_cells rebuilds the hash — but the take-over covers it as
// well.)  cfirst is only read for slots an update creates itself and is left alone.
// cell_buf = 0 and mod_of_cell = -1 are written explicitly: ids >= n_cells hold whatever the cells pruned away left there.
// The points go into slab 0 of the new id.  One thread bumps n_cells and ORs the blob's status; nothing here reads n_cells.
__global__ __launch_bounds__(256) void k_map_merge(MapView m, const unsigned char* head, const float4* pts, int n_blob, int n_points,
                                                   const MapMergeInfo* info, const int* rank, int status) {
  const MapStateRecord* rec = reinterpret_cast<const MapStateRecord*>(head + kMapStateHeaderBytes);
  const int nb = max(0, min(n_blob, m.max_cells));
  const int base = info->n_before, n_taken = info->n_taken;
  if (base < 0 || n_taken < 0 || base + n_taken > m.max_cells) return;       // (the host does not launch this then)
  const unsigned int mask = (unsigned int)m.ctable - 1u;
  const int nthreads = gridDim.x * gridDim.y * 256;
  for (int i = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < nb; i += nthreads) {
    const int r = rank[i];
    if (r < 0 || r >= n_taken) continue;
    const int id = base + r;
    const MapStateRecord rc = rec[i];
    unsigned long long key;
    if (map_pack_key(rc.key[0], rc.key[1], rc.key[2], &key)) {
      unsigned int h = map_hash(key, mask);
      for (int probe = 0; probe < m.ctable; probe++) {
        const unsigned long long prev = atomicCAS(&m.ckey[h], kMapEmptyKey, key);
        if (prev == kMapEmptyKey || prev == key) { m.cslot_cell[h] = id; break; }
        h = (h + 1) & mask;
      }
    }
    for (int a = 0; a < 3; a++) {
      m.cell_key[id * 3 + a] = rc.key[a];
      m.cell_org[id * 3 + a] = (int)((unsigned int)rc.corner_leaf[a] - (unsigned int)kMapLeafMargin);
    }
    m.cell_n[id] = max(0, min(rc.count, m.cell_cap));
    m.cell_buf[id] = 0;
    m.mod_of_cell[id] = -1;
  }
  for (int i = blockIdx.y; i < nb; i += gridDim.y) {
    const int r = rank[i];
    if (r < 0 || r >= n_taken) continue;
    const int first = rec[i].first, cnt = min(rec[i].count, m.cell_cap);
    float4* dst = m.slab + (size_t)(base + r) * m.cell_cap;          // slab 0
    for (int k = blockIdx.x * 256 + threadIdx.x; k < cnt; k += gridDim.x * 256) {
      const long long o = (long long)first + k;
      if (o >= 0 && o < n_points) dst[k] = pts[o];
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { m.st->n_cells = base + n_taken; if (status) atomicOr(&m.st->status, status); }
}

}  // namespace liodom_dev

#include "kernels_reloc.h"
#include "kernels_reloc_bnb.h"
#include "kernels_map_hits.h"
#include "kernels_register.h"
