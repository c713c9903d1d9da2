// kernels_register.h — liodom_map_register_poses (contract: include/liodom_hip.h "registering a scan to the map"; plain-C++ half:
// map_register.h; host entry point: liodom_map_host.h).  Included at the end of liodom_map.h.  No counterpart in the reference.
// Nothing of the map is written: both kernels work on the map's registration workspace, which k_map_local_rows has filled with
// the rows' local maps.
// =============================================================================================
// k_map_register_grid: one 256-thread workgroup per row builds a uniform 1 m grid over the row's cloud.
//   Voxel of a point: floorf of its float coordinates, packed as map_pack_key packs a cell key (+-2^20; a point beyond, or a
//   non-finite one, is left out: slot -1).  Open-addressing table of table_size(n) >= 2 n slots (map_register.h), so an insert
//   always finds a slot within `table` probes.  Count -> exclusive scan -> fill -> every voxel's run of `order` sorted ascending:
//   what a stable fill leaves (points of a voxel in row order).  Atomics on global memory are used here only, inside one
//   workgroup's own row; every loop is bounded by n or the table size.
// k_map_register: one 256-thread workgroup per start pose; every pass and every LM iteration inside the launch.
//   search   lanes run over the edges (plain cached loads); the query is transform_point(T(q, t), e); the 27 voxels around it are
//            looked up and their points kept in a top-5 in registers ordered by (distance, index) — the order orc.knn5(mode 0)
//            gives.  A point outside the 27 voxels differs from the query by more than 1 in one coordinate, so its float squared
//            distance is >= 1.0f: whenever the fifth neighbour passes `d[4] < 1.0f` the five are the exact five; fewer than five
//            inside means invalid, as the oracle decides.  The gate (line_gate) runs per lane; (a, b) or (-1, -1) goes to the
//            workspace, so the LM iterations of a pass do not search again (a lane reads back what it wrote itself).
//   solve    residual_accumulate per lane, the kAccN sums reduced in registers per wave (wave_reduce_scatter32_f64) and through
//            LDS across the four waves in wave order; thread 0 runs lm_begin / lm_update and publishes the candidate's matrix
//            through LDS behind a workgroup barrier, as k_lm_solve's controller does.
//   No cross-workgroup communication, no flag polling, no atomics on global memory; the only waits are __syncthreads, all in
//   uniform control flow.  Loop bounds: max_passes <= 16, kLmMaxIterations evaluations, 27 voxels, the table size, a voxel's count.
// =============================================================================================
#pragma once
#include "map_register.h"
#include "wave_ops.h"

namespace liodom_dev {

constexpr int kRegThreads = 256;
constexpr int kRegWaves = kRegThreads / 64;

struct RegisterView {
  const double* pose;            // [rows][8] start pose, quaternion normalised
  const int* count;              // [rows] points of the row's local map
  const float4* pts;             // [rows][local_cap]
  int* order;                    // [rows][local_cap]
  int* slot;                     // [rows][local_cap]
  unsigned long long* key;       // [rows][table]
  int* first;                    // [rows][table]
  int* fill;                     // [rows][table]
  int2* corr;                    // [rows][edge_cap]
  liodom_map_registration_t* out;
  const float4* edges;
  int n_edges, local_cap, edge_cap;
  long long table;               // slots per row of the allocation
  int max_passes, min_matches;
  double stop_t, stop_r, min_range, max_range;
};

__device__ __forceinline__ int reg_row_points(const RegisterView& v, int row) {
  const int n = v.count[row];
  return n < 0 ? 0 : (n > v.local_cap ? v.local_cap : n);
}
__device__ __forceinline__ int reg_table_size(int n) {      // map_register_table_size
  long long t = kRegisterTableMin;
  for (int i = 0; i < 32 && t < 2ll * n; i++) t <<= 1;
  return (int)t;
}
// voxel of a point; false: non-finite or beyond +-2^20
__device__ __forceinline__ bool reg_voxel(float x, float y, float z, int* vx, int* vy, int* vz) {
  const float B = 1048576.0f;
  if (!(fabsf(x) < B) || !(fabsf(y) < B) || !(fabsf(z) < B)) return false;
  *vx = (int)floorf(x); *vy = (int)floorf(y); *vz = (int)floorf(z);
  return true;
}

__global__ __launch_bounds__(kRegThreads) void k_map_register_grid(RegisterView v) {
  __shared__ int sh_w[kRegWaves];
  __shared__ int sh_base;
  const int tid = (int)threadIdx.x, row = (int)blockIdx.x;
  const int n = reg_row_points(v, row);
  const int ts = reg_table_size(n);
  const unsigned int mask = (unsigned int)ts - 1u;
  const float4* pts = v.pts + (size_t)row * v.local_cap;
  int* order = v.order + (size_t)row * v.local_cap;
  int* slot = v.slot + (size_t)row * v.local_cap;
  unsigned long long* key = v.key + (size_t)row * v.table;
  int* first = v.first + (size_t)row * v.table;
  int* fill = v.fill + (size_t)row * v.table;
  for (int s = tid; s < ts; s += kRegThreads) { key[s] = kMapEmptyKey; fill[s] = 0; }
  if (tid == 0) sh_base = 0;
  __syncthreads();
  // count
  for (int i = tid; i < n; i += kRegThreads) {
    const float4 p = pts[i];
    int vx, vy, vz, found = -1;
    unsigned long long k;
    if (reg_voxel(p.x, p.y, p.z, &vx, &vy, &vz) && map_pack_key(vx, vy, vz, &k)) {
      unsigned int h = map_hash(k, mask);
      for (int probe = 0; probe < ts; probe++) {
        const unsigned long long prev = atomicCAS(&key[h], kMapEmptyKey, k);
        if (prev == kMapEmptyKey || prev == k) { found = (int)h; break; }
        h = (h + 1) & mask;
      }
    }
    slot[i] = found;
    if (found >= 0) atomicAdd(&fill[found], 1);
  }
  __syncthreads();
  // exclusive scan of the counts, 256 slots at a time
  for (int base = 0; base < ts; base += kRegThreads) {
    const int s = base + tid;
    const int c = s < ts ? fill[s] : 0;
    const int inc = wave_incl_scan_i32(c);
    if ((tid & 63) == 63) sh_w[tid >> 6] = inc;
    __syncthreads();
    int o = sh_base + inc - c;
    for (int w = 0; w < (tid >> 6); w++) o += sh_w[w];
    if (s < ts) first[s] = o;
    __syncthreads();
    if (tid == kRegThreads - 1) sh_base = o + c;
    __syncthreads();
  }
  for (int s = tid; s < ts; s += kRegThreads) fill[s] = 0;
  __syncthreads();
  // fill
  for (int i = tid; i < n; i += kRegThreads) {
    const int s = slot[i];
    if (s >= 0) {
      const int pos = first[s] + atomicAdd(&fill[s], 1);
      if (pos >= 0 && pos < n) order[pos] = i;
    }
  }
  __syncthreads();
  // row order inside every voxel
  for (int s = tid; s < ts; s += kRegThreads) {
    const int c = fill[s], f = first[s];
    if (c < 2 || f < 0 || f + c > n) continue;
    for (int a = 1; a < c; a++) {
      const int x = order[f + a];
      int b = a - 1;
      while (b >= 0 && order[f + b] > x) { order[f + b + 1] = order[f + b]; b--; }
      order[f + b + 1] = x;
    }
  }
}

// the five nearest so far, ascending by (distance, index); empty places hold (+inf, INT_MAX)
struct RegTop5 { float d0, d1, d2, d3, d4; int i0, i1, i2, i3, i4; };
__device__ __forceinline__ bool reg_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }
#define LIODOM_REG_CSWAP(a, b)                                                  \
  if (reg_less(k.d##b, k.i##b, k.d##a, k.i##a)) {                               \
    const float td = k.d##a; k.d##a = k.d##b; k.d##b = td;                      \
    const int ti = k.i##a; k.i##a = k.i##b; k.i##b = ti;                        \
  }
__device__ __forceinline__ void reg_insert(RegTop5& k, float d, int i) {
  if (!reg_less(d, i, k.d4, k.i4)) return;
  k.d4 = d; k.i4 = i;
  LIODOM_REG_CSWAP(3, 4)
  LIODOM_REG_CSWAP(2, 3)
  LIODOM_REG_CSWAP(1, 2)
  LIODOM_REG_CSWAP(0, 1)
}
#undef LIODOM_REG_CSWAP

// One edge's correspondence under Rm: (a, b) into the row's cloud, or false.
__device__ __forceinline__ bool reg_match(const double* Rm, const float4 e, const float4* pts, const int* order, const unsigned long long* key,
                                          const int* first, const int* fill, int n, int ts, int* ia, int* ib) {
  float qx, qy, qz;
  transform_point(Rm, e.x, e.y, e.z, &qx, &qy, &qz);
  int vx, vy, vz;
  if (!reg_voxel(qx, qy, qz, &vx, &vy, &vz)) return false;
  const unsigned int mask = (unsigned int)ts - 1u;
  RegTop5 k;
  k.d0 = k.d1 = k.d2 = k.d3 = k.d4 = __builtin_inff();
  k.i0 = k.i1 = k.i2 = k.i3 = k.i4 = 0x7fffffff;
  for (int c = 0; c < 27; c++) {
    const int dx = c % 3 - 1, dy = (c / 3) % 3 - 1, dz = c / 9 - 1;
    unsigned long long want;
    if (!map_pack_key(vx + dx, vy + dy, vz + dz, &want)) continue;
    unsigned int h = map_hash(want, mask);
    int s = -1;
    for (int probe = 0; probe < ts; probe++) {
      const unsigned long long have = key[h];
      if (have == want) { s = (int)h; break; }
      if (have == kMapEmptyKey) break;
      h = (h + 1) & mask;
    }
    if (s < 0) continue;
    const int f = first[s], cnt = fill[s];
    if (f < 0 || cnt < 0 || f + cnt > n) continue;
    for (int j = 0; j < cnt; j++) {
      const int i = order[f + j];
      if (i < 0 || i >= n) continue;
      const float4 p = pts[i];
      reg_insert(k, sqdist_f(qx, qy, qz, p.x, p.y, p.z), i);
    }
  }
  if (k.i4 == 0x7fffffff || !(k.d4 < 1.0f)) return false;      // fewer than five, or the fifth not closer than 1 m (:324)
  const float4 p0 = pts[k.i0], p1 = pts[k.i1], p2 = pts[k.i2], p3 = pts[k.i3], p4 = pts[k.i4];
  const float nx[5] = {p0.x, p1.x, p2.x, p3.x, p4.x}, ny[5] = {p0.y, p1.y, p2.y, p3.y, p4.y}, nz[5] = {p0.z, p1.z, p2.z, p3.z, p4.z};
  if (!line_gate(nx, ny, nz)) return false;
  *ia = k.i0; *ib = k.i1;
  return true;
}

// The accumulator of the row's valid correspondences at the matrix in Rm_sh -> sh_acc[0 .. 31]; every thread takes part; ends
// behind a barrier.  Fixed order: deterministic.
__device__ __forceinline__ void reg_eval(const RegisterView& v, const float4* pts, const int2* corr, const double* Rm_sh, double* wsum, double* sh_acc) {
  const int tid = (int)threadIdx.x;
  double acc[32];
#pragma unroll
  for (int i = 0; i < 32; i++) acc[i] = 0.0;
  double Rm[12];
#pragma unroll
  for (int i = 0; i < 12; i++) Rm[i] = Rm_sh[i];
  for (int e = tid; e < v.n_edges; e += kRegThreads) {
    const int2 c = corr[e];
    if (c.x < 0) continue;
    const float4 P = v.edges[e], A = pts[c.x], B = pts[c.y];
    const double p[3] = {(double)P.x, (double)P.y, (double)P.z};
    const double a[3] = {(double)A.x, (double)A.y, (double)A.z};
    const double b[3] = {(double)B.x, (double)B.y, (double)B.z};
    residual_accumulate(Rm, p, a, b, v.min_range, v.max_range, acc);
  }
  const double x = wave_reduce_scatter32_f64(acc);
  if ((tid & 1) == 0) wsum[(tid >> 6) * 32 + ((tid & 63) >> 1)] = x;
  __syncthreads();
  if (tid < 32) sh_acc[tid] = ((wsum[tid] + wsum[32 + tid]) + wsum[64 + tid]) + wsum[96 + tid];
  __syncthreads();
}

__global__ __launch_bounds__(kRegThreads) void k_map_register(RegisterView v) {
  __shared__ LmState sh_lm;
  __shared__ double sh_q[4], sh_t[3], sh_Rm[12], sh_acc[32], sh_wsum[kRegWaves * 32];
  __shared__ double sh_cov[36], sh_evals[6], sh_evecs[36];
  __shared__ int sh_cnt[kRegWaves];
  __shared__ int sh_f, sh_end;
  __shared__ liodom_map_registration_t sh_out;
  static_assert(sizeof(liodom_map_registration_t) % 8 == 0, "record is copied as 8-byte words");
  const int tid = (int)threadIdx.x, row = (int)blockIdx.x;
  const int n = reg_row_points(v, row);
  const int ts = reg_table_size(n);
  const float4* pts = v.pts + (size_t)row * v.local_cap;
  const int* order = v.order + (size_t)row * v.local_cap;
  const unsigned long long* key = v.key + (size_t)row * v.table;
  const int* first = v.first + (size_t)row * v.table;
  const int* fill = v.fill + (size_t)row * v.table;
  int2* corr = v.corr + (size_t)row * v.edge_cap;
  if (tid == 0) {
    const double* p = v.pose + (size_t)row * 8;
    for (int k = 0; k < 4; k++) sh_q[k] = p[k];
    for (int k = 0; k < 3; k++) sh_t[k] = p[4 + k];
    sh_out.passes = 0; sh_out.matches = 0; sh_out.n_residuals = 0; sh_out.local_points = v.count[row];
    sh_out.last_move_t = 0.0; sh_out.last_move_r = 0.0;
    sh_out.last_lm.iterations = 0; sh_out.last_lm.accepted = 0; sh_out.last_lm.termination = 0; sh_out.last_lm.pad = 0;
    sh_out.last_lm.initial_cost = 0.0; sh_out.last_lm.final_cost = 0.0;
    sh_end = n == 0 ? LIODOM_REG_NO_MAP : -1;
    sh_f = LM_DONE;
  }
  if (n == 0) {
    for (int e = tid; e < v.n_edges; e += kRegThreads) corr[e] = make_int2(-1, -1);
  }
  __syncthreads();
  for (int pass = 0; pass < v.max_passes; pass++) {
    if (sh_end >= 0) break;                                   // (uniform: written before the barrier that ended the last pass)
    if (tid == 0) iso_from_qt(sh_q, sh_t, sh_Rm);
    __syncthreads();
    // ---- search
    int mine = 0;
    {
      double Rm[12];
#pragma unroll
      for (int i = 0; i < 12; i++) Rm[i] = sh_Rm[i];
      for (int e = tid; e < v.n_edges; e += kRegThreads) {
        int ia = -1, ib = -1;
        const bool ok = reg_match(Rm, v.edges[e], pts, order, key, first, fill, n, ts, &ia, &ib);
        corr[e] = ok ? make_int2(ia, ib) : make_int2(-1, -1);
        mine += ok ? 1 : 0;
      }
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((tid & 63) == 0) sh_cnt[tid >> 6] = mine;
    __syncthreads();
    const int nvalid = (sh_cnt[0] + sh_cnt[1]) + (sh_cnt[2] + sh_cnt[3]);
    if (nvalid < v.min_matches) {
      if (tid == 0) {
        sh_out.matches = nvalid; sh_end = LIODOM_REG_FEW_MATCHES;
        sh_out.last_lm.iterations = 0; sh_out.last_lm.accepted = 0; sh_out.last_lm.termination = 0;
        sh_out.last_lm.initial_cost = 0.0; sh_out.last_lm.final_cost = 0.0;
      }
      __syncthreads();
      continue;
    }
    // ---- one LM solve from (q, t)
    reg_eval(v, pts, corr, sh_Rm, sh_wsum, sh_acc);
    if (tid == 0) {
      const int f = lm_begin(sh_lm, sh_q, sh_t, sh_acc, nvalid, 0);
      if (f == LM_NEED_EVAL) iso_from_qt(sh_lm.cand_q, sh_lm.cand_t, sh_Rm);
      sh_f = f;
    }
    __syncthreads();
    for (int step = 0; step < kLmMaxIterations; step++) {
      if (sh_f != LM_NEED_EVAL) break;                        // (uniform)
      reg_eval(v, pts, corr, sh_Rm, sh_wsum, sh_acc);
      if (tid == 0) {
        const int f = lm_update(sh_lm, sh_acc);
        if (f == LM_NEED_EVAL) iso_from_qt(sh_lm.cand_q, sh_lm.cand_t, sh_Rm);
        sh_f = f;
      }
      __syncthreads();
    }
    if (tid == 0) {
      sh_out.matches = nvalid;
      sh_out.last_lm.iterations = sh_lm.iter; sh_out.last_lm.accepted = sh_lm.accepted; sh_out.last_lm.termination = sh_lm.termination;
      sh_out.last_lm.initial_cost = sh_lm.initial_cost; sh_out.last_lm.final_cost = sh_lm.cost;
      if (sh_lm.termination == LM_TERM_EVAL_FAILURE) {
        sh_end = LIODOM_REG_EVAL_FAILURE;
      } else {
        double mt, mr;
        const bool conv = register_pass_converged(sh_q, sh_t, sh_lm.q, sh_lm.t, v.stop_t, v.stop_r, &mt, &mr);
        for (int k = 0; k < 4; k++) sh_q[k] = sh_lm.q[k];
        for (int k = 0; k < 3; k++) sh_t[k] = sh_lm.t[k];
        sh_out.passes = pass + 1; sh_out.last_move_t = mt; sh_out.last_move_r = mr;
        if (conv) sh_end = LIODOM_REG_CONVERGED;
        else if (pass + 1 >= v.max_passes) sh_end = LIODOM_REG_MAX_PASSES;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int end = sh_end < 0 ? LIODOM_REG_MAX_PASSES : sh_end;
    const bool taken = end == LIODOM_REG_CONVERGED || end == LIODOM_REG_MAX_PASSES;
    const bool failed = end == LIODOM_REG_EVAL_FAILURE;
    for (int k = 0; k < 4; k++) sh_out.pose[k] = sh_q[k];
    for (int k = 0; k < 3; k++) sh_out.pose[4 + k] = sh_t[k];
    sh_out.termination = end;
    sh_out.n_residuals = taken ? sh_out.matches : 0;
    sh_out.final_cost = taken ? sh_lm.cost : 0.0;
    sh_out.cov_flags = pose_cov_compute(sh_lm.H, sh_lm.cost, sh_out.matches, failed ? (int)LM_TERM_EVAL_FAILURE : sh_lm.termination,
                                        (taken || failed) ? 1 : 0, &sh_out.sigma2, sh_out.information, sh_cov, sh_evals, sh_evecs);
  }
  __syncthreads();
  constexpr int kWords = (int)(sizeof(liodom_map_registration_t) / 8);
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&sh_out);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(v.out + row);
  for (int i = tid; i < kWords; i += kRegThreads) dst[i] = src[i];
}

}  // namespace liodom_dev
