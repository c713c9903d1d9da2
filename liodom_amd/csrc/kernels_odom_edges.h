// kernels_odom_edges.h — k_odom_edges: the measured relative pose Z and the information Omega of odometry intervals of one stream,
// chained from the per-scan covariance records (contract: include/liodom_hip.h "odometry edges from the scans' own covariances";
// the arithmetic: liodom_math.h "Odometry edges from the scans' covariances"; host side: liodom_chain_odometry_edges and
// liodom_get_odometry_edges in liodom_hip.hip, odom_edges.h).  A header of its own, like kernels_graph.h.
// =============================================================================================
// k_odom_edges: one 64-thread workgroup (one wave) per interval, grid (n).  poses: 7 doubles per scan, recs: one
//   liodom_pose_cov_t (944 bytes) per scan, entry k is scan k — host-checked: 0 <= from[i] < to[i] < the entries behind both
//   pointers.  Lane l takes the scans k = l (mod 64) of a + 1 .. b in ascending order (odom_lane_partial: the kernel's one loop,
//   at most ceil((b - a) / 64) rounds) and keeps the 21 lower-triangle sums of its M_k and three counts in registers.  The 64
//   partials are combined by wave_reduce_scatter32_f64 (wave_ops.h: v_permlane32_swap, v_permlane16_swap, three DPP row steps,
//   one DPP add — a fixed tree, restated as odom_combine64), which leaves entry e in lanes 2 e and 2 e + 1; v_readlane hands
//   the 24 totals to the wave as scalars.  Lane 0 forms Z, B, Sigma_e and Omega (odom_edge_finish) into 656 bytes of LDS — the
//   one use of LDS: 82 words written by one lane, read once by all, no bank question arises — and the wave stores the record as
//   8-byte words, lane l words l and l + 64.  No atomics, no polling, no scalar memory writes; FP64 throughout, no contraction
//   (the library is built with -ffp-contract=off): the bytes equal odom_edge_host's.
//   Occupancy is not what bounds it: a launch is n waves of a few hundred FP64 instructions on one lane each, and its cost is
//   the launch and the 944-byte strided record reads (288 of them used).  profiles/odom_edges_kernel_resources.txt has the
//   registers and scratch.
// =============================================================================================
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/liodom_hip.h"
#include "liodom_math.h"
#include "wave_ops.h"

namespace liodom_dev {

static_assert(sizeof(liodom_pose_cov_t) == 944, "k_odom_edges reads 944-byte records");
static_assert(sizeof(liodom_odom_edge_t) == 8 * kOdomEdgeWords, "the record is stored as 82 8-byte words");
static_assert(kOdomAccN <= 32, "the accumulator goes through wave_reduce_scatter32_f64");

__device__ __forceinline__ double readlane_f64(double v, int lane /*a constant*/) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)b, lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(64) void k_odom_edges(const double* __restrict__ poses, const liodom_pose_cov_t* __restrict__ recs,
                                                   const int* __restrict__ from, const int* __restrict__ to, int n, double inflation,
                                                   double fr2, double ft2, liodom_odom_edge_t* __restrict__ out) {
  const int row = (int)blockIdx.x;
  if (row >= n) return;
  const int lane = (int)threadIdx.x;
  const int a = from[row], b = to[row];
  __shared__ unsigned long long words[kOdomEdgeWords];
  double acc[32];
  odom_lane_partial(poses, recs, a, b, lane, inflation, fr2, ft2, acc);
#pragma unroll
  for (int e = kOdomAccN; e < 32; e++) acc[e] = 0.0;
  const double mine = wave_reduce_scatter32_f64(acc);      // entry e's total in lanes 2 e and 2 e + 1
  double tot[kOdomAccN];
#pragma unroll
  for (int e = 0; e < kOdomAccN; e++) tot[e] = readlane_f64(mine, 2 * e);
  if (lane == 0) odom_edge_finish(poses + (size_t)a * 7, poses + (size_t)b * 7, a, b, tot, words);
  __syncthreads();
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(out + row);
  dst[lane] = words[lane];
  if (lane + 64 < kOdomEdgeWords) dst[lane + 64] = words[lane + 64];
}

}  // namespace liodom_dev
