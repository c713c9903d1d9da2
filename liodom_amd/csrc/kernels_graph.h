// Closing loops (liodom_graph_*; no counterpart in the reference): a pose graph over key frames, linearised and solved on the
// device.  Included by liodom_hip.hip.  The arithmetic of one edge is liodom_math.h "Pose graph"; tests/graph_model.py restates
// everything here in NumPy (graph_robust_model.py the losses, graph_cov_model.py the covariances).  By subject:
//
//   edges     graph_load_edge     Xi, Xj, Z, Omega of one edge, for every kernel with a thread per edge
//             k_graph_linearize<ROBUST>   e, chi2, A^T Omega e, B^T Omega e, A^T Omega A, A^T Omega B, B^T Omega B.  Outputs are
//                       component-major (entry k of edge e at [k * edge_cap + e]): consecutive lanes store consecutive addresses.
//             k_graph_cost<ROBUST>        chi2 per edge at the candidate poses
//                       ROBUST = true where a graph has a loss on some edge's kind or an edge switched off: rho and w per edge as
//                       well.  ROBUST = false reads no code and no scale and writes no rho and no w.
//             k_graph_gate        the chi-square gate of a candidate edge (launched only by the covariance calls)
//   nodes     k_graph_gather      one thread per node over the CSR of its (edge, side) pairs, in CSR order: gradient, diagonal block,
//                       inverse of the damped block.  No atomics: a sum depends on the graph alone.
//             k_graph_multiply    y = (H + lambda diag H) x by node rows (graph_row_multiply: the row code of the PCG loop)
//             k_graph_retract / k_graph_sum   the candidate poses, and a sum in a fixed order
//   solving   graph_pcg_run       the whole preconditioned conjugate-gradient loop in ONE workgroup of 1024 threads: no workgroup
//                       waits for another, the host is not asked anything inside the loop.  The preconditioner is block-Jacobi in
//                       the coordinates of the odometry chain ("the preconditioner" below).  Its two callers:
//             k_graph_pcg         (H + lambda diag H) x = -g, the Levenberg-Marquardt step, with the exit on max |g|
//             k_graph_pcg_columns columns of H^-1, one workgroup per column (the covariance calls), and
//             k_graph_cov_gather  the 6 x 6 blocks of H^-1 picked out of them
//
// Fixed nodes: delta = 0; their rows and columns drop out (gradient 0, inverse block 0, skipped as a neighbour).  A free node
// without edges: its block counts as the identity, its gradient is 0, it stays where it is.
#pragma once

#include "graph_lm.h"
#include "liodom_math.h"
#include "wave_ops.h"

namespace liodom_dev {

constexpr int kGraphThreads = 256;          // the edge- and node-parallel kernels
constexpr int kGraphPcgThreads = 1024;      // the one workgroup of graph_pcg_run and k_graph_sum
constexpr int kGraphPcgWaves = kGraphPcgThreads / 64;

struct GraphPcgStatus {
  int iterations, flag;     // GRAPH_PCG_* (graph_lm.h)
  double gmax;              // max |g| over the free nodes (k_graph_pcg_columns: 0)
  double residual;          // |r| / |b| when the loop ended
};

// ---- edges ---------------------------------------------------------------------------------------------------------------------
// Edge e = (ei[e], ej[e], z, info): the poses of its two nodes, its measurement and its information matrix
__device__ __forceinline__ void graph_load_edge(long long e, const double* __restrict__ poses, const int* __restrict__ ei,
                                                const int* __restrict__ ej, const double* __restrict__ z, const double* __restrict__ info,
                                                double* Xi, double* Xj, double* Z, double* Om) {
  const double* pi = poses + 7ll * ei[e];
  const double* pj = poses + 7ll * ej[e];
#pragma unroll
  for (int k = 0; k < 7; k++) { Xi[k] = pi[k]; Xj[k] = pj[k]; Z[k] = z[7ll * e + k]; }
#pragma unroll
  for (int k = 0; k < 36; k++) Om[k] = info[36ll * e + k];
}

// ROBUST: code[e] is the edge's loss (kGraphLoss*) or kGraphLossInactive, scale[e] its c; the host derives both from the graph's
// table and flags.  Per edge: the raw s = e^T Omega e in chi2, rho(s) and w = rho'(s); w multiplies the finished entries of the
// five blocks at the store (graph_edge_blocks_t), so code 0 — or w = 1 — gives the quadratic instance's bytes.  An inactive
// edge: s, rho = w = 0, and nothing else — no node's list names it, its blocks are never read.
template <bool ROBUST>
__global__ __launch_bounds__(kGraphThreads) void k_graph_linearize(int n_edges, long long edge_cap, const double* __restrict__ poses,
                                                                   const int* __restrict__ ei, const int* __restrict__ ej,
                                                                   const double* __restrict__ z, const double* __restrict__ info,
                                                                   const int* __restrict__ code, const double* __restrict__ scale,
                                                                   double* __restrict__ chi2, double* __restrict__ rho,
                                                                   double* __restrict__ w, double* __restrict__ gi,
                                                                   double* __restrict__ gj, double* __restrict__ Hii,
                                                                   double* __restrict__ Hij, double* __restrict__ Hjj) {
  const int e = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (e >= n_edges) return;
  double Xi[7], Xj[7], Z[7], Om[36], err[6], A[36], B[36];
  graph_load_edge(e, poses, ei, ej, z, info, Xi, Xj, Z, Om);
  const int ce = ROBUST ? code[e] : kGraphLossNone;
  if (ROBUST && ce == kGraphLossInactive) {
    graph_edge_error(Xi, Xj, Z, err, nullptr, nullptr);
    chi2[e] = graph_edge_chi2(err, Om);
    rho[e] = 0.0; w[e] = 0.0;
    return;
  }
  graph_edge_error(Xi, Xj, Z, err, A, B);
  graph_edge_blocks_t<ROBUST>(err, A, B, Om, edge_cap, ce, ROBUST ? scale[e] : 0.0, chi2 + e, ROBUST ? rho + e : nullptr,
                              ROBUST ? w + e : nullptr, gi + e, gj + e, Hii + e, Hij + e, Hjj + e);
}

template <bool ROBUST>
__global__ __launch_bounds__(kGraphThreads) void k_graph_cost(int n_edges, const double* __restrict__ poses, const int* __restrict__ ei,
                                                              const int* __restrict__ ej, const double* __restrict__ z,
                                                              const double* __restrict__ info, const int* __restrict__ code,
                                                              const double* __restrict__ scale, double* __restrict__ chi2,
                                                              double* __restrict__ rho, double* __restrict__ w) {
  const int e = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (e >= n_edges) return;
  double Xi[7], Xj[7], Z[7], Om[36], err[6];
  graph_load_edge(e, poses, ei, ej, z, info, Xi, Xj, Z, Om);
  graph_edge_error(Xi, Xj, Z, err, nullptr, nullptr);
  const double s = graph_edge_chi2(err, Om);
  chi2[e] = s;
  if (ROBUST) {
    const int ce = code[e];
    double r = 0.0, wt = 0.0;
    if (ce != kGraphLossInactive) graph_loss(ce, scale[e], s, &r, &wt);
    rho[e] = r; w[e] = wt;
  }
}

// One thread per candidate edge c = (ci[c], cj[c], z, info): graph_gate (liodom_math.h) at the current poses with the blocks
// Sigma[i, i], Sigma[i, j], Sigma[j, j] at blocks[3 c], [3 c + 1], [3 c + 2].  flag[c] = 1 where Omega or S is not positive
// definite (d2[c] is then NaN), else 0.
__global__ __launch_bounds__(kGraphThreads) void k_graph_gate(int n, const double* __restrict__ poses, const int* __restrict__ ci,
                                                              const int* __restrict__ cj, const double* __restrict__ z,
                                                              const double* __restrict__ info, const double* __restrict__ blocks,
                                                              double* __restrict__ d2, int* __restrict__ flag) {
  const int c = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (c >= n) return;
  double Xi[7], Xj[7], Z[7], Om[36], Sii[36], Sij[36], Sjj[36];
  graph_load_edge(c, poses, ci, cj, z, info, Xi, Xj, Z, Om);
#pragma unroll
  for (int k = 0; k < 36; k++) { Sii[k] = blocks[108ll * c + k]; Sij[k] = blocks[108ll * c + 36 + k]; Sjj[k] = blocks[108ll * c + 72 + k]; }
  double d;
  const bool ok = graph_gate(Xi, Xj, Z, Om, Sii, Sij, Sjj, &d);
  d2[c] = d;
  flag[c] = ok ? 0 : 1;
}

// ---- nodes ---------------------------------------------------------------------------------------------------------------------
// g [n * 6 + k]; D and Minv component-major ([k * node_cap + n]).  Minv is the inverse of the node's damped preconditioner block:
// for a node on the chain (parent[n] >= 0: the edge (n - 1, n) it hangs on; graph_precondition below) the B^T Omega B of that
// edge, otherwise its diagonal block D.  *bad = 1 where a free node's damped block is not positive definite (every writer
// writes the same value).
__global__ __launch_bounds__(kGraphThreads) void k_graph_gather(int n_nodes, long long node_cap, long long edge_cap, double lambda,
                                                                const int* __restrict__ fixed, const int* __restrict__ parent,
                                                                const int* __restrict__ offsets,
                                                                const int* __restrict__ entries, const double* __restrict__ gi,
                                                                const double* __restrict__ gj, const double* __restrict__ Hii,
                                                                const double* __restrict__ Hjj, double* __restrict__ g,
                                                                double* __restrict__ D, double* __restrict__ Minv, int* __restrict__ bad) {
  const int n = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (n >= n_nodes) return;
  double gs[6], Ds[36], inv[36];
#pragma unroll
  for (int k = 0; k < 6; k++) gs[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 36; k++) { Ds[k] = 0.0; inv[k] = 0.0; }
  const int k0 = offsets[n], k1 = offsets[n + 1];
  for (int k = k0; k < k1; k++) {
    const int ent = entries[k];
    const long long e = ent >> 1;
    const double* gsrc = (ent & 1) ? gj : gi;
    const double* hsrc = (ent & 1) ? Hjj : Hii;
#pragma unroll
    for (int c = 0; c < 6; c++) gs[c] += gsrc[c * edge_cap + e];
#pragma unroll
    for (int c = 0; c < 36; c++) Ds[c] += hsrc[c * edge_cap + e];
  }
  const bool is_fixed = fixed[n] != 0;
  if (!is_fixed) {
    if (k1 == k0) {
#pragma unroll
      for (int k = 0; k < 6; k++) inv[k * 7] = 1.0;
    } else if (parent[n] >= 0) {
      double Bs[36];
      const long long e = parent[n];
#pragma unroll
      for (int c = 0; c < 36; c++) Bs[c] = Hjj[c * edge_cap + e];
      if (!graph_damped_inverse(Bs, lambda, inv)) *bad = 1;
    } else if (!graph_damped_inverse(Ds, lambda, inv)) {
      *bad = 1;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) g[6ll * n + k] = is_fixed ? 0.0 : gs[k];
#pragma unroll
  for (int k = 0; k < 36; k++) { D[k * node_cap + n] = Ds[k]; Minv[k * node_cap + n] = inv[k]; }
}

// Row n of y = (H + lambda diag H) x with the fixed rows and columns dropped; the neighbours in CSR order.
__device__ __forceinline__ void graph_row_multiply(int n, long long node_cap, long long edge_cap, double lambda, const int* __restrict__ fixed,
                                                   const int* __restrict__ offsets, const int* __restrict__ entries,
                                                   const int* __restrict__ ei, const int* __restrict__ ej, const double* __restrict__ D,
                                                   const double* __restrict__ Hij, const double* x, double* y) {
  if (fixed[n] != 0) {
#pragma unroll
    for (int r = 0; r < 6; r++) y[r] = 0.0;
    return;
  }
  double xn[6];
#pragma unroll
  for (int r = 0; r < 6; r++) xn[r] = x[6ll * n + r];
  const int k0 = offsets[n], k1 = offsets[n + 1];
  if (k1 == k0) {
#pragma unroll
    for (int r = 0; r < 6; r++) y[r] = xn[r];
    return;
  }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) s += D[(r * 6 + c) * node_cap + n] * xn[c];
    y[r] = s + lambda * D[(r * 7) * node_cap + n] * xn[r];
  }
  for (int k = k0; k < k1; k++) {
    const int ent = entries[k];
    const long long e = ent >> 1;
    const int o = (ent & 1) ? ei[e] : ej[e];
    if (fixed[o] != 0) continue;
    double xo[6];
#pragma unroll
    for (int c = 0; c < 6; c++) xo[c] = x[6ll * o + c];
    if (ent & 1) {               // n is the edge's j: Hij^T
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += Hij[(c * 6 + r) * edge_cap + e] * xo[c];
        y[r] += s;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += Hij[(r * 6 + c) * edge_cap + e] * xo[c];
        y[r] += s;
      }
    }
  }
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_multiply(int n_nodes, long long node_cap, long long edge_cap, double lambda,
                                                                  const int* __restrict__ fixed, const int* __restrict__ offsets,
                                                                  const int* __restrict__ entries, const int* __restrict__ ei,
                                                                  const int* __restrict__ ej, const double* __restrict__ D,
                                                                  const double* __restrict__ Hij, const double* __restrict__ x,
                                                                  double* __restrict__ y) {
  const int n = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (n >= n_nodes) return;
  double yr[6];
  graph_row_multiply(n, node_cap, edge_cap, lambda, fixed, offsets, entries, ei, ej, D, Hij, x, yr);
#pragma unroll
  for (int r = 0; r < 6; r++) y[6ll * n + r] = yr[r];
}

// cand = poses (+) delta for the free nodes, poses for the fixed ones
__global__ __launch_bounds__(kGraphThreads) void k_graph_retract(int n_nodes, const double* __restrict__ poses, const int* __restrict__ fixed,
                                                                 const double* __restrict__ delta, double* __restrict__ cand) {
  const int n = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (n >= n_nodes) return;
  double X[7], d[6], out[7];
#pragma unroll
  for (int k = 0; k < 7; k++) X[k] = poses[7ll * n + k];
#pragma unroll
  for (int k = 0; k < 6; k++) d[k] = delta[6ll * n + k];
  if (fixed[n] != 0) {
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = X[k];
  } else {
    graph_retract(X, d, out);
  }
#pragma unroll
  for (int k = 0; k < 7; k++) cand[7ll * n + k] = out[k];
}

// Sum over the wave in a fixed order (DPP within a row of 16 lanes, v_permlane16_swap and v_permlane32_swap across); every lane
// active, every lane gets the result.
__device__ __forceinline__ double graph_wave_sum(double x) {
  x = row_sum_f64(x);
  x += __longlong_as_double((long long)xor16_u64((unsigned long long)__double_as_longlong(x)));
  x += __longlong_as_double((long long)xor32_u64((unsigned long long)__double_as_longlong(x)));
  return x;
}
// Sums of K values over the workgroup of kGraphPcgThreads threads: per wave as above, the 16 wave sums through the LDS, added by
// every thread in wave order.  One barrier; `lds` (16 * K doubles) must not be written again before another barrier has passed.
template <int K>
__device__ __forceinline__ void graph_block_sum(double (&v)[K], double* lds) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < K; k++) {
    v[k] = graph_wave_sum(v[k]);
    if (lane == 0) lds[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kGraphPcgWaves; w++) s += lds[w * K + k];
    v[k] = s;
  }
}

// *out = in[0] + ... + in[n - 1], one workgroup: thread t adds entries t, t + 1024, ... in ascending order, then graph_block_sum
__global__ __launch_bounds__(kGraphPcgThreads) void k_graph_sum(int n, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double sh[kGraphPcgWaves];
  double s[1] = {0.0};
  for (int i = (int)threadIdx.x; i < n; i += kGraphPcgThreads) s[0] += in[i];
  graph_block_sum<1>(s, sh);
  if (threadIdx.x == 0) *out = s[0];
}

// ---- the preconditioner -------------------------------------------------------------------------------------------------------
// Block-Jacobi alone does not hold on a chain of poses: the chain is an elastic rod, its H has bending modes with eigenvalues ~ k^4,
// and a ring of 257 key frames needs three times its unknowns in iterations.  The chain's own coordinates mend
// that.  Node n HANGS ON node n - 1 if it is free and the graph has an edge (n - 1, n) (parent[n]: the first such edge; -1: a
// ROOT — a fixed node, a node without that edge, node 0).  A run of nodes from a root to the last node hanging on it is a segment.
// Let xi_k = (a_k, b_k) move node k AND everything after it in its segment rigidly about t_k: delta_n = sum over k <= n of
// (a_k, b_k + 2 a_k x (t_n - t_k)) (a rotation increment a is the half angle: the rotation vector is 2 a).  In these coordinates
// an edge (k - 1, k) sees xi_k alone — a rigid motion of both its nodes changes nothing — so the chain's part of S^T H S is
// block diagonal with the blocks B^T Omega B of those edges, and
//   M^-1 = S Binv S^T,   Binv_k = (damped block of parent[k], or of D_k for a free root, 0 for a fixed one)^-1   (k_graph_gather)
// is symmetric positive definite whatever else the graph holds; loop edges are what is left for the iterations.  A graph without
// such edges has only roots: S = I and this is block-Jacobi.
//   S^T r:  w_k = (Q1 + 2 Q3 - 2 t_k x Q2,  Q2),  Q1, Q2, Q3 = sums over n >= k of r^d_n, r^t_n, t_n x r^t_n       (suffix sums)
//   S y:    z_n = (P1,  P2 + 2 P1 x t_n - 2 P3),  P1, P2, P3 = sums over k <= n of a_k, b_k, a_k x t_k             (prefix sums)
// Both are segmented scans of 9 doubles over the nodes in a fixed order: thread t takes the nodes [t c, (t + 1) c), c =
// ceil(N / 1024), sums them, the 1024 sums are scanned per wave (six shuffle steps) and across the 16 waves through the LDS, and
// the thread walks its nodes again from what came before it.
__device__ __forceinline__ void graph_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// In: this thread's sum v and whether its nodes hold a segment boundary (f).  Out in v: what the threads before it (REV: after
// it) add to its first node — the sums since the last boundary.  One barrier; lds_v (16 * 9) and lds_f (16) as graph_block_sum's.
template <bool REV>
__device__ __forceinline__ void graph_block_segscan(double (&v)[9], bool f, double* lds_v, int* lds_f) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int ll = REV ? 63 - lane : lane, lw = REV ? kGraphPcgWaves - 1 - wave : wave;      // place in scan order
  int fi = f ? 1 : 0;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {                      // inclusive over the wave
    const int src = REV ? lane + off : lane - off;
    const int of = __shfl(fi, src & 63, 64);
    double ov[9];
#pragma unroll
    for (int k = 0; k < 9; k++) ov[k] = __shfl(v[k], src & 63, 64);
    if (ll >= off) {
      if (!fi) {
#pragma unroll
        for (int k = 0; k < 9; k++) v[k] = ov[k] + v[k];
      }
      fi |= of;
    }
  }
  if (ll == 63) {
#pragma unroll
    for (int k = 0; k < 9; k++) lds_v[lw * 9 + k] = v[k];
    lds_f[lw] = fi;
  }
  // exclusive: the inclusive value of the lane before
  const int prev = REV ? lane + 1 : lane - 1;
  const int ef = __shfl(fi, prev & 63, 64);
  double ev[9];
#pragma unroll
  for (int k = 0; k < 9; k++) ev[k] = __shfl(v[k], prev & 63, 64);
  __syncthreads();
  double cv[9];
#pragma unroll
  for (int k = 0; k < 9; k++) cv[k] = 0.0;
  for (int w = 0; w < lw; w++) {                                // the waves before this one, in order
    const bool wf = lds_f[w] != 0;
#pragma unroll
    for (int k = 0; k < 9; k++) cv[k] = wf ? lds_v[w * 9 + k] : cv[k] + lds_v[w * 9 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = ll == 0 ? cv[k] : (ef ? ev[k] : cv[k] + ev[k]);
}

// The LDS of one PCG workgroup: the sums of graph_block_sum<1> and <2> and of the two scans of the preconditioner
struct GraphPcgLds {
  double a[kGraphPcgWaves], b[kGraphPcgWaves * 2], v1[kGraphPcgWaves * 9], v2[kGraphPcgWaves * 9];
  int f1[kGraphPcgWaves], f2[kGraphPcgWaves];
};

// z = M^-1 r (above).  Every thread of the workgroup calls it; it begins and ends with a barrier, so r may have been written by
// any thread before and z may be read by any thread after.  z doubles as the store of Binv S^T r between the two scans.
__device__ __forceinline__ void graph_precondition(int n_nodes, long long node_cap, const int* __restrict__ parent,
                                                   const double* __restrict__ poses, const double* __restrict__ Minv, const double* r,
                                                   double* z, GraphPcgLds* lds) {
  __syncthreads();
  const int c = (n_nodes + kGraphPcgThreads - 1) / kGraphPcgThreads;
  const int lo = min(n_nodes, (int)threadIdx.x * c), hi = min(n_nodes, lo + c);
  double q[9];
  // S^T: suffix sums.  Node n is the last of its segment if the next node is a root.
  for (int pass = 0; pass < 2; pass++) {
    bool f = false;
    if (pass == 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) q[k] = 0.0;
    }
    for (int n = hi - 1; n >= lo; n--) {
      if (n == n_nodes - 1 || parent[n + 1] < 0) {
        f = true;
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = 0.0;
      }
      double rn[6], t[3], x3[3];
#pragma unroll
      for (int k = 0; k < 6; k++) rn[k] = r[6ll * n + k];
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = poses[7ll * n + 4 + k];
      graph_cross(t, rn + 3, x3);
#pragma unroll
      for (int k = 0; k < 3; k++) { q[k] += rn[k]; q[3 + k] += rn[3 + k]; q[6 + k] += x3[k]; }
      if (pass == 1) {
        double w[6], y[6];
        graph_cross(t, q + 3, x3);
#pragma unroll
        for (int k = 0; k < 3; k++) { w[k] = q[k] + 2.0 * q[6 + k] - 2.0 * x3[k]; w[3 + k] = q[3 + k]; }
#pragma unroll
        for (int a = 0; a < 6; a++) {
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < 6; b++) s += Minv[(a * 6 + b) * node_cap + n] * w[b];
          y[a] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; k++) z[6ll * n + k] = y[k];
      }
    }
    if (pass == 0) graph_block_segscan<true>(q, f, lds->v1, lds->f1);
  }
  // S: prefix sums.  A root begins its segment.
  for (int pass = 0; pass < 2; pass++) {
    bool f = false;
    if (pass == 0) {
#pragma unroll
      for (int k = 0; k < 9; k++) q[k] = 0.0;
    }
    for (int n = lo; n < hi; n++) {
      if (parent[n] < 0) {
        f = true;
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = 0.0;
      }
      double y[6], t[3], x3[3];
#pragma unroll
      for (int k = 0; k < 6; k++) y[k] = z[6ll * n + k];
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = poses[7ll * n + 4 + k];
      graph_cross(y, t, x3);
#pragma unroll
      for (int k = 0; k < 3; k++) { q[k] += y[k]; q[3 + k] += y[3 + k]; q[6 + k] += x3[k]; }
      if (pass == 1) {
        graph_cross(q, t, x3);
#pragma unroll
        for (int k = 0; k < 3; k++) { z[6ll * n + k] = q[k]; z[6ll * n + 3 + k] = q[3 + k] + 2.0 * x3[k] - 2.0 * q[6 + k]; }
      }
    }
    if (pass == 0) graph_block_segscan<false>(q, f, lds->v2, lds->f2);
  }
  __syncthreads();
}

// ---- solving --------------------------------------------------------------------------------------------------------------------
// Preconditioned conjugate gradients for (H + lambda diag H) x = b, one workgroup; every thread calls it with x = 0, r = b and
// z = M^-1 r in place (the caller's graph_precondition has ended with its barrier).  Thread t owns nodes t, t + 1024, ...: it
// alone reads and writes their entries of x, r and Ap; p — read across nodes by the row product — and r and z around the
// preconditioner need barriers.  Per iteration: p visible; p^T A p; the preconditioner's four; (r^T r, r^T z).  The vectors live
// in global memory ([n * 6 + k]).  Ends with |r| <= tolerance |b| (converged), after max_iterations, or at p^T A p <= 0 or a
// block that is not positive definite (breakdown; x is then what the iterations before had).  gradient_exit: nothing is solved.
// Returns the status with gmax = 0.
__device__ __forceinline__ GraphPcgStatus graph_pcg_run(int n_nodes, long long node_cap, long long edge_cap, double lambda, int max_iterations,
                                                        double tolerance, bool gradient_exit, const int* __restrict__ fixed,
                                                        const int* __restrict__ parent, const double* __restrict__ poses,
                                                        const int* __restrict__ offsets, const int* __restrict__ entries,
                                                        const int* __restrict__ ei, const int* __restrict__ ej, const double* __restrict__ D,
                                                        const double* __restrict__ Minv, const double* __restrict__ Hij,
                                                        const int* __restrict__ bad, double* x, double* r, double* p, double* zv, double* Ap,
                                                        GraphPcgLds* lds) {
  const int tid = (int)threadIdx.x;
  double s2[2] = {0.0, 0.0};
  for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double rk = r[6ll * n + k], zk = zv[6ll * n + k];
      p[6ll * n + k] = zk;
      s2[0] += rk * rk; s2[1] += rk * zk;
    }
  }
  graph_block_sum<2>(s2, lds->b);
  const double g2 = s2[0];
  double rz = s2[1], rr = s2[0];
  int iterations = 0, flag = GRAPH_PCG_MAX_ITER;
  if (gradient_exit) flag = GRAPH_PCG_GRADIENT;
  else if (*bad != 0 || !(g2 > 0.0) || !ld_isfinite(g2) || !(rz > 0.0)) flag = GRAPH_PCG_BREAKDOWN;
  else {
    for (int it = 0; it < max_iterations; it++) {
      __syncthreads();                               // p of every node is written
      double s1[1] = {0.0};
      for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
        double y[6];
        graph_row_multiply(n, node_cap, edge_cap, lambda, fixed, offsets, entries, ei, ej, D, Hij, p, y);
#pragma unroll
        for (int k = 0; k < 6; k++) { Ap[6ll * n + k] = y[k]; s1[0] += p[6ll * n + k] * y[k]; }
      }
      graph_block_sum<1>(s1, lds->a);
      const double pAp = s1[0];
      if (!(pAp > 0.0) || !ld_isfinite(pAp)) { flag = GRAPH_PCG_BREAKDOWN; break; }
      const double alpha = rz / pAp;
      for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
        for (int k = 0; k < 6; k++) {
          x[6ll * n + k] += alpha * p[6ll * n + k];
          r[6ll * n + k] -= alpha * Ap[6ll * n + k];
        }
      }
      graph_precondition(n_nodes, node_cap, parent, poses, Minv, r, zv, lds);
      s2[0] = 0.0; s2[1] = 0.0;
      for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
        for (int k = 0; k < 6; k++) { const double rk = r[6ll * n + k]; s2[0] += rk * rk; s2[1] += rk * zv[6ll * n + k]; }
      }
      graph_block_sum<2>(s2, lds->b);
      rr = s2[0];
      iterations = it + 1;
      if (rr <= tolerance * tolerance * g2) { flag = GRAPH_PCG_CONVERGED; break; }
      if (!ld_isfinite(rr) || !(s2[1] > 0.0)) { flag = GRAPH_PCG_BREAKDOWN; break; }
      const double beta = s2[1] / rz;
      rz = s2[1];
      for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
        for (int k = 0; k < 6; k++) p[6ll * n + k] = zv[6ll * n + k] + beta * p[6ll * n + k];
      }
    }
  }
  return GraphPcgStatus{iterations, flag, 0.0, g2 > 0.0 ? sqrt(rr / g2) : 0.0};
}

// The Levenberg-Marquardt step: b = -g.  max |g| <= gradient_tolerance: nothing is solved (GRAPH_PCG_GRADIENT); status->gmax is
// max |g| either way, a NaN where g holds one.
__global__ __launch_bounds__(kGraphPcgThreads) void k_graph_pcg(int n_nodes, long long node_cap, long long edge_cap, double lambda,
                                                                int max_iterations, double tolerance, double gradient_tolerance,
                                                                const int* __restrict__ fixed, const int* __restrict__ parent,
                                                                const double* __restrict__ poses, const int* __restrict__ offsets,
                                                                const int* __restrict__ entries, const int* __restrict__ ei,
                                                                const int* __restrict__ ej, const double* __restrict__ g,
                                                                const double* __restrict__ D, const double* __restrict__ Minv,
                                                                const double* __restrict__ Hij, const int* __restrict__ bad,
                                                                double* x, double* r, double* p, double* zv, double* Ap,
                                                                GraphPcgStatus* __restrict__ status) {
  __shared__ GraphPcgLds lds;
  __shared__ double sh_m[kGraphPcgWaves];
  const int tid = (int)threadIdx.x;
  double gmax = 0.0;
  bool g_nan = false;
  for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double gk = g[6ll * n + k];
      gmax = fmax(gmax, fabs(gk));
      g_nan = g_nan || gk != gk;                     // (fmax drops a NaN; it is kept: it is within nobody's tolerance)
      x[6ll * n + k] = 0.0; r[6ll * n + k] = -gk;
    }
  }
  {
    // max over the workgroup: the order does not matter to a maximum; a NaN of any thread wins
    const int lane = tid & 63, wave = tid >> 6;
    double m = g_nan ? __builtin_nan("") : gmax;
    bool nan = g_nan;
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(m, off, 64);
      nan = nan || o != o;
      m = nan ? __builtin_nan("") : fmax(m, o);
    }
    if (lane == 0) sh_m[wave] = m;
  }
  graph_precondition(n_nodes, node_cap, parent, poses, Minv, r, zv, &lds);      // (its barriers also publish sh_m)
  gmax = 0.0;
  {
    bool nan = false;
#pragma unroll
    for (int w = 0; w < kGraphPcgWaves; w++) { const double o = sh_m[w]; nan = nan || o != o; gmax = fmax(gmax, o); }
    if (nan) gmax = __builtin_nan("");
  }
  GraphPcgStatus st = graph_pcg_run(n_nodes, node_cap, edge_cap, lambda, max_iterations, tolerance, gmax <= gradient_tolerance, fixed, parent, poses,
                                    offsets, entries, ei, ej, D, Minv, Hij, bad, x, r, p, zv, Ap, &lds);
  st.gmax = gmax;
  if (tid == 0) *status = st;
}

// Columns of H^-1 (liodom_graph_solve_columns / _covariance / _gate_edges; graph_marginals.h plans the launches;
// tests/graph_cov_model.py restates them).  Workgroup b solves H x = e_c, c = first_column + b = 6 slot + k: the unit vector at
// component k of node col_node[slot] (a free node whose component holds a fixed one: the host leaves every other node out), at
// lambda = 0 and without a gradient exit; |e_c| = 1, so the stopping rule is |r| <= tolerance.  Workgroup b owns the five vectors
// x, r, p, z, Ap (6 node_cap doubles each) at ws + b * 30 * node_cap; it reads nothing another workgroup writes: no polling, no
// atomic, no flag.  status[b]: iterations, flag (GRAPH_PCG_*), residual |r| when the loop ended; gmax is 0.
__global__ __launch_bounds__(kGraphPcgThreads) void k_graph_pcg_columns(int n_nodes, long long node_cap, long long edge_cap, int first_column,
                                                                        int max_iterations, double tolerance, const int* __restrict__ col_node,
                                                                        const int* __restrict__ fixed, const int* __restrict__ parent,
                                                                        const double* __restrict__ poses, const int* __restrict__ offsets,
                                                                        const int* __restrict__ entries, const int* __restrict__ ei,
                                                                        const int* __restrict__ ej, const double* __restrict__ D,
                                                                        const double* __restrict__ Minv, const double* __restrict__ Hij,
                                                                        const int* __restrict__ bad, double* ws,
                                                                        GraphPcgStatus* __restrict__ status) {
  __shared__ GraphPcgLds lds;
  const int tid = (int)threadIdx.x;
  const int column = first_column + (int)blockIdx.x;
  const int rhs_node = col_node[column / 6], rhs_k = column % 6;
  double* x = ws + (long long)blockIdx.x * 30ll * node_cap;
  double* r = x + 6ll * node_cap;
  double* p = r + 6ll * node_cap;
  double* zv = p + 6ll * node_cap;
  double* Ap = zv + 6ll * node_cap;
  for (int n = tid; n < n_nodes; n += kGraphPcgThreads) {
#pragma unroll
    for (int k = 0; k < 6; k++) { x[6ll * n + k] = 0.0; r[6ll * n + k] = (n == rhs_node && k == rhs_k) ? 1.0 : 0.0; }
  }
  graph_precondition(n_nodes, node_cap, parent, poses, Minv, r, zv, &lds);
  const GraphPcgStatus st = graph_pcg_run(n_nodes, node_cap, edge_cap, 0.0, max_iterations, tolerance, false, fixed, parent, poses, offsets,
                                          entries, ei, ej, D, Minv, Hij, bad, x, r, p, zv, Ap, &lds);
  if (tid == 0) status[blockIdx.x] = st;
}

// One thread per requested block k = Sigma[row[k], col[k]] (36 doubles, row-major): entry (a, b) is x of column 6 slot[col[k]] + b
// at [6 row[k] + a], copied if that column is one of the n_columns this launch's workspace holds (first_column on); the other
// entries are left as they are — the host clears the blocks once and launches this after every batch of columns.  slot[n] < 0 (a
// fixed node, or one the solve leaves out) and fixed rows: nothing is written, the entries stay 0.
__global__ __launch_bounds__(kGraphThreads) void k_graph_cov_gather(int n_blocks, long long node_cap, int first_column, int n_columns,
                                                                    const int* __restrict__ row, const int* __restrict__ col,
                                                                    const int* __restrict__ slot, const int* __restrict__ fixed,
                                                                    const double* __restrict__ ws, double* __restrict__ blocks) {
  const int k = (int)(blockIdx.x * kGraphThreads + threadIdx.x);
  if (k >= n_blocks) return;
  const int rn = row[k], s = slot[col[k]];
  if (s < 0 || fixed[rn] != 0) return;
  for (int b = 0; b < 6; b++) {
    const int c = 6 * s + b - first_column;
    if (c < 0 || c >= n_columns) continue;
    const double* x = ws + (long long)c * 30ll * node_cap + 6ll * rn;
#pragma unroll
    for (int a = 0; a < 6; a++) blocks[36ll * k + a * 6 + b] = x[a];
  }
}

}  // namespace liodom_dev
