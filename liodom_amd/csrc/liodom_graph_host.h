// Host side of the pose graph (C-ABI liodom_graph_* of include/liodom_hip.h).  Included by liodom_hip.hip (same translation unit:
// shares HIP_TRY / g_last_error).  A graph touches no handle and no map: it has a HIP stream and a mutex of its own, and every call
// synchronises that stream before it returns.
//
// The graph lives on the host (poses, fixed flags, edge records): that copy is what the calls read and write, and what an error
// leaves untouched.  The device copy and the CSR are made again, before the next launch, whenever the host copy has changed.
// The Levenberg-Marquardt loop runs here around the launches and graph_lm.h decides; per step tried: k_graph_gather, k_graph_pcg,
// k_graph_retract, k_graph_cost, k_graph_sum, and after an accepted one k_graph_linearize, k_graph_sum — whatever the number of
// PCG iterations.
//
// Robust losses and switched-off edges: the table of losses per kind and the active flags are part of the host copy.  At upload
// every edge gets a code (its kind's loss, or "inactive") and a scale, and the CSR and the chain are made of the active edges.
// If every code is 0 the quadratic instances of k_graph_linearize and k_graph_cost run; otherwise the robust ones, which also
// write rho and w per edge, and the cost that is summed is rho.
//
// Covariances and the loop gate (liodom_graph_solve_columns / _covariance / _gate_edges): graph_marginals.h decides which nodes
// have a covariance, which columns of H^-1 are solved and in how many launches; here graph_cov_solve launches
// k_graph_pcg_columns on the linearisation graph_prepare keeps (lambda 0), k_graph_cov_gather picks the requested blocks out of
// each launch's columns, k_graph_gate turns three blocks and a candidate edge into d2.  The host copy of the graph is only read.
#pragma once
#include <cmath>
#include <mutex>
#include <vector>

#include "graph_csr.h"
#include "graph_lm.h"
#include "graph_marginals.h"
#include "kernels_graph.h"

struct liodom_graph {
  int max_nodes = 0, max_edges = 0, device = 0;
  hipStream_t stream = nullptr;
  std::mutex mx;
  std::vector<void*> allocs;
  // the graph
  std::vector<double> poses;                  // [n][7]
  std::vector<int32_t> fixed;                 // [n]
  std::vector<liodom_graph_edge_t> edges;
  std::vector<int32_t> active;                // [n_edges]
  int32_t loss[liodom_dev::kGraphLossKinds] = {};        // per edge kind 0 .. 15; kept by reset
  double loss_scale[liodom_dev::kGraphLossKinds] = {};
  std::vector<int32_t> ei, ej;                // (made at upload) the edges' nodes, as the device holds them
  bool robust = false;                        // (made at upload) some edge's code is not 0: the robust kernels run
  int n_active = 0;                           // (made at upload)
  bool uploaded = false;                      // the device holds this graph (poses in d_poses) and its CSR
  bool linearized = false;                    // ... and its linearisation (per-edge blocks, D, g; Minv for d_lambda)
  // device
  double *d_poses = nullptr, *d_cand = nullptr, *d_z = nullptr, *d_info = nullptr;
  int *d_fixed = nullptr, *d_parent = nullptr, *d_ei = nullptr, *d_ej = nullptr, *d_offsets = nullptr, *d_entries = nullptr, *d_bad = nullptr;
  double *d_chi2 = nullptr, *d_gi = nullptr, *d_gj = nullptr, *d_Hii = nullptr, *d_Hij = nullptr, *d_Hjj = nullptr;
  double *d_g = nullptr, *d_D = nullptr, *d_Minv = nullptr;
  int* d_code = nullptr;
  double *d_scale = nullptr, *d_rho = nullptr, *d_w = nullptr;
  double *d_x = nullptr, *d_r = nullptr, *d_p = nullptr, *d_zv = nullptr, *d_Ap = nullptr, *d_in = nullptr, *d_sum = nullptr;
  liodom_dev::GraphPcgStatus* d_status = nullptr;
  // the covariance calls (graph_marginals.h): buffers made at the first call that needs them, grown when a call needs more, freed
  // with the graph
  struct Grown { void* p = nullptr; size_t bytes = 0; };
  Grown cov_ws, cov_status, cov_col_node, cov_slot, cov_rows, cov_cols, cov_blocks, cov_z, cov_info, cov_d2, cov_flag;
  int64_t cov_launches = 0, cov_columns = 0;
};

namespace {

void graph_free(liodom_graph* g) {
  if (!g) return;
  hipSetDevice(g->device);
  if (g->stream) { hipStreamSynchronize(g->stream); hipStreamDestroy(g->stream); }
  for (void* p : g->allocs) hipFree(p);
  delete g;
}

template <typename T>
int graph_alloc(liodom_graph* g, T** ptr, size_t count) {
  void* raw = nullptr;
  HIP_TRY(hipMalloc(&raw, sizeof(T) * std::max<size_t>(count, 1)));
  g->allocs.push_back(raw);
  *ptr = static_cast<T*>(raw);
  return LIODOM_OK;
}

inline int graph_n_free(const liodom_graph* g) {
  int n_free = 0;
  for (int32_t f : g->fixed) n_free += f ? 0 : 1;
  return n_free;
}

// why an edge (one to add, or a candidate for the gate) is refused; nullptr: it is not
inline const char* graph_edge_refusal(const liodom_graph_edge_t& ed, int n_nodes) {
  return ed.reserved != 0 ? "an edge's reserved field is not 0" : liodom_dev::graph_edge_refusal(ed.i, ed.j, ed.z, ed.info, n_nodes);
}

inline unsigned graph_blocks(int n) { return (unsigned)std::max(1, (n + liodom_dev::kGraphThreads - 1) / liodom_dev::kGraphThreads); }

// the device copy of the graph and its CSR
int graph_upload(liodom_graph* g) {
  if (g->uploaded) return LIODOM_OK;
  const int N = (int)g->fixed.size(), E = (int)g->edges.size();
  std::vector<int32_t>&ei = g->ei, &ej = g->ej, offsets, entries, parent, code((size_t)E);
  ei.resize((size_t)E); ej.resize((size_t)E);
  std::vector<double> z(7 * (size_t)E), info(36 * (size_t)E), scale((size_t)E);
  bool robust = false;
  int n_active = 0;
  for (int e = 0; e < E; e++) {
    const liodom_graph_edge_t& ed = g->edges[(size_t)e];
    ei[(size_t)e] = ed.i; ej[(size_t)e] = ed.j;
    std::memcpy(&z[7 * (size_t)e], ed.z, sizeof(ed.z));
    std::memcpy(&info[36 * (size_t)e], ed.info, sizeof(ed.info));
    const bool has_loss = ed.kind >= 0 && ed.kind < liodom_dev::kGraphLossKinds;      // (any other kind is quadratic)
    code[(size_t)e] = !g->active[(size_t)e] ? liodom_dev::kGraphLossInactive : has_loss ? g->loss[ed.kind] : liodom_dev::kGraphLossNone;
    scale[(size_t)e] = has_loss && g->loss[ed.kind] != liodom_dev::kGraphLossNone ? g->loss_scale[ed.kind] : 1.0;
    robust = robust || code[(size_t)e] != liodom_dev::kGraphLossNone;
    n_active += g->active[(size_t)e] ? 1 : 0;
  }
  if (!liodom_dev::graph_build_csr(ei.data(), ej.data(), E, N, &offsets, &entries, g->active.data())) {
    g_last_error = "liodom_graph: an edge names a node that does not exist"; return LIODOM_ERR_INVALID_ARG;      // (checked when it was added)
  }
  // the chain the preconditioner works along (kernels_graph.h): a free node n hangs on the first active edge (n - 1, n)
  liodom_dev::graph_chain_parents(ei.data(), ej.data(), E, g->fixed.data(), N, g->active.data(), &parent);
  g->linearized = false;
  g->robust = robust; g->n_active = n_active;
  if (N) {
    HIP_TRY(hipMemcpyAsync(g->d_parent, parent.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->d_poses, g->poses.data(), sizeof(double) * 7 * (size_t)N, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->d_fixed, g->fixed.data(), sizeof(int) * (size_t)N, hipMemcpyHostToDevice, g->stream));
  }
  HIP_TRY(hipMemcpyAsync(g->d_offsets, offsets.data(), sizeof(int) * ((size_t)N + 1), hipMemcpyHostToDevice, g->stream));
  if (E) {
    HIP_TRY(hipMemcpyAsync(g->d_ei, ei.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->d_ej, ej.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice, g->stream));
    if (!entries.empty()) HIP_TRY(hipMemcpyAsync(g->d_entries, entries.data(), sizeof(int) * entries.size(), hipMemcpyHostToDevice, g->stream));
    if (robust) {
      HIP_TRY(hipMemcpyAsync(g->d_code, code.data(), sizeof(int) * (size_t)E, hipMemcpyHostToDevice, g->stream));
      HIP_TRY(hipMemcpyAsync(g->d_scale, scale.data(), sizeof(double) * (size_t)E, hipMemcpyHostToDevice, g->stream));
    }
    HIP_TRY(hipMemcpyAsync(g->d_z, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->d_info, info.data(), sizeof(double) * info.size(), hipMemcpyHostToDevice, g->stream));
  }
  HIP_TRY(hipStreamSynchronize(g->stream));          // (the staging vectors are this function's)
  g->uploaded = true;
  return LIODOM_OK;
}

// *cost = the edges' chi2 — with a loss or an edge switched off: their rho — summed, at `poses`: the candidate's, or d_poses, and
// then the per-edge blocks are made as well (the linearisation).  Enqueued and waited for.
int graph_enqueue_cost(liodom_graph* g, const double* poses, double* cost) {
  using namespace liodom_dev;
  const int E = (int)g->edges.size();
  if (E && poses == g->d_poses) {
    hipLaunchKernelGGL(g->robust ? k_graph_linearize<true> : k_graph_linearize<false>, dim3(graph_blocks(E)), dim3(kGraphThreads), 0, g->stream, E,
                       (long long)g->max_edges, poses, g->d_ei, g->d_ej, g->d_z, g->d_info, g->d_code, g->d_scale, g->d_chi2, g->d_rho, g->d_w, g->d_gi,
                       g->d_gj, g->d_Hii, g->d_Hij, g->d_Hjj);
    HIP_TRY(hipGetLastError());
  } else if (E) {
    hipLaunchKernelGGL(g->robust ? k_graph_cost<true> : k_graph_cost<false>, dim3(graph_blocks(E)), dim3(kGraphThreads), 0, g->stream, E, poses, g->d_ei,
                       g->d_ej, g->d_z, g->d_info, g->d_code, g->d_scale, g->d_chi2, g->d_rho, g->d_w);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_graph_sum, dim3(1), dim3(kGraphPcgThreads), 0, g->stream, E, g->robust ? g->d_rho : g->d_chi2, g->d_sum);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cost, g->d_sum, sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  return LIODOM_OK;
}

int graph_gather(liodom_graph* g, double lambda) {
  using namespace liodom_dev;
  const int N = (int)g->fixed.size();
  HIP_TRY(hipMemsetAsync(g->d_bad, 0, sizeof(int), g->stream));
  hipLaunchKernelGGL(k_graph_gather, dim3(graph_blocks(N)), dim3(kGraphThreads), 0, g->stream, N, (long long)g->max_nodes, (long long)g->max_edges,
                     lambda, g->d_fixed, g->d_parent, g->d_offsets, g->d_entries, g->d_gi, g->d_gj, g->d_Hii, g->d_Hjj, g->d_g, g->d_D, g->d_Minv, g->d_bad);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// upload + linearise + gather at lambda 0, if the device does not hold them
int graph_prepare(liodom_graph* g) {
  int rc;
  if ((rc = graph_upload(g))) return rc;
  if (g->linearized) return LIODOM_OK;
  double cost = 0.0;
  if ((rc = graph_enqueue_cost(g, g->d_poses, &cost))) return rc;
  if ((rc = graph_gather(g, 0.0))) return rc;
  HIP_TRY(hipStreamSynchronize(g->stream));
  g->linearized = true;
  return LIODOM_OK;
}

int graph_check_range(const liodom_graph* g, int first, int n, size_t have, const void* ptr, const char* who) {
  if (!g || first < 0 || n < 0 || (size_t)first + (size_t)n > have || (n > 0 && !ptr)) {
    g_last_error = std::string(who) + ": null argument, a negative count, or a range beyond what the graph holds"; return LIODOM_ERR_INVALID_ARG;
  }
  return LIODOM_OK;
}

// ---- the covariance calls ----
int graph_grow(liodom_graph* g, liodom_graph::Grown* b, size_t bytes) {
  if (bytes <= b->bytes && b->p) return LIODOM_OK;
  void* raw = nullptr;
  HIP_TRY(hipMalloc(&raw, std::max<size_t>(bytes, 16)));
  if (b->p) {
    for (void*& q : g->allocs) if (q == b->p) { q = raw; break; }
    hipFree(b->p);
  } else {
    g->allocs.push_back(raw);
  }
  b->p = raw; b->bytes = std::max<size_t>(bytes, 16);
  return LIODOM_OK;
}

int graph_cov_options(const liodom_graph_cov_options_t* in, liodom_graph_cov_options_t* opt, const char* who) {
  liodom_dev::graph_cov_options_default(opt);
  if (in) *opt = *in;
  if (const char* why = liodom_dev::graph_cov_options_refusal(opt)) { g_last_error = std::string(who) + ": " + why; return LIODOM_ERR_INVALID_ARG; }
  return LIODOM_OK;
}

// What a solve of the columns of some nodes leaves: which nodes have a covariance, the column nodes and, per column, its status.
struct GraphCovSolve {
  std::vector<int32_t> anchored, col_node, slot;
  std::vector<liodom_graph_cov_status_t> column;      // [6 x column nodes]
  // the status of node n's six columns: fixed OK, not anchored UNANCHORED, else the worst of the six
  int32_t node_status(const liodom_graph* g, int32_t n) const {
    if (g->fixed[(size_t)n]) return LIODOM_GRAPH_COV_OK;
    if (!anchored[(size_t)n]) return LIODOM_GRAPH_COV_UNANCHORED;
    int32_t s = LIODOM_GRAPH_COV_OK;
    for (int b = 0; b < 6; b++) s = liodom_dev::graph_cov_worst(s, column[6 * (size_t)slot[(size_t)n] + (size_t)b].status);
    return s;
  }
};

// Solves the columns of the distinct free, anchored nodes among nodes[0 .. n) in launches of the plan's size; after each launch,
// with its columns in g->cov_ws and before the next one overwrites them, after_launch(first column, columns) enqueues what reads
// them.  The caller has validated the query and holds the mutex.
template <typename F>
int graph_cov_solve(liodom_graph* g, const liodom_graph_cov_options_t& opt, const int32_t* nodes, int n, GraphCovSolve* out, F after_launch) {
  using namespace liodom_dev;
  const int N = (int)g->fixed.size(), E = (int)g->edges.size();
  int rc;
  if ((rc = graph_prepare(g))) return rc;          // (the upload keeps ei, ej)
  if (!graph_anchored(g->ei.data(), g->ej.data(), E, g->active.data(), g->fixed.data(), N, &out->anchored)) {
    g_last_error = "liodom_graph: an edge names a node that does not exist"; return LIODOM_ERR_INVALID_ARG;      // (checked when it was added)
  }
  graph_column_nodes(nodes, n, g->fixed.data(), out->anchored.data(), N, &out->col_node, &out->slot);
  GraphCovPlan plan;
  if (!graph_cov_plan((int)out->col_node.size(), g->max_nodes, opt.batch_columns, kGraphCovWorkspaceBudget, &plan)) {
    g_last_error = "liodom_graph: the workspace of the covariance solve does not fit"; return LIODOM_ERR_INVALID_ARG;
  }
  out->column.assign((size_t)plan.columns, liodom_graph_cov_status_t{0, LIODOM_GRAPH_COV_OK, 0.0});
  if ((rc = graph_grow(g, &g->cov_slot, sizeof(int32_t) * (size_t)std::max(N, 1)))) return rc;
  if (N) HIP_TRY(hipMemcpyAsync(g->cov_slot.p, out->slot.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, g->stream));
  if (plan.columns == 0) { HIP_TRY(hipStreamSynchronize(g->stream)); return LIODOM_OK; }
  if ((rc = graph_grow(g, &g->cov_ws, plan.workspace_bytes)) || (rc = graph_grow(g, &g->cov_status, sizeof(GraphPcgStatus) * (size_t)plan.columns)) ||
      (rc = graph_grow(g, &g->cov_col_node, sizeof(int32_t) * out->col_node.size())))
    return rc;
  HIP_TRY(hipMemcpyAsync(g->cov_col_node.p, out->col_node.data(), sizeof(int32_t) * out->col_node.size(), hipMemcpyHostToDevice, g->stream));
  const int max_pcg = graph_cov_iterations(&opt, graph_n_free(g));
  GraphPcgStatus* d_st = static_cast<GraphPcgStatus*>(g->cov_status.p);
  for (int l = 0; l < plan.launches; l++) {
    int first = 0, count = 0;
    graph_cov_launch(&plan, l, &first, &count);
    hipLaunchKernelGGL(k_graph_pcg_columns, dim3((unsigned)count), dim3(kGraphPcgThreads), 0, g->stream, N, (long long)g->max_nodes, (long long)g->max_edges,
                       first, max_pcg, opt.pcg_tolerance, static_cast<const int*>(g->cov_col_node.p), g->d_fixed, g->d_parent, g->d_poses, g->d_offsets,
                       g->d_entries, g->d_ei, g->d_ej, g->d_D, g->d_Minv, g->d_Hij, g->d_bad, static_cast<double*>(g->cov_ws.p), d_st + first);
    HIP_TRY(hipGetLastError());
    g->cov_launches++; g->cov_columns += count;
    if ((rc = after_launch(first, count))) return rc;
  }
  std::vector<GraphPcgStatus> st((size_t)plan.columns);
  HIP_TRY(hipMemcpyAsync(st.data(), d_st, sizeof(GraphPcgStatus) * st.size(), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  for (size_t c = 0; c < st.size(); c++) {
    out->column[c].iterations = st[c].iterations;
    out->column[c].residual = st[c].residual;
    out->column[c].status = st[c].flag == GRAPH_PCG_CONVERGED ? LIODOM_GRAPH_COV_OK
                          : st[c].flag == GRAPH_PCG_MAX_ITER ? LIODOM_GRAPH_COV_NOT_CONVERGED : LIODOM_GRAPH_COV_BREAKDOWN;
  }
  return LIODOM_OK;
}

// blocks[k] = Sigma[rows[k], cols[k]] into g->cov_blocks (left on the device, entries of fixed nodes 0; enqueued and waited for)
// and status[k] by the rules of include/liodom_hip.h.  A status of BREAKDOWN or UNANCHORED means the caller writes NaN.
int graph_cov_blocks(liodom_graph* g, const liodom_graph_cov_options_t& opt, const int32_t* rows, const int32_t* cols, int n, int32_t* status) {
  using namespace liodom_dev;
  int rc;
  if ((rc = graph_grow(g, &g->cov_rows, sizeof(int32_t) * (size_t)n)) || (rc = graph_grow(g, &g->cov_cols, sizeof(int32_t) * (size_t)n)) ||
      (rc = graph_grow(g, &g->cov_blocks, sizeof(double) * 36 * (size_t)n)))
    return rc;
  HIP_TRY(hipMemcpyAsync(g->cov_rows.p, rows, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
  HIP_TRY(hipMemcpyAsync(g->cov_cols.p, cols, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
  HIP_TRY(hipMemsetAsync(g->cov_blocks.p, 0, sizeof(double) * 36 * (size_t)n, g->stream));
  GraphCovSolve sol;
  rc = graph_cov_solve(g, opt, cols, n, &sol, [&](int first, int count) -> int {
    hipLaunchKernelGGL(k_graph_cov_gather, dim3(graph_blocks(n)), dim3(kGraphThreads), 0, g->stream, n, (long long)g->max_nodes, first, count,
                       static_cast<const int*>(g->cov_rows.p), static_cast<const int*>(g->cov_cols.p), static_cast<const int*>(g->cov_slot.p), g->d_fixed,
                       static_cast<const double*>(g->cov_ws.p), static_cast<double*>(g->cov_blocks.p));
    HIP_TRY(hipGetLastError());
    return LIODOM_OK;
  });
  if (rc) return rc;
  for (int k = 0; k < n; k++) {
    const int32_t r = rows[k], c = cols[k];
    if (g->fixed[(size_t)r] || g->fixed[(size_t)c]) status[k] = LIODOM_GRAPH_COV_OK;
    else if (!sol.anchored[(size_t)r] || !sol.anchored[(size_t)c]) status[k] = LIODOM_GRAPH_COV_UNANCHORED;
    else status[k] = sol.node_status(g, c);
  }
  return LIODOM_OK;
}

inline bool graph_cov_is_nan(int32_t status) { return status == LIODOM_GRAPH_COV_BREAKDOWN || status == LIODOM_GRAPH_COV_UNANCHORED || status == LIODOM_GRAPH_COV_NOT_PD; }

}  // namespace

extern "C" {

int liodom_graph_create(int max_nodes, int max_edges, liodom_graph_t** out) {
  using namespace liodom_dev;
  if (!out) { g_last_error = "liodom_graph_create: null argument"; return LIODOM_ERR_INVALID_ARG; }
  *out = nullptr;
  if (max_nodes < 1 || max_nodes > kGraphMaxNodes || max_edges < 1 || max_edges > kGraphMaxEdges) {
    g_last_error = "liodom_graph_create: max_nodes outside 1 .. 65536 or max_edges outside 1 .. 262144"; return LIODOM_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "liodom_graph_create: no HIP device available (this library has no CPU fallback)";
    return LIODOM_ERR_NO_DEVICE;
  }
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  liodom_graph* g = new liodom_graph();
  g->max_nodes = max_nodes; g->max_edges = max_edges; g->device = dev;
  auto build = [&]() -> int {
    HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    const size_t N = (size_t)max_nodes, E = (size_t)max_edges;
    int rc;
    if ((rc = graph_alloc(g, &g->d_poses, 7 * N)) || (rc = graph_alloc(g, &g->d_cand, 7 * N)) || (rc = graph_alloc(g, &g->d_fixed, N)) || (rc = graph_alloc(g, &g->d_parent, N)) ||
        (rc = graph_alloc(g, &g->d_offsets, N + 1)) || (rc = graph_alloc(g, &g->d_ei, E)) || (rc = graph_alloc(g, &g->d_ej, E)) ||
        (rc = graph_alloc(g, &g->d_entries, 2 * E)) || (rc = graph_alloc(g, &g->d_z, 7 * E)) || (rc = graph_alloc(g, &g->d_info, 36 * E)) ||
        (rc = graph_alloc(g, &g->d_chi2, E)) || (rc = graph_alloc(g, &g->d_gi, 6 * E)) || (rc = graph_alloc(g, &g->d_gj, 6 * E)) ||
        (rc = graph_alloc(g, &g->d_Hii, 36 * E)) || (rc = graph_alloc(g, &g->d_Hij, 36 * E)) || (rc = graph_alloc(g, &g->d_Hjj, 36 * E)) ||
        (rc = graph_alloc(g, &g->d_g, 6 * N)) || (rc = graph_alloc(g, &g->d_D, 36 * N)) || (rc = graph_alloc(g, &g->d_Minv, 36 * N)) ||
        (rc = graph_alloc(g, &g->d_x, 6 * N)) || (rc = graph_alloc(g, &g->d_r, 6 * N)) || (rc = graph_alloc(g, &g->d_p, 6 * N)) ||
        (rc = graph_alloc(g, &g->d_zv, 6 * N)) || (rc = graph_alloc(g, &g->d_Ap, 6 * N)) || (rc = graph_alloc(g, &g->d_in, 6 * N)) ||
        (rc = graph_alloc(g, &g->d_code, E)) || (rc = graph_alloc(g, &g->d_scale, E)) || (rc = graph_alloc(g, &g->d_rho, E)) || (rc = graph_alloc(g, &g->d_w, E)) ||
        (rc = graph_alloc(g, &g->d_sum, 1)) || (rc = graph_alloc(g, &g->d_bad, 1)) || (rc = graph_alloc(g, &g->d_status, 1)))
      return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    return LIODOM_OK;
  };
  const int rc = build();
  if (rc != LIODOM_OK) { graph_free(g); return rc; }
  *out = g;
  return LIODOM_OK;
}

void liodom_graph_destroy(liodom_graph_t* g) { graph_free(g); }

int liodom_graph_reset(liodom_graph_t* g) {
  if (!g) { g_last_error = "liodom_graph_reset: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  g->poses.clear(); g->fixed.clear(); g->edges.clear(); g->active.clear();        // (the loss table is a setting: it stays)
  g->uploaded = false; g->linearized = false;
  return LIODOM_OK;
}

int liodom_graph_count(liodom_graph_t* g, int32_t* n_nodes, int32_t* n_edges) {
  if (!g) { g_last_error = "liodom_graph_count: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (n_nodes) *n_nodes = (int32_t)g->fixed.size();
  if (n_edges) *n_edges = (int32_t)g->edges.size();
  return LIODOM_OK;
}

int liodom_graph_add_nodes(liodom_graph_t* g, const double* poses, const int32_t* fixed, int n, int32_t* first) {
  if (!g || n < 0 || (n > 0 && !poses)) { g_last_error = "liodom_graph_add_nodes: null graph or poses, or a negative count"; return LIODOM_ERR_INVALID_ARG; }
  for (int k = 0; k < n; k++) {
    if (const char* why = liodom_dev::graph_pose_refusal(poses + 7 * (size_t)k)) { g_last_error = std::string("liodom_graph_add_nodes: ") + why; return LIODOM_ERR_INVALID_ARG; }
  }
  std::lock_guard<std::mutex> lk(g->mx);
  if (g->fixed.size() + (size_t)n > (size_t)g->max_nodes) { g_last_error = "liodom_graph_add_nodes: more nodes than max_nodes"; return LIODOM_ERR_CAPACITY; }
  if (first) *first = (int32_t)g->fixed.size();
  if (n == 0) return LIODOM_OK;
  const size_t at = g->fixed.size();
  g->poses.resize(7 * (at + (size_t)n));
  g->fixed.resize(at + (size_t)n);
  for (int k = 0; k < n; k++) {
    liodom_dev::graph_pose_normalised(poses + 7 * (size_t)k, &g->poses[7 * (at + (size_t)k)]);
    g->fixed[at + (size_t)k] = (fixed && fixed[k]) ? 1 : 0;
  }
  g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_add_edges(liodom_graph_t* g, const liodom_graph_edge_t* edges, int n) {
  if (!g || n < 0 || (n > 0 && !edges)) { g_last_error = "liodom_graph_add_edges: null graph or edges, or a negative count"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size();
  for (int k = 0; k < n; k++) {
    if (const char* why = graph_edge_refusal(edges[k], N)) { g_last_error = std::string("liodom_graph_add_edges: ") + why; return LIODOM_ERR_INVALID_ARG; }
  }
  if (g->edges.size() + (size_t)n > (size_t)g->max_edges) { g_last_error = "liodom_graph_add_edges: more edges than max_edges"; return LIODOM_ERR_CAPACITY; }
  if (n == 0) return LIODOM_OK;
  g->edges.reserve(g->edges.size() + (size_t)n);
  for (int k = 0; k < n; k++) {
    liodom_graph_edge_t ed = edges[k];
    liodom_dev::graph_pose_normalised(edges[k].z, ed.z);
    g->edges.push_back(ed);
  }
  g->active.resize(g->edges.size(), 1);
  g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_set_fixed(liodom_graph_t* g, int first, int n, const int32_t* fixed) {
  if (!g) { g_last_error = "liodom_graph_set_fixed: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->fixed.size(), fixed, "liodom_graph_set_fixed")) return rc;
  for (int k = 0; k < n; k++) g->fixed[(size_t)first + (size_t)k] = fixed[k] ? 1 : 0;
  if (n) g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_get_poses(liodom_graph_t* g, int first, int n, double* poses) {
  if (!g) { g_last_error = "liodom_graph_get_poses: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->fixed.size(), poses, "liodom_graph_get_poses")) return rc;
  if (n) std::memcpy(poses, &g->poses[7 * (size_t)first], sizeof(double) * 7 * (size_t)n);
  return LIODOM_OK;
}

int liodom_graph_set_poses(liodom_graph_t* g, int first, int n, const double* poses) {
  if (!g) { g_last_error = "liodom_graph_set_poses: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->fixed.size(), poses, "liodom_graph_set_poses")) return rc;
  for (int k = 0; k < n; k++) {
    if (const char* why = liodom_dev::graph_pose_refusal(poses + 7 * (size_t)k)) { g_last_error = std::string("liodom_graph_set_poses: ") + why; return LIODOM_ERR_INVALID_ARG; }
  }
  for (int k = 0; k < n; k++) liodom_dev::graph_pose_normalised(poses + 7 * (size_t)k, &g->poses[7 * ((size_t)first + (size_t)k)]);
  if (n) g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_get_edges(liodom_graph_t* g, int first, int n, liodom_graph_edge_t* edges) {
  if (!g) { g_last_error = "liodom_graph_get_edges: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->edges.size(), edges, "liodom_graph_get_edges")) return rc;
  if (n) std::memcpy(edges, &g->edges[(size_t)first], sizeof(liodom_graph_edge_t) * (size_t)n);
  return LIODOM_OK;
}

int liodom_graph_linearize(liodom_graph_t* g, double* chi2_per_edge, double* gradient, double* diag) {
  if (!g) { g_last_error = "liodom_graph_linearize: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  HIP_TRY(hipSetDevice(g->device));
  if (int rc = graph_prepare(g)) return rc;
  const size_t N = g->fixed.size(), E = g->edges.size();
  std::vector<double> D;
  if (chi2_per_edge && E) HIP_TRY(hipMemcpyAsync(chi2_per_edge, g->d_chi2, sizeof(double) * E, hipMemcpyDeviceToHost, g->stream));
  if (gradient && N) HIP_TRY(hipMemcpyAsync(gradient, g->d_g, sizeof(double) * 6 * N, hipMemcpyDeviceToHost, g->stream));
  if (diag && N) {
    D.resize(36 * N);
    HIP_TRY(hipMemcpy2DAsync(D.data(), sizeof(double) * N, g->d_D, sizeof(double) * (size_t)g->max_nodes, sizeof(double) * N, 36, hipMemcpyDeviceToHost, g->stream));
  }
  HIP_TRY(hipStreamSynchronize(g->stream));
  if (diag && N) {
    for (size_t n = 0; n < N; n++)
      for (size_t k = 0; k < 36; k++) diag[36 * n + k] = D[k * N + n];          // the device keeps the blocks component-major
  }
  return LIODOM_OK;
}

int liodom_graph_multiply(liodom_graph_t* g, double lambda, const double* x, double* y) {
  using namespace liodom_dev;
  if (!g) { g_last_error = "liodom_graph_multiply: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size();
  if (N > 0 && (!x || !y)) { g_last_error = "liodom_graph_multiply: null x or y"; return LIODOM_ERR_INVALID_ARG; }
  if (!(lambda >= 0.0) || !std::isfinite(lambda)) { g_last_error = "liodom_graph_multiply: lambda is negative or not finite"; return LIODOM_ERR_INVALID_ARG; }
  if (N == 0) return LIODOM_OK;
  HIP_TRY(hipSetDevice(g->device));
  if (int rc = graph_prepare(g)) return rc;
  HIP_TRY(hipMemcpyAsync(g->d_in, x, sizeof(double) * 6 * (size_t)N, hipMemcpyHostToDevice, g->stream));
  hipLaunchKernelGGL(k_graph_multiply, dim3(graph_blocks(N)), dim3(kGraphThreads), 0, g->stream, N, (long long)g->max_nodes, (long long)g->max_edges,
                     lambda, g->d_fixed, g->d_offsets, g->d_entries, g->d_ei, g->d_ej, g->d_D, g->d_Hij, g->d_in, g->d_Ap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(y, g->d_Ap, sizeof(double) * 6 * (size_t)N, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  return LIODOM_OK;
}

int liodom_graph_set_loss(liodom_graph_t* g, int kind, int loss, double scale) {
  using namespace liodom_dev;
  if (!g) { g_last_error = "liodom_graph_set_loss: null graph"; return LIODOM_ERR_INVALID_ARG; }
  if (kind < 0 || kind >= kGraphLossKinds) { g_last_error = "liodom_graph_set_loss: kind outside 0 .. 15"; return LIODOM_ERR_INVALID_ARG; }
  if (loss < kGraphLossNone || loss > kGraphLossGemanMcClure) { g_last_error = "liodom_graph_set_loss: unknown loss"; return LIODOM_ERR_INVALID_ARG; }
  if (loss != kGraphLossNone && (!std::isfinite(scale) || !(scale > 0.0))) {
    g_last_error = "liodom_graph_set_loss: the scale is not finite and > 0"; return LIODOM_ERR_INVALID_ARG;
  }
  std::lock_guard<std::mutex> lk(g->mx);
  g->loss[kind] = loss;
  g->loss_scale[kind] = loss == kGraphLossNone ? 0.0 : scale;
  g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_get_loss(liodom_graph_t* g, int kind, int32_t* loss, double* scale) {
  if (!g) { g_last_error = "liodom_graph_get_loss: null graph"; return LIODOM_ERR_INVALID_ARG; }
  if (kind < 0 || kind >= liodom_dev::kGraphLossKinds) { g_last_error = "liodom_graph_get_loss: kind outside 0 .. 15"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (loss) *loss = g->loss[kind];
  if (scale) *scale = g->loss_scale[kind];
  return LIODOM_OK;
}

int liodom_graph_set_edge_active(liodom_graph_t* g, int first, int n, const int32_t* active) {
  if (!g) { g_last_error = "liodom_graph_set_edge_active: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->edges.size(), active, "liodom_graph_set_edge_active")) return rc;
  for (int k = 0; k < n; k++) g->active[(size_t)first + (size_t)k] = active[k] ? 1 : 0;
  if (n) g->uploaded = false;
  return LIODOM_OK;
}

int liodom_graph_get_edge_active(liodom_graph_t* g, int first, int n, int32_t* active) {
  if (!g) { g_last_error = "liodom_graph_get_edge_active: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (int rc = graph_check_range(g, first, n, g->edges.size(), active, "liodom_graph_get_edge_active")) return rc;
  if (n) std::memcpy(active, &g->active[(size_t)first], sizeof(int32_t) * (size_t)n);
  return LIODOM_OK;
}

int liodom_graph_edge_weights(liodom_graph_t* g, double* rho, double* weight) {
  if (!g) { g_last_error = "liodom_graph_edge_weights: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  const size_t E = g->edges.size();
  if (E == 0 || (!rho && !weight)) return LIODOM_OK;
  HIP_TRY(hipSetDevice(g->device));
  if (int rc = graph_prepare(g)) return rc;
  if (g->robust) {
    if (rho) HIP_TRY(hipMemcpyAsync(rho, g->d_rho, sizeof(double) * E, hipMemcpyDeviceToHost, g->stream));
    if (weight) HIP_TRY(hipMemcpyAsync(weight, g->d_w, sizeof(double) * E, hipMemcpyDeviceToHost, g->stream));
  } else {                                            // quadratic, every edge active: rho = chi2, w = 1
    if (rho) HIP_TRY(hipMemcpyAsync(rho, g->d_chi2, sizeof(double) * E, hipMemcpyDeviceToHost, g->stream));
    if (weight) for (size_t e = 0; e < E; e++) weight[e] = 1.0;
  }
  HIP_TRY(hipStreamSynchronize(g->stream));
  return LIODOM_OK;
}

void liodom_graph_options_default(liodom_graph_options_t* opt) {
  if (opt) liodom_dev::graph_lm_options_default(opt);
}

int liodom_graph_optimize(liodom_graph_t* g, const liodom_graph_options_t* opt_in, liodom_graph_report_t* report) {
  using namespace liodom_dev;
  if (!g) { g_last_error = "liodom_graph_optimize: null graph"; return LIODOM_ERR_INVALID_ARG; }
  liodom_graph_options_t opt;
  graph_lm_options_default(&opt);
  if (opt_in) opt = *opt_in;
  if (const char* why = graph_lm_options_refusal(&opt)) { g_last_error = std::string("liodom_graph_optimize: ") + why; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size(), n_free = graph_n_free(g);
  if (n_free == N) { g_last_error = "liodom_graph_optimize: the graph has no fixed node"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(g->device));
  int rc;
  if ((rc = graph_upload(g))) return rc;
  double cost = 0.0;
  if ((rc = graph_enqueue_cost(g, g->d_poses, &cost))) return rc;
  g->linearized = false;                              // (Minv is about to be made for another lambda)
  GraphLm lm;
  if (!lm.begin(opt, cost, n_free, g->n_active)) { if (report) *report = lm.rep; return LIODOM_OK; }
  bool moved = false;                                 // d_poses differs from the host's poses
  // from here on an error must leave the host copy as it is and the device copy marked stale
  auto run = [&]() -> int {
    while (true) {
      if ((rc = graph_gather(g, lm.lambda))) return rc;
      hipLaunchKernelGGL(k_graph_pcg, dim3(1), dim3(kGraphPcgThreads), 0, g->stream, N, (long long)g->max_nodes, (long long)g->max_edges, lm.lambda,
                         lm.pcg_iterations(), opt.pcg_tolerance, opt.gradient_tolerance, g->d_fixed, g->d_parent, g->d_poses, g->d_offsets, g->d_entries,
                         g->d_ei, g->d_ej, g->d_g, g->d_D, g->d_Minv, g->d_Hij, g->d_bad, g->d_x, g->d_r, g->d_p, g->d_zv, g->d_Ap, g->d_status);
      HIP_TRY(hipGetLastError());
      GraphPcgStatus st;
      HIP_TRY(hipMemcpyAsync(&st, g->d_status, sizeof(st), hipMemcpyDeviceToHost, g->stream));
      HIP_TRY(hipStreamSynchronize(g->stream));
      if (!lm.after_pcg(st.flag, st.iterations, st.gmax)) return LIODOM_OK;
      hipLaunchKernelGGL(k_graph_retract, dim3(graph_blocks(N)), dim3(kGraphThreads), 0, g->stream, N, g->d_poses, g->d_fixed, g->d_x, g->d_cand);
      HIP_TRY(hipGetLastError());
      double cand = 0.0;
      if ((rc = graph_enqueue_cost(g, g->d_cand, &cand))) return rc;
      const GraphLmStep step = lm.after_cost(cand);
      if (step == GRAPH_LM_DONE) return LIODOM_OK;
      if (step == GRAPH_LM_ACCEPTED) {
        std::swap(g->d_poses, g->d_cand);
        moved = true;
        if ((rc = graph_enqueue_cost(g, g->d_poses, &cost))) return rc;
        lm.relinearized(cost);
      }
    }
  };
  rc = run();
  std::vector<double> out;
  if (rc == LIODOM_OK && moved) {
    out.resize(7 * (size_t)N);
    hipError_t e = hipMemcpyAsync(out.data(), g->d_poses, sizeof(double) * out.size(), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) { g_last_error = std::string("liodom_graph_optimize: download failed: ") + hipGetErrorString(e); rc = LIODOM_ERR_HIP; }
  }
  if (rc != LIODOM_OK) { g->uploaded = false; g->linearized = false; return rc; }
  if (moved) g->poses.swap(out);
  if (report) *report = lm.rep;
  return LIODOM_OK;
}

void liodom_graph_cov_options_default(liodom_graph_cov_options_t* opt) {
  if (opt) liodom_dev::graph_cov_options_default(opt);
}

int liodom_graph_cov_counters(liodom_graph_t* g, int64_t* launches, int64_t* columns) {
  if (!g) { g_last_error = "liodom_graph_cov_counters: null graph"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(g->mx);
  if (launches) *launches = g->cov_launches;
  if (columns) *columns = g->cov_columns;
  return LIODOM_OK;
}

int liodom_graph_solve_columns(liodom_graph_t* g, const int32_t* nodes, int n, const liodom_graph_cov_options_t* opt_in, double* x,
                               liodom_graph_cov_status_t* status) {
  using namespace liodom_dev;
  if (!g) { g_last_error = "liodom_graph_solve_columns: null graph"; return LIODOM_ERR_INVALID_ARG; }
  liodom_graph_cov_options_t opt;
  if (int rc = graph_cov_options(opt_in, &opt, "liodom_graph_solve_columns")) return rc;
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size();
  if (const char* why = graph_query_refusal(nodes, n, N)) { g_last_error = std::string("liodom_graph_solve_columns: ") + why; return LIODOM_ERR_INVALID_ARG; }
  if (n > 0 && (!x || !status)) { g_last_error = "liodom_graph_solve_columns: null x or status"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  HIP_TRY(hipSetDevice(g->device));
  const size_t len = 6 * (size_t)N;
  std::vector<double> solved;                         // [column][6 N]: every solved column, copied out launch by launch
  GraphCovSolve sol;
  bool sized = false;
  int rc = graph_cov_solve(g, opt, nodes, n, &sol, [&](int first, int count) -> int {
    if (!sized) { solved.resize(6 * sol.col_node.size() * len); sized = true; }
    HIP_TRY(hipMemcpy2DAsync(&solved[(size_t)first * len], sizeof(double) * len, g->cov_ws.p, sizeof(double) * kGraphCovColumnDoubles * (size_t)g->max_nodes,
                             sizeof(double) * len, (size_t)count, hipMemcpyDeviceToHost, g->stream));
    return LIODOM_OK;
  });
  if (rc) return rc;
  const double nan = std::nan("");
  for (int k = 0; k < n; k++) {
    const int32_t v = nodes[k];
    for (int b = 0; b < 6; b++) {
      double* out = x + (6 * (size_t)k + (size_t)b) * len;
      liodom_graph_cov_status_t* st = status + 6 * (size_t)k + (size_t)b;
      if (g->fixed[(size_t)v]) {
        std::fill(out, out + len, 0.0);
        *st = liodom_graph_cov_status_t{0, LIODOM_GRAPH_COV_OK, 0.0};
      } else if (!sol.anchored[(size_t)v]) {
        std::fill(out, out + len, nan);
        *st = liodom_graph_cov_status_t{0, LIODOM_GRAPH_COV_UNANCHORED, nan};
      } else {
        const size_t c = 6 * (size_t)sol.slot[(size_t)v] + (size_t)b;
        *st = sol.column[c];
        if (st->status == LIODOM_GRAPH_COV_BREAKDOWN) std::fill(out, out + len, nan);
        else std::memcpy(out, &solved[c * len], sizeof(double) * len);
      }
    }
  }
  return LIODOM_OK;
}

int liodom_graph_covariance(liodom_graph_t* g, const int32_t* rows, const int32_t* cols, int n, const liodom_graph_cov_options_t* opt_in,
                            double* blocks, int32_t* status) {
  using namespace liodom_dev;
  if (!g) { g_last_error = "liodom_graph_covariance: null graph"; return LIODOM_ERR_INVALID_ARG; }
  liodom_graph_cov_options_t opt;
  if (int rc = graph_cov_options(opt_in, &opt, "liodom_graph_covariance")) return rc;
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size();
  const char* why = graph_query_refusal(rows, n, N);
  if (!why) why = graph_query_refusal(cols, n, N);
  if (why) { g_last_error = std::string("liodom_graph_covariance: ") + why; return LIODOM_ERR_INVALID_ARG; }
  if (n > 0 && (!blocks || !status)) { g_last_error = "liodom_graph_covariance: null blocks or status"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  HIP_TRY(hipSetDevice(g->device));
  std::vector<int32_t> st((size_t)n);
  if (int rc = graph_cov_blocks(g, opt, rows, cols, n, st.data())) return rc;
  std::vector<double> out(36 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(out.data(), g->cov_blocks.p, sizeof(double) * out.size(), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  for (int k = 0; k < n; k++) {
    if (graph_cov_is_nan(st[(size_t)k])) std::fill(out.begin() + 36 * (size_t)k, out.begin() + 36 * ((size_t)k + 1), std::nan(""));
  }
  std::memcpy(blocks, out.data(), sizeof(double) * out.size());
  std::memcpy(status, st.data(), sizeof(int32_t) * st.size());
  return LIODOM_OK;
}

int liodom_graph_gate_edges(liodom_graph_t* g, const liodom_graph_edge_t* candidates, int n, const liodom_graph_cov_options_t* opt_in, double* d2,
                            int32_t* status) {
  using namespace liodom_dev;
  if (!g || n < 0 || (n > 0 && !candidates)) { g_last_error = "liodom_graph_gate_edges: null graph or candidates, or a negative count"; return LIODOM_ERR_INVALID_ARG; }
  liodom_graph_cov_options_t opt;
  if (int rc = graph_cov_options(opt_in, &opt, "liodom_graph_gate_edges")) return rc;
  std::lock_guard<std::mutex> lk(g->mx);
  const int N = (int)g->fixed.size();
  for (int k = 0; k < n; k++) {
    if (const char* why = ::graph_edge_refusal(candidates[k], N)) { g_last_error = std::string("liodom_graph_gate_edges: ") + why; return LIODOM_ERR_INVALID_ARG; }
  }
  if (n > 0 && (!d2 || !status)) { g_last_error = "liodom_graph_gate_edges: null d2 or status"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  if ((size_t)n > (size_t)0x7fffffff / 3) { g_last_error = "liodom_graph_gate_edges: too many candidates"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(g->device));
  // three blocks per candidate: Sigma[i, i], Sigma[i, j], Sigma[j, j]
  std::vector<int32_t> rows(3 * (size_t)n), cols(3 * (size_t)n), st(3 * (size_t)n), ci((size_t)n), cj((size_t)n), flag((size_t)n);
  std::vector<double> z(7 * (size_t)n), info(36 * (size_t)n), out((size_t)n);
  for (int k = 0; k < n; k++) {
    const liodom_graph_edge_t& c = candidates[k];
    rows[3 * (size_t)k] = c.i; cols[3 * (size_t)k] = c.i;
    rows[3 * (size_t)k + 1] = c.i; cols[3 * (size_t)k + 1] = c.j;
    rows[3 * (size_t)k + 2] = c.j; cols[3 * (size_t)k + 2] = c.j;
    ci[(size_t)k] = c.i; cj[(size_t)k] = c.j;
    graph_pose_normalised(c.z, &z[7 * (size_t)k]);          // (as liodom_graph_add_edges stores it)
    std::memcpy(&info[36 * (size_t)k], c.info, sizeof(c.info));
  }
  int rc;
  if ((rc = graph_cov_blocks(g, opt, rows.data(), cols.data(), 3 * n, st.data()))) return rc;
  // (the candidates' i and j reuse the buffers of the rows and columns: the gather that read those has been waited for)
  if ((rc = graph_grow(g, &g->cov_z, sizeof(double) * z.size())) || (rc = graph_grow(g, &g->cov_info, sizeof(double) * info.size())) ||
      (rc = graph_grow(g, &g->cov_d2, sizeof(double) * (size_t)n)) || (rc = graph_grow(g, &g->cov_flag, sizeof(int32_t) * (size_t)n)))
    return rc;
  HIP_TRY(hipMemcpyAsync(g->cov_rows.p, ci.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
  HIP_TRY(hipMemcpyAsync(g->cov_cols.p, cj.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, g->stream));
  HIP_TRY(hipMemcpyAsync(g->cov_z.p, z.data(), sizeof(double) * z.size(), hipMemcpyHostToDevice, g->stream));
  HIP_TRY(hipMemcpyAsync(g->cov_info.p, info.data(), sizeof(double) * info.size(), hipMemcpyHostToDevice, g->stream));
  hipLaunchKernelGGL(k_graph_gate, dim3(graph_blocks(n)), dim3(kGraphThreads), 0, g->stream, n, g->d_poses, static_cast<const int*>(g->cov_rows.p),
                     static_cast<const int*>(g->cov_cols.p), static_cast<const double*>(g->cov_z.p), static_cast<const double*>(g->cov_info.p),
                     static_cast<const double*>(g->cov_blocks.p), static_cast<double*>(g->cov_d2.p), static_cast<int*>(g->cov_flag.p));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out.data(), g->cov_d2.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipMemcpyAsync(flag.data(), g->cov_flag.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(hipStreamSynchronize(g->stream));
  for (int k = 0; k < n; k++) {
    int32_t s = graph_cov_worst(st[3 * (size_t)k], st[3 * (size_t)k + 2]);
    if (s != LIODOM_GRAPH_COV_BREAKDOWN && s != LIODOM_GRAPH_COV_UNANCHORED && flag[(size_t)k]) s = LIODOM_GRAPH_COV_NOT_PD;
    status[k] = s;
    d2[k] = graph_cov_is_nan(s) ? std::nan("") : out[(size_t)k];
  }
  return LIODOM_OK;
}

}  // extern "C"
