// graph_marginals.h — the plain-C++ half of the graph's covariance calls (liodom_graph_solve_columns / _covariance / _gate_edges;
// kernels in kernels_graph.h, host entry points in liodom_graph_host.h; DESIGN.md §3 "Covariances of the graph and the
// loop gate"): the options' defaults and validation, the validation of a query, which nodes have a finite covariance at all, the
// distinct nodes whose columns of H^-1 are solved, and how those columns are cut into launches that fit a workspace —
// overflow-checked.  No HIP include: tests/graph_marginals_main.cc compiles it for the host alone, plain and under sanitizers
// (tests/test_graph_marginals_host.py).
//
// ANCHORING.  H is singular along every connected component (over the active edges) that holds no fixed node: such a component
// can move rigidly at no cost.  A free node of such a component — a free node without edges is one — has no finite covariance:
// its status is UNANCHORED and no column of it is ever solved.  Columns of fixed nodes are 0 and are not solved either.
//
// COLUMNS.  The distinct free, anchored nodes of a query, in the order of their first appearance, are its column nodes; node
// col_node[s] has slot s and the columns 6 s .. 6 s + 5.  A launch solves a run of consecutive columns, one workgroup each, in a
// workspace of 30 node_cap doubles per column (five vectors of 6 node_cap: x, r, p, z, Ap).  Columns do not know of each other,
// so how they are cut into launches changes no byte of any of them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/liodom_hip.h"
#include "graph_lm.h"
#include "liodom_sizes.h"

namespace liodom_dev {

constexpr int kGraphCovColumnsMin = 6;               // an automatic plan never solves less than one node per launch
constexpr size_t kGraphCovColumnDoubles = 30;        // per column and node_cap: x, r, p, z, Ap of 6 each

inline void graph_cov_options_default(liodom_graph_cov_options_t* o) {
  o->max_pcg_iterations = 0;      // 6 x free nodes, at most 65 536
  o->batch_columns = 0;           // as many as fit kGraphCovWorkspaceBudget
  o->pcg_tolerance = 1e-8;
}
// nullptr: fine; otherwise why not (static text)
inline const char* graph_cov_options_refusal(const liodom_graph_cov_options_t* o) {
  if (o->max_pcg_iterations < 0 || o->batch_columns < 0) return "max_pcg_iterations or batch_columns is negative";
  if (!(o->pcg_tolerance >= 0.0)) return "pcg_tolerance is negative or not a number";
  return nullptr;
}
inline int graph_cov_iterations(const liodom_graph_cov_options_t* o, int n_free) { return graph_pcg_cap(o->max_pcg_iterations, n_free); }

// A query names nodes: n >= 0, a list where n > 0, every index a node of the graph.
inline const char* graph_query_refusal(const int32_t* nodes, int n, int n_nodes) {
  if (n < 0) return "a negative count";
  if (n > 0 && !nodes) return "a null list of nodes";
  for (int k = 0; k < n; k++) if (nodes[k] < 0 || nodes[k] >= n_nodes) return "a query names a node that does not exist";
  return nullptr;
}

// anchored[n] = 1 where node n's connected component over the active edges (active null: every edge) holds a fixed node — a fixed
// node is anchored —, else 0.  Union-find with path halving, the smaller index as the root: the result depends on the graph
// alone.  false (output unspecified): a negative count or an edge that names no node.
inline bool graph_anchored(const int32_t* ei, const int32_t* ej, int n_edges, const int32_t* active, const int32_t* fixed, int n_nodes,
                           std::vector<int32_t>* anchored) {
  if (n_nodes < 0 || n_edges < 0) return false;
  std::vector<int32_t> root((size_t)n_nodes);
  for (int n = 0; n < n_nodes; n++) root[(size_t)n] = n;
  auto find = [&](int32_t n) {
    while (root[(size_t)n] != n) { root[(size_t)n] = root[(size_t)root[(size_t)n]]; n = root[(size_t)n]; }
    return n;
  };
  for (int e = 0; e < n_edges; e++) {
    if (ei[e] < 0 || ei[e] >= n_nodes || ej[e] < 0 || ej[e] >= n_nodes) return false;
    if (active && !active[e]) continue;
    const int32_t a = find(ei[e]), b = find(ej[e]);
    if (a < b) root[(size_t)b] = a; else if (b < a) root[(size_t)a] = b;
  }
  std::vector<int32_t> holds((size_t)n_nodes, 0);
  for (int n = 0; n < n_nodes; n++) if (fixed[n]) holds[(size_t)find(n)] = 1;
  anchored->assign((size_t)n_nodes, 0);
  for (int n = 0; n < n_nodes; n++) (*anchored)[(size_t)n] = holds[(size_t)find(n)];
  return true;
}

// The column nodes of a query that has passed graph_query_refusal: col_node = its distinct free, anchored nodes in the order of
// their first appearance; slot[n] (n_nodes entries) = the place of node n in col_node, -1 for every other node.
inline void graph_column_nodes(const int32_t* nodes, int n, const int32_t* fixed, const int32_t* anchored, int n_nodes,
                               std::vector<int32_t>* col_node, std::vector<int32_t>* slot) {
  col_node->clear();
  slot->assign((size_t)(n_nodes > 0 ? n_nodes : 0), -1);
  for (int k = 0; k < n; k++) {
    const int32_t v = nodes[k];
    if (fixed[v] || !anchored[v] || (*slot)[(size_t)v] >= 0) continue;
    (*slot)[(size_t)v] = (int32_t)col_node->size();
    col_node->push_back(v);
  }
}

struct GraphCovPlan {
  int columns;               // 6 x column nodes
  int per_launch;            // columns of a launch (the last one may hold fewer)
  int launches;
  size_t column_doubles;     // 30 node_cap: the stride from one column's vectors to the next
  size_t workspace_bytes;    // per_launch columns
};

inline bool graph_cov_mul(size_t a, size_t b, size_t* out) {
  if (a != 0 && b > (size_t)-1 / a) return false;
  *out = a * b;
  return true;
}

// The launches of n_col_nodes column nodes in a graph of capacity node_cap.  batch_columns > 0: that many columns per launch (no
// more than there are); 0: as many as fit `budget` bytes of workspace, at least kGraphCovColumnsMin and no more than there are.
// No column node: no launch, no workspace.  false: a negative argument, node_cap 0, or a size that does not fit size_t or an int.
inline bool graph_cov_plan(int n_col_nodes, long long node_cap, int batch_columns, size_t budget, GraphCovPlan* p) {
  memset(p, 0, sizeof(*p));
  if (n_col_nodes < 0 || node_cap < 1 || batch_columns < 0) return false;
  if (n_col_nodes > 0x7fffffff / 6) return false;
  size_t column_bytes;
  if (!graph_cov_mul(kGraphCovColumnDoubles, (size_t)node_cap, &p->column_doubles)) return false;
  if (!graph_cov_mul(p->column_doubles, sizeof(double), &column_bytes)) return false;
  p->columns = 6 * n_col_nodes;
  if (p->columns == 0) return true;
  size_t per = (size_t)batch_columns;
  if (batch_columns == 0) {
    per = budget / column_bytes;
    if (per < (size_t)kGraphCovColumnsMin) per = (size_t)kGraphCovColumnsMin;
  }
  if (per > (size_t)p->columns) per = (size_t)p->columns;
  p->per_launch = (int)per;
  p->launches = (int)(((long long)p->columns + p->per_launch - 1) / p->per_launch);
  return graph_cov_mul(per, column_bytes, &p->workspace_bytes);
}
// Launch l of a plan: its first column and how many it holds.
inline void graph_cov_launch(const GraphCovPlan* p, int l, int* first, int* count) {
  *first = l * p->per_launch;
  *count = p->columns - *first < p->per_launch ? p->columns - *first : p->per_launch;
}

// The worst of two statuses (LIODOM_GRAPH_COV_*: their numbers ascend from OK to NOT_PD).
inline int32_t graph_cov_worst(int32_t a, int32_t b) { return a > b ? a : b; }

}  // namespace liodom_dev
