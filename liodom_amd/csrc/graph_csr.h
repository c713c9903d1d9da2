// graph_csr.h — the host-side bookkeeping of a pose graph (DESIGN.md §3 "Closing loops"): which edges a graph accepts, and the
// node -> incident (edge, side) lists its node-parallel kernels sum over.
// Plain C++, no HIP include: tests/graph_csr_main.cc and tests/graph_csr_active_main.cc compile it for the host alone under sanitizers; liodom_graph_host.h uses it.
//
// An edge is (i, j, Z, Omega): nodes i != j, both in 0 .. n_nodes - 1; Z = [qx qy qz qw tx ty tz] as pose7.h takes it;
// Omega 6 x 6 row-major, finite, symmetric bit for bit.  The lists are a CSR: the pairs of node n are entries offsets[n] ..
// offsets[n + 1] - 1, each edge * 2 + side (side 0: n is the edge's i; 1: its j), in ascending edge order — so a sum over them
// depends on the graph alone.  An edge can be switched off (liodom_graph_set_edge_active): the lists and the preconditioner's
// chain are made of the active edges only.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pose7.h"

namespace liodom_dev {

constexpr int kGraphMaxNodes = 65536;
constexpr int kGraphMaxEdges = 262144;
constexpr int kGraphLossKinds = 16;           // a graph keeps a loss per edge kind 0 .. 15 (liodom_graph_set_loss)

// 0: fine; otherwise why not (static text)
inline const char* graph_pose_refusal(const double* pose) {
  const Pose7Verdict v = pose7_check(pose);
  return v == kPose7Ok ? nullptr : v == kPose7NonFinite ? "a pose has a non-finite number" : "a pose's quaternion is not normalised (" POSE7_RULE ")";
}
inline const char* graph_edge_refusal(int32_t i, int32_t j, const double* z, const double* info, int n_nodes) {
  if (i < 0 || j < 0 || i >= n_nodes || j >= n_nodes) return "an edge names a node that does not exist";
  if (i == j) return "an edge joins a node to itself";
  if (const char* why = graph_pose_refusal(z)) return why;
  for (int k = 0; k < 36; k++) if (!isfinite(info[k])) return "an information matrix has a non-finite number";
  for (int r = 0; r < 6; r++)
    for (int c = r + 1; c < 6; c++) {
      if (memcmp(&info[r * 6 + c], &info[c * 6 + r], sizeof(double)) != 0) return "an information matrix is not symmetric bit for bit";
    }
  return nullptr;
}
// pose with its quaternion divided by its norm (after graph_pose_refusal has passed)
inline void graph_pose_normalised(const double* pose, double* out) { pose7_normalised(pose, out); }

// The CSR of n_edges edges over n_nodes nodes.  false (outputs unspecified) if an index is out of range.  active (optional,
// [n_edges]; null: every edge): an edge whose flag is 0 is left out — it is in no node's list, so it adds nothing to a node's
// sums or degree — and the entries keep the ORIGINAL edge indices; entries then holds two per active edge.
inline bool graph_build_csr(const int32_t* ei, const int32_t* ej, int n_edges, int n_nodes, std::vector<int32_t>* offsets,
                            std::vector<int32_t>* entries, const int32_t* active = nullptr) {
  if (n_nodes < 0 || n_edges < 0) return false;
  offsets->assign((size_t)n_nodes + 1, 0);
  size_t n_active = 0;
  for (int e = 0; e < n_edges; e++) {
    if (ei[e] < 0 || ei[e] >= n_nodes || ej[e] < 0 || ej[e] >= n_nodes) return false;
    if (active && !active[e]) continue;
    (*offsets)[(size_t)ei[e] + 1]++;
    (*offsets)[(size_t)ej[e] + 1]++;
    n_active++;
  }
  entries->assign(2 * n_active, 0);
  for (int n = 0; n < n_nodes; n++) (*offsets)[(size_t)n + 1] += (*offsets)[(size_t)n];
  std::vector<int32_t> at(offsets->begin(), offsets->end() - 1);
  for (int e = 0; e < n_edges; e++) {          // ascending e: each node's pairs come out in edge order
    if (active && !active[e]) continue;
    (*entries)[(size_t)at[(size_t)ei[e]]++] = e * 2;
    (*entries)[(size_t)at[(size_t)ej[e]]++] = e * 2 + 1;
  }
  return true;
}

// The chain the preconditioner works along (kernels_graph.h "the preconditioner"): parent[n] = the first active edge (n - 1, n)
// of a free node n, -1 where there is none (a fixed node, node 0, a node whose edges (n - 1, n) are all switched off).  The
// indices must have passed graph_build_csr.  active as there.
inline void graph_chain_parents(const int32_t* ei, const int32_t* ej, int n_edges, const int32_t* fixed, int n_nodes,
                                const int32_t* active, std::vector<int32_t>* parent) {
  parent->assign((size_t)(n_nodes > 0 ? n_nodes : 0), -1);
  for (int e = n_edges - 1; e >= 0; e--) {      // descending e: the first such edge is the one that stays
    if (active && !active[e]) continue;
    if (ej[e] == ei[e] + 1 && !fixed[ej[e]]) (*parent)[(size_t)ej[e]] = e;
  }
}

}  // namespace liodom_dev
