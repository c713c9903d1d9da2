// graph_csr.h — the host-side bookkeeping of a pose graph (DESIGN.md §3 "Closing loops"): which edges a graph accepts, and the
// node -> incident (edge, side) lists its node-parallel kernels sum over.
// Plain C++, no HIP include: tests/graph_csr_main.cc compiles it for the host alone under sanitizers; liodom_graph_host.h uses it.
//
// An edge is (i, j, Z, Omega): nodes i != j, both in 0 .. n_nodes - 1; Z = [qx qy qz qw tx ty tz], finite, | |q| - 1 | <= 1e-6;
// Omega 6 x 6 row-major, finite, symmetric bit for bit.  The lists are a CSR: the pairs of node n are entries offsets[n] ..
// offsets[n + 1] - 1, each edge * 2 + side (side 0: n is the edge's i; 1: its j), in ascending edge order — so a sum over them
// depends on the graph alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace liodom_dev {

constexpr int kGraphMaxNodes = 65536;
constexpr int kGraphMaxEdges = 262144;

// 0: fine; otherwise why not (static text)
inline const char* graph_pose_refusal(const double* pose) {
  for (int k = 0; k < 7; k++) if (!isfinite(pose[k])) return "a pose has a non-finite number";
  const double n = sqrt(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3]);
  if (!(fabs(n - 1.0) <= 1e-6)) return "a pose's quaternion is not normalised (| |q| - 1 | > 1e-6)";
  return nullptr;
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
inline void graph_pose_normalised(const double* pose, double* out) {
  const double n = sqrt(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3]);
  for (int k = 0; k < 4; k++) out[k] = pose[k] / n;
  for (int k = 4; k < 7; k++) out[k] = pose[k];
}

// The CSR of n_edges edges over n_nodes nodes.  false (outputs unspecified) if an index is out of range.
inline bool graph_build_csr(const int32_t* ei, const int32_t* ej, int n_edges, int n_nodes, std::vector<int32_t>* offsets,
                            std::vector<int32_t>* entries) {
  if (n_nodes < 0 || n_edges < 0) return false;
  offsets->assign((size_t)n_nodes + 1, 0);
  entries->assign(2 * (size_t)n_edges, 0);
  for (int e = 0; e < n_edges; e++) {
    if (ei[e] < 0 || ei[e] >= n_nodes || ej[e] < 0 || ej[e] >= n_nodes) return false;
    (*offsets)[(size_t)ei[e] + 1]++;
    (*offsets)[(size_t)ej[e] + 1]++;
  }
  for (int n = 0; n < n_nodes; n++) (*offsets)[(size_t)n + 1] += (*offsets)[(size_t)n];
  std::vector<int32_t> at(offsets->begin(), offsets->end() - 1);
  for (int e = 0; e < n_edges; e++) {          // ascending e: each node's pairs come out in edge order
    (*entries)[(size_t)at[(size_t)ei[e]]++] = e * 2;
    (*entries)[(size_t)at[(size_t)ej[e]]++] = e * 2 + 1;
  }
  return true;
}

}  // namespace liodom_dev
