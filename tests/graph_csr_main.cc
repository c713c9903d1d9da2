// graph_csr.h in a program of its own (tests/test_graph_csr.py builds it plain and under ASan + UBSan and runs it).
//   graph_csr_main selftest            every refusal of an edge and of a pose, degrees 0, 1 and 1025, the maximal indices; prints
//                                      "ok <checks>" or the line of the first check that failed (exit 1)
//   graph_csr_main csr N i j i j ...   prints the CSR of the edges over N nodes: the offsets on one line, the entries on the next
//                                      ("refused" for an index that is no node)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>

#include "graph_csr.h"

using namespace liodom_dev;

static int g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    g_checks++;                                                              \
    if (!(cond)) { printf("failed at line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

static void identity_info(double* info) {
  for (int k = 0; k < 36; k++) info[k] = (k % 7 == 0) ? 2.0 : 0.0;
}

static int selftest() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double z[7] = {0, 0, 0, 1, 1, 2, 3}, info[36];
  identity_info(info);
  // an edge that is fine, at the smallest and at the largest indices
  CHECK(graph_edge_refusal(0, 1, z, info, 2) == nullptr);
  CHECK(graph_edge_refusal(kGraphMaxNodes - 1, 0, z, info, kGraphMaxNodes) == nullptr);
  CHECK(graph_edge_refusal(0, kGraphMaxNodes - 1, z, info, kGraphMaxNodes) == nullptr);
  // indices
  CHECK(graph_edge_refusal(-1, 1, z, info, 2) != nullptr);
  CHECK(graph_edge_refusal(0, -1, z, info, 2) != nullptr);
  CHECK(graph_edge_refusal(2, 1, z, info, 2) != nullptr);
  CHECK(graph_edge_refusal(0, 2, z, info, 2) != nullptr);
  CHECK(graph_edge_refusal(0, 1, z, info, 0) != nullptr);
  CHECK(graph_edge_refusal(std::numeric_limits<int32_t>::max(), 0, z, info, kGraphMaxNodes) != nullptr);
  CHECK(graph_edge_refusal(std::numeric_limits<int32_t>::min(), 0, z, info, kGraphMaxNodes) != nullptr);
  CHECK(graph_edge_refusal(1, 1, z, info, 2) != nullptr);
  // Z
  for (int k = 0; k < 7; k++) {
    for (double bad : {nan, inf, -inf}) {
      double zz[7];
      memcpy(zz, z, sizeof(zz));
      zz[k] = bad;
      CHECK(graph_edge_refusal(0, 1, zz, info, 2) != nullptr);
      CHECK(graph_pose_refusal(zz) != nullptr);
    }
  }
  {
    double zz[7] = {0, 0, 0, 1.0 + 0.9e-6, 0, 0, 0};
    CHECK(graph_edge_refusal(0, 1, zz, info, 2) == nullptr);
    zz[3] = 1.0 - 0.9e-6;
    CHECK(graph_edge_refusal(0, 1, zz, info, 2) == nullptr);
    zz[3] = 1.0 + 1.1e-6;
    CHECK(graph_edge_refusal(0, 1, zz, info, 2) != nullptr);
    zz[3] = 1.0 - 1.1e-6;
    CHECK(graph_edge_refusal(0, 1, zz, info, 2) != nullptr);
    zz[3] = 0.0;
    CHECK(graph_edge_refusal(0, 1, zz, info, 2) != nullptr);
    double out[7], q[7] = {0.6 * (1 + 5e-7), 0, 0, 0.8 * (1 + 5e-7), 7, 8, 9};
    CHECK(graph_pose_refusal(q) == nullptr);
    graph_pose_normalised(q, out);
    CHECK(fabs(sqrt(out[0] * out[0] + out[3] * out[3]) - 1.0) <= 3e-16 && out[4] == 7 && out[5] == 8 && out[6] == 9);
  }
  // Omega
  for (int k = 0; k < 36; k++) {
    for (double bad : {nan, inf, -inf}) {
      double om[36];
      identity_info(om);
      om[k] = bad;
      CHECK(graph_edge_refusal(0, 1, z, om, 2) != nullptr);
    }
  }
  for (int r = 0; r < 6; r++) {
    for (int c = r + 1; c < 6; c++) {
      double om[36];
      identity_info(om);
      om[r * 6 + c] = 0.25; om[c * 6 + r] = 0.25;
      CHECK(graph_edge_refusal(0, 1, z, om, 2) == nullptr);
      om[c * 6 + r] = nextafter(0.25, 1.0);                       // one bit apart
      CHECK(graph_edge_refusal(0, 1, z, om, 2) != nullptr);
      om[r * 6 + c] = 0.0; om[c * 6 + r] = -0.0;                  // equal as numbers, not as bits
      CHECK(graph_edge_refusal(0, 1, z, om, 2) != nullptr);
    }
  }
  {
    double om[36];                                                // an indefinite Omega is the solver's to find, not this check's
    identity_info(om);
    om[0] = -1.0;
    CHECK(graph_edge_refusal(0, 1, z, om, 2) == nullptr);
  }
  // the CSR: nothing at all
  std::vector<int32_t> off, ent;
  CHECK(graph_build_csr(nullptr, nullptr, 0, 0, &off, &ent) && off.size() == 1 && off[0] == 0 && ent.empty());
  CHECK(!graph_build_csr(nullptr, nullptr, -1, 0, &off, &ent));
  // a hub of degree 1025 at node 3 (alternating sides), a node of degree 0 (node 1), leaves of degree 1, the largest node index
  {
    const int N = kGraphMaxNodes, deg = 1025;
    std::vector<int32_t> ei, ej;
    for (int k = 0; k < deg; k++) {
      const int leaf = (k == deg - 1) ? N - 1 : 10 + k;
      if (k % 2 == 0) { ei.push_back(3); ej.push_back(leaf); } else { ei.push_back(leaf); ej.push_back(3); }
    }
    CHECK(graph_build_csr(ei.data(), ej.data(), deg, N, &off, &ent));
    CHECK((int)off.size() == N + 1 && (int)ent.size() == 2 * deg && off[N] == 2 * deg);
    CHECK(off[4] - off[3] == deg && off[2] - off[1] == 0 && off[11] - off[10] == 1 && off[N] - off[N - 1] == 1);
    for (int k = 0; k < deg; k++) CHECK(ent[(size_t)off[3] + (size_t)k] == k * 2 + (k % 2));             // edge order, the hub's side
    CHECK(ent[(size_t)off[N - 1]] == (deg - 1) * 2 + 1);                                                  // the leaf is the j of edge 1024
    for (int n = 0; n < N; n++) CHECK(off[(size_t)n] <= off[(size_t)n + 1]);
    std::vector<int> seen(2 * (size_t)deg, 0);
    for (int32_t v : ent) { CHECK(v >= 0 && v < 2 * deg); seen[(size_t)v]++; }
    for (int v : seen) CHECK(v == 1);
    ej[5] = N;                                                    // an index that is no node
    CHECK(!graph_build_csr(ei.data(), ej.data(), deg, N, &off, &ent));
    ej[5] = -1;
    CHECK(!graph_build_csr(ei.data(), ej.data(), deg, N, &off, &ent));
  }
  // the most edges a graph takes, all between the two largest indices
  {
    std::vector<int32_t> ei((size_t)kGraphMaxEdges, kGraphMaxNodes - 2), ej((size_t)kGraphMaxEdges, kGraphMaxNodes - 1);
    CHECK(graph_build_csr(ei.data(), ej.data(), kGraphMaxEdges, kGraphMaxNodes, &off, &ent));
    CHECK(off[kGraphMaxNodes - 2] == 0 && off[kGraphMaxNodes - 1] == kGraphMaxEdges && off[kGraphMaxNodes] == 2 * kGraphMaxEdges);
    CHECK(ent[0] == 0 && ent[(size_t)kGraphMaxEdges - 1] == 2 * (kGraphMaxEdges - 1) && ent[(size_t)kGraphMaxEdges] == 1 &&
          ent[2 * (size_t)kGraphMaxEdges - 1] == 2 * kGraphMaxEdges - 1);
  }
  printf("ok %d\n", g_checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "selftest") == 0) return selftest();
  if (argc >= 3 && strcmp(argv[1], "csr") == 0 && (argc - 3) % 2 == 0) {
    const int N = atoi(argv[2]), E = (argc - 3) / 2;
    std::vector<int32_t> ei, ej, off, ent;
    for (int e = 0; e < E; e++) { ei.push_back(atoi(argv[3 + 2 * e])); ej.push_back(atoi(argv[4 + 2 * e])); }
    if (!graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent)) { printf("refused\n"); return 0; }
    for (int32_t v : off) printf("%d ", v);
    printf("\n");
    for (int32_t v : ent) printf("%d ", v);
    printf("\n");
    return 0;
  }
  fprintf(stderr, "usage: graph_csr_main selftest | csr N i j i j ...\n");
  return 2;
}
