// graph_csr.h with switched-off edges, in a program of its own (tests/test_graph_csr_active.py builds it plain and under ASan +
// UBSan and runs it).
//   graph_csr_active_main selftest   the designed cases; prints "ok <checks>" or the line of the first check that failed (exit 1)
//   graph_csr_active_main csr N MASK i j f i j f ...
//        prints the CSR and the chain of the edges (i, j, active flag f) over N nodes: offsets, entries, parents, one line each
//        ("refused" for an index that is no node).  MASK "null": the flags are read and NOT passed on — the mask is nullptr;
//        "mask": they are passed.  Nodes are free except those named after a "fixed" word at the end: ... fixed 0 3
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "graph_csr.h"

using namespace liodom_dev;

static int g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    g_checks++;                                                              \
    if (!(cond)) { printf("failed at line %d: %s\n", __LINE__, #cond); return 1; } \
  } while (0)

typedef std::vector<int32_t> V;

static int selftest() {
  V off, ent, par;
  // a chain 0-1-2-3-4 (edges 0 .. 3), a loop 4 -> 0 (edge 4), a duplicate of the chain edge (1, 2) (edge 5); node 0 fixed
  const V ei = {0, 1, 2, 3, 4, 1}, ej = {1, 2, 3, 4, 0, 2}, fixed = {1, 0, 0, 0, 0};
  const int E = 6, N = 5;
  // the mask nullptr and a mask of ones: the same, and what it always was
  {
    V off1, ent1, par1;
    const V ones(E, 1);
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent));
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off1, &ent1, ones.data()));
    CHECK(off == off1 && ent == ent1);
    CHECK((off == V{0, 2, 5, 8, 10, 12}));
    CHECK((ent == V{0, 9, 1, 2, 10, 3, 4, 11, 5, 6, 7, 8}));
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, nullptr, &par);
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, ones.data(), &par1);
    CHECK(par == par1 && (par == V{-1, 0, 1, 2, 3}));              // node 2 hangs on edge 1, the FIRST edge (1, 2), not on 5
  }
  // all inactive: every node is a node without edges, nobody hangs on anybody
  {
    const V none(E, 0);
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent, none.data()));
    CHECK((off == V{0, 0, 0, 0, 0, 0}) && ent.empty());
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, none.data(), &par);
    CHECK((par == V{-1, -1, -1, -1, -1}));
  }
  // the chain edge (1, 2) inactive while its later duplicate is active: node 2 hangs on the duplicate, edge 5
  {
    const V act = {1, 0, 1, 1, 1, 1};
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent, act.data()));
    CHECK((off == V{0, 2, 4, 6, 8, 10}));
    CHECK((ent == V{0, 9, 1, 10, 4, 11, 5, 6, 7, 8}));           // the entries keep the original edge indices
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, act.data(), &par);
    CHECK((par == V{-1, 0, 5, 2, 3}));
  }
  // both edges (1, 2) inactive: node 2 is a root, the chain is two segments
  {
    const V act = {1, 0, 1, 1, 1, 0};
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent, act.data()));
    CHECK((off == V{0, 2, 3, 4, 6, 8}));
    CHECK((ent == V{0, 9, 1, 4, 5, 6, 7, 8}));
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, act.data(), &par);
    CHECK((par == V{-1, 0, -1, 2, 3}));
  }
  // a node left without active edges: node 3 (edges 2 and 3 off) has degree 0 and no parent; node 4 has lost its chain edge too
  {
    const V act = {1, 1, 0, 0, 1, 1};
    CHECK(graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent, act.data()));
    CHECK((off == V{0, 2, 5, 7, 7, 8}));
    CHECK((ent == V{0, 9, 1, 2, 10, 3, 11, 8}));
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, act.data(), &par);
    CHECK((par == V{-1, 0, 1, -1, -1}));
  }
  // a fixed node never hangs, whatever the mask; an edge (n - 1, n) INTO node 0 does not exist, one into a fixed node 2 is no parent
  {
    const V fx = {1, 0, 1, 0, 0}, act = {1, 1, 1, 0, 1, 1};
    graph_chain_parents(ei.data(), ej.data(), E, fx.data(), N, act.data(), &par);
    CHECK((par == V{-1, 0, -1, 2, -1}));
    graph_chain_parents(ei.data(), ej.data(), E, fx.data(), N, nullptr, &par);
    CHECK((par == V{-1, 0, -1, 2, 3}));
  }
  // an index that is no node is refused whether its edge is active or not
  {
    V bi = ei, bj = ej;
    const V act = {1, 1, 1, 1, 1, 0};
    bj[5] = N;
    CHECK(!graph_build_csr(bi.data(), bj.data(), E, N, &off, &ent, act.data()));
    bj[5] = -1;
    CHECK(!graph_build_csr(bi.data(), bj.data(), E, N, &off, &ent, act.data()));
  }
  // no edges, no nodes
  CHECK(graph_build_csr(nullptr, nullptr, 0, 0, &off, &ent, nullptr) && off.size() == 1 && ent.empty());
  graph_chain_parents(nullptr, nullptr, 0, nullptr, 0, nullptr, &par);
  CHECK(par.empty());
  // the most edges a graph takes, every other one off
  {
    V bi((size_t)kGraphMaxEdges, kGraphMaxNodes - 2), bj((size_t)kGraphMaxEdges, kGraphMaxNodes - 1), act((size_t)kGraphMaxEdges), fx((size_t)kGraphMaxNodes, 0);
    for (size_t e = 0; e < act.size(); e++) act[e] = (int32_t)(e & 1);
    CHECK(graph_build_csr(bi.data(), bj.data(), kGraphMaxEdges, kGraphMaxNodes, &off, &ent, act.data()));
    CHECK(off[kGraphMaxNodes - 1] == kGraphMaxEdges / 2 && off[kGraphMaxNodes] == kGraphMaxEdges && (int)ent.size() == kGraphMaxEdges);
    CHECK(ent[0] == 2 && ent[(size_t)kGraphMaxEdges / 2] == 3 && ent[(size_t)kGraphMaxEdges - 1] == 2 * kGraphMaxEdges - 1);
    graph_chain_parents(bi.data(), bj.data(), kGraphMaxEdges, fx.data(), kGraphMaxNodes, act.data(), &par);
    CHECK(par[(size_t)kGraphMaxNodes - 1] == 1 && par[(size_t)kGraphMaxNodes - 2] == -1);
  }
  printf("ok %d\n", g_checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "selftest") == 0) return selftest();
  if (argc >= 4 && strcmp(argv[1], "csr") == 0) {
    const int N = atoi(argv[2]);
    const bool pass_mask = strcmp(argv[3], "mask") == 0;
    V ei, ej, act, off, ent, par, fixed((size_t)(N > 0 ? N : 0), 0);
    int a = 4;
    for (; a + 2 < argc && strcmp(argv[a], "fixed") != 0; a += 3) { ei.push_back(atoi(argv[a])); ej.push_back(atoi(argv[a + 1])); act.push_back(atoi(argv[a + 2])); }
    if (a < argc && strcmp(argv[a], "fixed") == 0) {
      for (a++; a < argc; a++) { const int n = atoi(argv[a]); if (n >= 0 && n < N) fixed[(size_t)n] = 1; }
    }
    const int E = (int)ei.size();
    const int32_t* mask = pass_mask ? act.data() : nullptr;
    if (!graph_build_csr(ei.data(), ej.data(), E, N, &off, &ent, mask)) { printf("refused\n"); return 0; }
    graph_chain_parents(ei.data(), ej.data(), E, fixed.data(), N, mask, &par);
    for (int32_t v : off) printf("%d ", v);
    printf("\n");
    for (int32_t v : ent) printf("%d ", v);
    printf("\n");
    for (int32_t v : par) printf("%d ", v);
    printf("\n");
    return 0;
  }
  fprintf(stderr, "usage: graph_csr_active_main selftest | csr N null|mask i j f i j f ... [fixed n n ...]\n");
  return 2;
}
