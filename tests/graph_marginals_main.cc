// graph_marginals.h in a program of its own (tests/test_graph_marginals_host.py builds it plain and under ASan + UBSan and runs it).
//   selftest                                   every refusal, the options, the plans at their limits, size overflow -> "ok <checks>"
//   anchored N f0 .. fN-1 E (i j active) x E   -> the anchored flags, or "refused"
//   columns N f0 .. fN-1 a0 .. aN-1 n q0 ..    -> the column nodes, then the slots
//   plan col_nodes node_cap batch budget       -> columns per_launch launches column_doubles workspace_bytes, or "refused"
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "graph_marginals.h"

using namespace liodom_dev;

static int g_checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    g_checks++;                                                         \
    if (!(c)) { printf("failed line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

static int selftest() {
  // options
  liodom_graph_cov_options_t o;
  memset(&o, 0xff, sizeof(o));
  graph_cov_options_default(&o);
  CHECK(o.max_pcg_iterations == 0 && o.batch_columns == 0 && o.pcg_tolerance == 1e-8);
  CHECK(graph_cov_options_refusal(&o) == nullptr);
  CHECK(sizeof(liodom_graph_cov_options_t) == 16 && sizeof(liodom_graph_cov_status_t) == 16);
  { liodom_graph_cov_options_t b = o; b.max_pcg_iterations = -1; CHECK(graph_cov_options_refusal(&b) != nullptr); }
  { liodom_graph_cov_options_t b = o; b.batch_columns = -1; CHECK(graph_cov_options_refusal(&b) != nullptr); }
  { liodom_graph_cov_options_t b = o; b.pcg_tolerance = -1e-300; CHECK(graph_cov_options_refusal(&b) != nullptr); }
  { liodom_graph_cov_options_t b = o; b.pcg_tolerance = __builtin_nan(""); CHECK(graph_cov_options_refusal(&b) != nullptr); }
  { liodom_graph_cov_options_t b = o; b.pcg_tolerance = 0.0; b.batch_columns = INT_MAX; b.max_pcg_iterations = INT_MAX; CHECK(graph_cov_options_refusal(&b) == nullptr); }
  CHECK(graph_cov_iterations(&o, 0) == 0 && graph_cov_iterations(&o, 1) == 6 && graph_cov_iterations(&o, 10922) == 65532);
  CHECK(graph_cov_iterations(&o, 10923) == 65536 && graph_cov_iterations(&o, 65536) == 65536 && graph_cov_iterations(&o, INT_MAX) == 65536);
  { liodom_graph_cov_options_t b = o; b.max_pcg_iterations = 7; CHECK(graph_cov_iterations(&b, 1000) == 7); }
  // queries
  const int32_t q[4] = {0, 3, 3, 2};
  CHECK(graph_query_refusal(q, 4, 4) == nullptr);
  CHECK(graph_query_refusal(q, 4, 3) != nullptr);
  CHECK(graph_query_refusal(nullptr, 0, 0) == nullptr && graph_query_refusal(q, 0, 0) == nullptr);
  CHECK(graph_query_refusal(nullptr, 1, 4) != nullptr);
  CHECK(graph_query_refusal(q, -1, 4) != nullptr);
  { const int32_t neg[1] = {-1}; CHECK(graph_query_refusal(neg, 1, 4) != nullptr); }
  { const int32_t big[1] = {INT_MAX - 1}; CHECK(graph_query_refusal(big, 1, INT_MAX) == nullptr && graph_query_refusal(big, 1, 65536) != nullptr); }
  // anchoring: refusals and the empty graph
  std::vector<int32_t> anc;
  { const int32_t ei[1] = {0}, ej[1] = {2}, fx[2] = {1, 0}; CHECK(!graph_anchored(ei, ej, 1, nullptr, fx, 2, &anc)); }
  { const int32_t ei[1] = {-1}, ej[1] = {0}, fx[2] = {1, 0}; CHECK(!graph_anchored(ei, ej, 1, nullptr, fx, 2, &anc)); }
  CHECK(!graph_anchored(nullptr, nullptr, -1, nullptr, nullptr, 0, &anc) && !graph_anchored(nullptr, nullptr, 0, nullptr, nullptr, -1, &anc));
  CHECK(graph_anchored(nullptr, nullptr, 0, nullptr, nullptr, 0, &anc) && anc.empty());
  { const int32_t fx[3] = {0, 1, 0}; CHECK(graph_anchored(nullptr, nullptr, 0, nullptr, fx, 3, &anc) && anc[0] == 0 && anc[1] == 1 && anc[2] == 0); }
  {  // a chain of 65 536 nodes fixed at its far end, edges in an order that makes long paths
    const int N = 65536;
    std::vector<int32_t> ei, ej, fx((size_t)N, 0);
    for (int k = N - 2; k >= 0; k--) { ei.push_back(k + 1); ej.push_back(k); }
    fx[(size_t)N - 1] = 1;
    CHECK(graph_anchored(ei.data(), ej.data(), N - 1, nullptr, fx.data(), N, &anc));
    bool all = true;
    for (int k = 0; k < N; k++) all = all && anc[(size_t)k] == 1;
    CHECK(all);
    std::vector<int32_t> act((size_t)N - 1, 1);
    act[100] = 0;                                      // cuts edge (N - 101, N - 102): the nodes below lose the anchor
    CHECK(graph_anchored(ei.data(), ej.data(), N - 1, act.data(), fx.data(), N, &anc));
    CHECK(anc[(size_t)N - 101] == 1 && anc[(size_t)N - 102] == 0 && anc[0] == 0);
  }
  // column nodes
  {
    const int32_t fx[6] = {1, 0, 0, 0, 0, 0}, an[6] = {1, 1, 1, 0, 1, 1}, qq[8] = {4, 0, 2, 4, 3, 2, 5, 4};
    std::vector<int32_t> cn, sl;
    graph_column_nodes(qq, 8, fx, an, 6, &cn, &sl);
    CHECK(cn.size() == 3 && cn[0] == 4 && cn[1] == 2 && cn[2] == 5);
    CHECK(sl.size() == 6 && sl[0] == -1 && sl[1] == -1 && sl[2] == 1 && sl[3] == -1 && sl[4] == 0 && sl[5] == 2);
    graph_column_nodes(nullptr, 0, fx, an, 6, &cn, &sl);
    CHECK(cn.empty() && sl.size() == 6 && sl[4] == -1);
    graph_column_nodes(nullptr, 0, nullptr, nullptr, 0, &cn, &sl);
    CHECK(cn.empty() && sl.empty());
  }
  // plans
  GraphCovPlan p;
  const size_t B = kGraphCovWorkspaceBudget;
  CHECK(B == (size_t)256 << 20);
  for (int batch : {1, 6, 7}) {
    CHECK(graph_cov_plan(3, 1030, batch, B, &p));
    CHECK(p.columns == 18 && p.per_launch == batch && p.launches == (18 + batch - 1) / batch);
    CHECK(p.column_doubles == (size_t)30 * 1030 && p.workspace_bytes == (size_t)batch * 30 * 1030 * 8);
    int covered = 0;
    for (int l = 0; l < p.launches; l++) {
      int first, count;
      graph_cov_launch(&p, l, &first, &count);
      CHECK(first == covered && count >= 1 && count <= batch);
      covered += count;
    }
    CHECK(covered == 18);
  }
  CHECK(graph_cov_plan(1, 8, 1000, B, &p) && p.per_launch == 6 && p.launches == 1);          // no more than there are
  CHECK(graph_cov_plan(0, 8, 0, B, &p) && p.columns == 0 && p.launches == 0 && p.workspace_bytes == 0);
  // auto: node_cap 1 — everything fits; 4096 — 273 columns fit; 65 536 — 17 fit; a budget of nothing — the minimum of 6
  CHECK(graph_cov_plan(1, 1, 0, B, &p) && p.per_launch == 6 && p.launches == 1 && p.workspace_bytes == 6 * 240);
  CHECK(graph_cov_plan(4096, 4096, 0, B, &p) && p.columns == 24576 && p.per_launch == 273 && p.launches == 91 && p.workspace_bytes <= B);
  CHECK(graph_cov_plan(40, 4096, 0, B, &p) && p.per_launch == 240 && p.launches == 1);
  CHECK(graph_cov_plan(65536, 65536, 0, B, &p) && p.columns == 393216 && p.per_launch == 17 && p.launches == 23131 && p.workspace_bytes == (size_t)17 * 30 * 65536 * 8);
  { int first, count; graph_cov_launch(&p, 23130, &first, &count); CHECK(first == 393210 && count == 6); }
  CHECK(graph_cov_plan(65536, 65536, 0, 0, &p) && p.per_launch == 6 && p.workspace_bytes == (size_t)6 * 30 * 65536 * 8);
  CHECK(graph_cov_plan(1, 65536, 0, 0, &p) && p.per_launch == 6 && p.launches == 1);
  // refusals and overflow
  CHECK(!graph_cov_plan(-1, 8, 0, B, &p) && !graph_cov_plan(1, 0, 0, B, &p) && !graph_cov_plan(1, -5, 0, B, &p) && !graph_cov_plan(1, 8, -1, B, &p));
  CHECK(!graph_cov_plan(INT_MAX / 6 + 1, 8, 0, B, &p));                                        // 6 x nodes beyond an int
  CHECK(graph_cov_plan(INT_MAX / 6, 8, 0, B, &p) && p.columns == INT_MAX / 6 * 6);
  CHECK(!graph_cov_plan(1, LLONG_MAX, 0, B, &p));                                              // 30 x node_cap beyond size_t
  CHECK(!graph_cov_plan(1, (long long)((size_t)-1 / 30), 0, B, &p));                           // ... fits, x 8 does not
  CHECK(!graph_cov_plan(INT_MAX / 6, (long long)1 << 54, INT_MAX, B, &p));                     // one column fits, the launch's do not
  CHECK(graph_cov_plan(1, (long long)1 << 54, 1, B, &p) && p.workspace_bytes == ((size_t)30 * 8) << 54);
  { size_t r; CHECK(graph_cov_mul(0, (size_t)-1, &r) && r == 0 && graph_cov_mul((size_t)-1, 1, &r) && r == (size_t)-1 && !graph_cov_mul((size_t)-1, 2, &r)); }
  CHECK(graph_cov_worst(0, 3) == 3 && graph_cov_worst(4, 2) == 4 && graph_cov_worst(1, 1) == 1);
  CHECK(LIODOM_GRAPH_COV_OK < LIODOM_GRAPH_COV_NOT_CONVERGED && LIODOM_GRAPH_COV_NOT_CONVERGED < LIODOM_GRAPH_COV_BREAKDOWN &&
        LIODOM_GRAPH_COV_BREAKDOWN < LIODOM_GRAPH_COV_UNANCHORED && LIODOM_GRAPH_COV_UNANCHORED < LIODOM_GRAPH_COV_NOT_PD);
  printf("ok %d\n", g_checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  int at = 2;
  auto next = [&]() -> long long { return at < argc ? atoll(argv[at++]) : 0; };
  if (mode == "selftest") return selftest();
  if (mode == "anchored") {
    const int N = (int)next();
    std::vector<int32_t> fx((size_t)N);
    for (int k = 0; k < N; k++) fx[(size_t)k] = (int32_t)next();
    const int E = (int)next();
    std::vector<int32_t> ei((size_t)E), ej((size_t)E), act((size_t)E);
    for (int e = 0; e < E; e++) { ei[(size_t)e] = (int32_t)next(); ej[(size_t)e] = (int32_t)next(); act[(size_t)e] = (int32_t)next(); }
    std::vector<int32_t> anc;
    if (!graph_anchored(ei.data(), ej.data(), E, act.data(), fx.data(), N, &anc)) { printf("refused\n"); return 0; }
    for (int k = 0; k < N; k++) printf("%d ", anc[(size_t)k]);
    printf("\n");
    return 0;
  }
  if (mode == "columns") {
    const int N = (int)next();
    std::vector<int32_t> fx((size_t)N), an((size_t)N);
    for (int k = 0; k < N; k++) fx[(size_t)k] = (int32_t)next();
    for (int k = 0; k < N; k++) an[(size_t)k] = (int32_t)next();
    const int n = (int)next();
    std::vector<int32_t> q((size_t)n), cn, sl;
    for (int k = 0; k < n; k++) q[(size_t)k] = (int32_t)next();
    if (graph_query_refusal(q.data(), n, N)) { printf("refused\n"); return 0; }
    graph_column_nodes(q.data(), n, fx.data(), an.data(), N, &cn, &sl);
    for (int32_t v : cn) printf("%d ", v);
    printf("\n");
    for (int32_t v : sl) printf("%d ", v);
    printf("\n");
    return 0;
  }
  if (mode == "plan") {
    const int cols = (int)next();
    const long long cap = next();
    const int batch = (int)next();
    const size_t budget = (size_t)next();
    GraphCovPlan p;
    if (!graph_cov_plan(cols, cap, batch, budget, &p)) { printf("refused\n"); return 0; }
    printf("%d %d %d %zu %zu\n", p.columns, p.per_launch, p.launches, p.column_doubles, p.workspace_bytes);
    return 0;
  }
  return 2;
}
