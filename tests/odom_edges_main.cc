// odom_edges.h in a program of its own (tests/test_odom_edges_host.py builds it plain and under ASan + UBSan and runs it).
//   selftest                                  the options and every refusal, the range rule at each edge, n at its limit -> "ok <checks>"
//   ranges first limit n (from to) x n        -> "ok", or "refused <row>"
//   limit scans_enqueued pose_log_capacity    -> the limit of the handle form
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "odom_edges.h"

using namespace liodom_dev;

static int g_checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    g_checks++;                                                         \
    if (!(c)) { printf("failed line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

static int selftest() {
  CHECK(sizeof(liodom_odom_edge_t) == 656 && sizeof(liodom_odom_edge_options_t) == 40 && sizeof(liodom_pose_cov_t) == 944);
  CHECK(offsetof(liodom_odom_edge_t, z) == 24 && offsetof(liodom_odom_edge_t, covariance) == 80 && offsetof(liodom_odom_edge_t, information) == 368);
  CHECK(kOdomEdgesMax == (1 << 20));
  // options
  liodom_odom_edge_options_t o;
  memset(&o, 0xff, sizeof(o));
  odom_edge_options_default(&o);
  CHECK(o.inflation == 1.0 && o.floor_rotation == 0.0 && o.floor_translation == 0.0);
  CHECK(o.reserved[0] == 0 && o.reserved[1] == 0 && o.reserved[2] == 0 && o.reserved[3] == 0);
  CHECK(odom_edge_options_refusal(&o) == nullptr);
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const double bad_inflation[] = {0.0, -0.0, -1.0, -1e-300, nan, inf, -inf};
  for (double v : bad_inflation) { liodom_odom_edge_options_t b = o; b.inflation = v; CHECK(odom_edge_options_refusal(&b) != nullptr); }
  const double bad_floor[] = {-1.0, -1e-300, nan, inf, -inf};
  for (double v : bad_floor) {
    { liodom_odom_edge_options_t b = o; b.floor_rotation = v; CHECK(odom_edge_options_refusal(&b) != nullptr); }
    { liodom_odom_edge_options_t b = o; b.floor_translation = v; CHECK(odom_edge_options_refusal(&b) != nullptr); }
  }
  for (int i = 0; i < 4; i++) {
    { liodom_odom_edge_options_t b = o; b.reserved[i] = 1; CHECK(odom_edge_options_refusal(&b) != nullptr); }
    { liodom_odom_edge_options_t b = o; b.reserved[i] = INT_MIN; CHECK(odom_edge_options_refusal(&b) != nullptr); }
  }
  { liodom_odom_edge_options_t b = o; b.inflation = 1e-300; b.floor_rotation = 1e300; b.floor_translation = -0.0; CHECK(odom_edge_options_refusal(&b) == nullptr); }
  { liodom_odom_edge_options_t b = o; b.inflation = 1e300; CHECK(odom_edge_options_refusal(&b) == nullptr); }
  // the limit of the handle form
  CHECK(odom_edge_log_limit(0, 32) == 0 && odom_edge_log_limit(12, 32) == 12 && odom_edge_log_limit(32, 32) == 32 && odom_edge_log_limit(33, 32) == 32);
  CHECK(odom_edge_log_limit(INT_MAX, 1024) == 1024 && odom_edge_log_limit(5, 0) == 0 && odom_edge_log_limit(-1, 32) == 0 && odom_edge_log_limit(INT_MAX, INT_MAX) == INT_MAX);
  // the range rule first <= a < b < limit, at each of its edges
  int bad = 7;
  auto one = [&](int a, int b, int first, int limit) { const int32_t f[1] = {a}, t[1] = {b}; return odom_edge_ranges_refusal(f, t, 1, first, limit, &bad) == nullptr; };
  CHECK(one(0, 1, 0, 2) && bad == -1);
  CHECK(!one(0, 1, 0, 1) && bad == 0);                 // b == limit
  CHECK(!one(0, 2, 0, 2));
  CHECK(!one(1, 1, 0, 4) && !one(2, 1, 0, 4));         // a == b, a > b
  CHECK(!one(-1, 1, 0, 4));                            // a < 0
  CHECK(one(3, 4, 3, 5) && !one(2, 4, 3, 5));          // a == first, a == first - 1
  CHECK(one(0, 11, 0, 12) && !one(0, 12, 0, 12));      // the last logged scan, one past it
  CHECK(!one(0, 1, 0, 0) && !one(0, 1, 5, 5));         // an empty log
  CHECK(one(INT_MAX - 2, INT_MAX - 1, 0, INT_MAX) && !one(INT_MAX - 1, INT_MAX, 0, INT_MAX));
  CHECK(!one(INT_MIN, INT_MAX, 0, INT_MAX) && !one(INT_MIN, 1, 0, 4));
  { const int32_t f[3] = {0, 5, 2}, t[3] = {3, 6, 9}; CHECK(odom_edge_ranges_refusal(f, t, 3, 0, 10, &bad) == nullptr && bad == -1);
    CHECK(odom_edge_ranges_refusal(f, t, 3, 0, 9, &bad) != nullptr && bad == 2);
    CHECK(odom_edge_ranges_refusal(f, t, 3, 1, 10, &bad) != nullptr && bad == 0);
    CHECK(odom_edge_ranges_refusal(f, t, 3, 0, 10, nullptr) == nullptr && odom_edge_ranges_refusal(f, t, 3, 0, 9, nullptr) != nullptr); }
  // counts
  CHECK(odom_edge_ranges_refusal(nullptr, nullptr, 0, 0, 0, &bad) == nullptr);
  CHECK(odom_edge_ranges_refusal(nullptr, nullptr, -1, 0, 10, &bad) != nullptr && odom_edge_ranges_refusal(nullptr, nullptr, INT_MIN, 0, 10, &bad) != nullptr);
  { const int32_t f[1] = {0}, t[1] = {1};
    CHECK(odom_edge_ranges_refusal(nullptr, t, 1, 0, 10, &bad) != nullptr && odom_edge_ranges_refusal(f, nullptr, 1, 0, 10, &bad) != nullptr); }
  {  // n at its limit: 2^20 intervals pass, one more is refused before a single one is read
    std::vector<int32_t> f((size_t)kOdomEdgesMax), t((size_t)kOdomEdgesMax);
    for (int i = 0; i < kOdomEdgesMax; i++) { f[(size_t)i] = i % 31; t[(size_t)i] = 31 + i % 33; }
    CHECK(odom_edge_ranges_refusal(f.data(), t.data(), kOdomEdgesMax, 0, 64, &bad) == nullptr && bad == -1);
    t[(size_t)kOdomEdgesMax - 1] = 64;
    CHECK(odom_edge_ranges_refusal(f.data(), t.data(), kOdomEdgesMax, 0, 64, &bad) != nullptr && bad == kOdomEdgesMax - 1);
    CHECK(odom_edge_ranges_refusal(f.data(), t.data(), kOdomEdgesMax + 1, 0, 64, &bad) != nullptr && bad == -1);
    CHECK(odom_edge_ranges_refusal(nullptr, nullptr, INT_MAX, 0, 64, &bad) != nullptr && bad == -1);
  }
  printf("ok %d\n", g_checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "selftest")) return selftest();
  if (argc >= 5 && !strcmp(argv[1], "ranges")) {
    const int first = atoi(argv[2]), limit = atoi(argv[3]), n = atoi(argv[4]);
    if (n < 0 || argc != 5 + 2 * n) return 2;
    std::vector<int32_t> f((size_t)n), t((size_t)n);
    for (int i = 0; i < n; i++) { f[(size_t)i] = atoi(argv[5 + 2 * i]); t[(size_t)i] = atoi(argv[6 + 2 * i]); }
    int bad = -1;
    if (odom_edge_ranges_refusal(f.data(), t.data(), n, first, limit, &bad)) printf("refused %d\n", bad); else printf("ok\n");
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "limit")) { printf("%d\n", odom_edge_log_limit(atoi(argv[2]), atoi(argv[3]))); return 0; }
  return 2;
}
