// Stand-alone driver of the branch-and-bound search (liodom_amd/csrc/reloc_bnb.h), built plain and with -fsanitize=address,undefined
// by tests/test_reloc_bnb_driver.py.  The scores are synthetic: the search sees them only through its two callbacks.
//   search wx wy slabs batch kind seed slack
//       kind table | equal | last: a tabulated score per candidate (hashed from seed | all equal | hashed, the largest at the last
//       index); the bound of a tile is the brute-force maximum of its candidates' scores + slack.
//       kind closed: score = max(0, 1000 - (|x - cx| + |y - cy|) / 7 - 3 |slab - cs|), (cx, cy, cs) hashed from seed; the bound of a
//       tile is the score at the tile's point nearest to (cx, cy), + slack.  Nothing is tabulated.
//     prints "want <index> <score>": the exhaustive arg-max, ties to the lowest index, and
//            "best <index> <hits_r> <hits_0> rounds <r> bounded <b> scored <s> twice <candidates scored more than once> calls <bound> <exact> largest <bound call> <exact call>"
//   levels step_xy resolution radius      prints reloc_bnb_level of the widths 2^0 .. 2^31
//   count nx ny nz nyaw                   prints reloc_candidate_count under the search's limit, and the grid's wx wy slabs K
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reloc_bnb.h"

using namespace liodom_dev;

namespace {

uint64_t mix(uint64_t k) { k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33; return k; }

struct Scores {
  RelocBnbGrid g;
  int kind;      // 0 table, 1 equal, 2 last, 3 closed
  uint64_t seed;
  int64_t cx, cy, cs;
  int32_t at(int64_t slab, int64_t x, int64_t y) const {
    const int64_t i = (slab * g.wy + y) * g.wx + x;
    if (kind == 1) return 5;
    if (kind == 2 && i == g.wx * g.wy * g.slabs - 1) return 9;
    if (kind == 3) {
      const int64_t d = 1000 - (std::llabs(x - cx) + std::llabs(y - cy)) / 7 - 3 * std::llabs(slab - cs);
      return (int32_t)std::max<int64_t>(d, 0);
    }
    return (int32_t)(mix(seed + (uint64_t)i) % (kind == 2 ? 9 : 13));      // (few values: many ties)
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "levels")) {
    for (int k = 0; k < 32; k++) std::printf("%d%c", reloc_bnb_level((int64_t)1 << k, std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr), std::atoi(argv[4])), k == 31 ? '\n' : ' ');
    return 0;
  }
  if (argc == 6 && !std::strcmp(argv[1], "count")) {
    liodom_pose_search_t s = {};
    s.centre[3] = 1.0; s.step_xy = 0.4; s.step_z = 0.4; s.step_yaw = 0.02; s.radius = 1;
    s.nx = std::atoi(argv[2]); s.ny = std::atoi(argv[3]); s.nz = std::atoi(argv[4]); s.nyaw = std::atoi(argv[5]);
    const char* why = "";
    const int64_t n = reloc_candidate_count(&s, &why, kRelocBnbCandidatesMax);
    if (n <= 0) { std::printf("refused: %s\n", why); return 3; }
    const RelocBnbGrid g = reloc_bnb_grid(&s);
    std::printf("n %lld grid %lld %lld %lld %d\n", (long long)n, (long long)g.wx, (long long)g.wy, (long long)g.slabs, g.K);
    return 0;
  }
  if (argc != 9 || std::strcmp(argv[1], "search")) { std::fprintf(stderr, "usage: %s search wx wy slabs batch kind seed slack | levels ... | count ...\n", argv[0]); return 2; }
  Scores sc;
  sc.g.wx = std::atoll(argv[2]); sc.g.wy = std::atoll(argv[3]); sc.g.slabs = std::atoll(argv[4]);
  sc.g.K = 0;
  while (((int64_t)1 << sc.g.K) < std::max(sc.g.wx, sc.g.wy)) sc.g.K++;
  const int batch = std::atoi(argv[5]);
  const char* kinds[4] = {"table", "equal", "last", "closed"};
  sc.kind = -1;
  for (int k = 0; k < 4; k++) if (!std::strcmp(argv[6], kinds[k])) sc.kind = k;
  if (sc.kind < 0 || sc.g.wx < 1 || sc.g.wy < 1 || sc.g.slabs < 1) return 2;
  sc.seed = std::strtoull(argv[7], nullptr, 10);
  const int slack = std::atoi(argv[8]);
  sc.cx = (int64_t)(mix(sc.seed + 1) % (uint64_t)sc.g.wx); sc.cy = (int64_t)(mix(sc.seed + 2) % (uint64_t)sc.g.wy); sc.cs = (int64_t)(mix(sc.seed + 3) % (uint64_t)sc.g.slabs);
  const int64_t n = sc.g.wx * sc.g.wy * sc.g.slabs;
  // the exhaustive arg-max: the first of the largest
  int64_t want = 0;
  int32_t want_score = -1;
  for (int64_t s = 0; s < sc.g.slabs; s++)
    for (int64_t y = 0; y < sc.g.wy; y++)
      for (int64_t x = 0; x < sc.g.wx; x++) {
        const int32_t v = sc.at(s, x, y);
        if (v > want_score) { want_score = v; want = (s * sc.g.wy + y) * sc.g.wx + x; }
      }
  std::printf("want %lld %d\n", (long long)want, want_score);
  std::vector<bool> seen((size_t)n, false);
  int64_t twice = 0, calls[2] = {0, 0};
  size_t largest[2] = {0, 0};
  auto bound_fn = [&](const RelocBnbNode* nodes, size_t cnt, int32_t* ub) -> int {
    calls[0]++; largest[0] = std::max(largest[0], cnt);
    for (size_t i = 0; i < cnt; i++) {
      const RelocBnbNode& nd = nodes[i];
      const int64_t x1 = std::min<int64_t>((int64_t)nd.x0 + ((int64_t)1 << nd.k), sc.g.wx) - 1, y1 = std::min<int64_t>((int64_t)nd.y0 + ((int64_t)1 << nd.k), sc.g.wy) - 1;
      if (reloc_bnb_highest(sc.g, nd) != (nd.slab * sc.g.wy + y1) * sc.g.wx + x1 || x1 < nd.x0 || y1 < nd.y0 || nd.k < 0 || nd.k >= sc.g.K) return 7;
      int32_t best = 0;
      if (sc.kind == 3) {
        best = sc.at(nd.slab, std::min(std::max<int64_t>(sc.cx, nd.x0), x1), std::min(std::max<int64_t>(sc.cy, nd.y0), y1));
      } else {
        for (int64_t y = nd.y0; y <= y1; y++) for (int64_t x = nd.x0; x <= x1; x++) best = std::max(best, sc.at(nd.slab, x, y));
      }
      // split over the two counts as a kernel's would be: the search uses their sum only
      ub[2 * i] = (best + slack + 1) / 2; ub[2 * i + 1] = (best + slack) / 2;
    }
    return 0;
  };
  auto exact_fn = [&](const int64_t* index, size_t cnt, int32_t* hits) -> int {
    calls[1]++; largest[1] = std::max(largest[1], cnt);
    for (size_t i = 0; i < cnt; i++) {
      if (index[i] < 0 || index[i] >= n) return 8;
      if (seen[(size_t)index[i]]) twice++;
      seen[(size_t)index[i]] = true;
      const int64_t x = index[i] % sc.g.wx, y = (index[i] / sc.g.wx) % sc.g.wy, s = index[i] / (sc.g.wx * sc.g.wy);
      const int32_t v = sc.at(s, x, y);
      hits[2 * i] = (v + 1) / 2; hits[2 * i + 1] = v / 2;
    }
    return 0;
  };
  int32_t max_score = 0;      // what 2 * n_edges is to the library: no score is larger
  max_score = (sc.kind == 3 ? 1000 : 13) + slack;
  RelocBnbResult res;
  const int rc = reloc_bnb_search(sc.g, max_score, batch, bound_fn, exact_fn, &res);
  if (rc) { std::printf("error %d\n", rc); return 4; }
  std::printf("best %lld %d %d rounds %lld bounded %lld scored %lld twice %lld calls %lld %lld largest %zu %zu\n", (long long)res.best_index, res.hits_r, res.hits_0,
              (long long)res.rounds, (long long)res.nodes_bounded, (long long)res.candidates_scored, (long long)twice, (long long)calls[0], (long long)calls[1],
              largest[0], largest[1]);
  return 0;
}
