// Stand-alone driver of map_state_split / map_state_join (liodom_amd/csrc/map_state_cells.h), built with
// -fsanitize=address,undefined by tests/test_map_state_cells.py.  argv[1]: a good blob written by api.build_map_state (3 cells or
// more).  Every blob is handed over in a heap buffer of exactly its size, so that a read beyond `bytes` is a sanitizer error.
// Exit code 0: all as documented.
#include <climits>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "map_state_cells.h"

using namespace liodom_dev;

static int g_failures = 0, g_cases = 0;
static void expect(const char* what, bool ok) {
  g_cases++;
  if (!ok) { std::fprintf(stderr, "FAIL %s\n", what); g_failures++; }
}
template <typename T> static void poke(std::vector<unsigned char>& b, size_t off, T v) { memcpy(b.data() + off, &v, sizeof(v)); }
template <typename T> static T peek(const std::vector<unsigned char>& b, size_t off) { T v; memcpy(&v, b.data() + off, sizeof(v)); return v; }

static double g_xy, g_z, g_res;
// splits a copy of b[0, len) that lives in a heap block of exactly len bytes
static int split(const std::vector<unsigned char>& b, size_t len, std::vector<MapStateCell>* cells, uint32_t* status) {
  unsigned char* exact = new unsigned char[len];
  if (len) memcpy(exact, b.data(), len);
  const char* why = nullptr;
  const int rc = map_state_split(exact, (int64_t)len, g_xy, g_z, g_res, cells, status, &why);
  if (!why || (rc != LIODOM_OK && !why[0])) { std::fprintf(stderr, "no reason given for rc %d\n", rc); g_failures++; }
  delete[] exact;
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s good_blob\n", argv[0]); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<unsigned char> good((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (good.size() < 64) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  g_xy = peek<double>(good, 24); g_z = peek<double>(good, 32); g_res = peek<double>(good, 40);
  const int n = peek<int32_t>(good, 48);
  if (n < 3) { std::fprintf(stderr, "the good blob needs 3 cells or more\n"); return 2; }

  std::vector<MapStateCell> cells;
  uint32_t status = 77;
  expect("good blob splits", split(good, good.size(), &cells, &status) == LIODOM_OK && (int)cells.size() == n && status == peek<uint32_t>(good, 52));
  int64_t pts = 0;
  for (int c = 0; c < n; c++) {
    const size_t rec = 64 + 32 * (size_t)c;
    expect("cell record", cells[(size_t)c].count() == peek<int32_t>(good, rec + 24) && cells[(size_t)c].key[1] == peek<int32_t>(good, rec + 4) &&
                              cells[(size_t)c].corner_leaf[2] == peek<int32_t>(good, rec + 20));
    expect("cell points", cells[(size_t)c].count() == 0 ||
                              memcmp(cells[(size_t)c].xyzi.data(), good.data() + 64 + 32 * (size_t)n + 16 * (size_t)pts, 16 * (size_t)cells[(size_t)c].count()) == 0);
    pts += cells[(size_t)c].count();
  }
  {  // join after split is the identity
    std::vector<const MapStateCell*> ptrs;
    for (const MapStateCell& c : cells) ptrs.push_back(&c);
    expect("join(split) == blob", map_state_join(g_xy, g_z, g_res, ptrs, status) == good);
    // a subset in another order, and nothing at all, are well-formed blobs
    std::vector<const MapStateCell*> some{&cells[2], &cells[0]};
    const std::vector<unsigned char> sub = map_state_join(g_xy, g_z, g_res, some, 5);
    std::vector<MapStateCell> again;
    uint32_t st2 = 0;
    expect("subset splits", split(sub, sub.size(), &again, &st2) == LIODOM_OK && again.size() == 2 && st2 == 5 && again[0].key == cells[2].key &&
                                again[1].xyzi == cells[0].xyzi && again[0].corner_leaf == cells[2].corner_leaf);
    const std::vector<unsigned char> none = map_state_join(g_xy, g_z, g_res, {}, 0);
    expect("0 cells", none.size() == 64 && split(none, 64, &again, &st2) == LIODOM_OK && again.empty());
    MapStateCell empty_cell;
    empty_cell.key = {{1, 2, 3}};
    std::vector<const MapStateCell*> with_empty{&cells[1], &empty_cell, &cells[0]};
    const std::vector<unsigned char> we = map_state_join(g_xy, g_z, g_res, with_empty, 0);
    expect("an empty cell travels", split(we, we.size(), &again, nullptr) == LIODOM_OK && again.size() == 3 && again[1].count() == 0 && again[2].xyzi == cells[0].xyzi);
    expect("null outputs", split(good, good.size(), nullptr, nullptr) == LIODOM_OK);
  }
  // hostile bytes: rejected before anything is read, and `cells` comes back empty
  for (size_t len = 0; len < good.size(); len++) {
    std::vector<MapStateCell> out(1);
    expect("truncation", split(good, len, &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty());
    if (len >= 64) {
      std::vector<unsigned char> b(good.begin(), good.begin() + (long)len);
      poke<uint64_t>(b, 16, (uint64_t)len);
      expect("truncation, total_bytes patched", split(b, b.size(), &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty());
    }
  }
  for (int32_t v : {INT32_MAX, -1, INT32_MIN}) {
    for (int c = 0; c < n; c++) {
      std::vector<MapStateCell> out(1);
      std::vector<unsigned char> b = good; poke<int32_t>(b, 64 + 32 * (size_t)c + 24, v);
      expect("count", split(b, b.size(), &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty());
      b = good; poke<int32_t>(b, 64 + 32 * (size_t)c + 28, v);
      expect("first", split(b, b.size(), &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty());
    }
  }
  for (int32_t v : {-1, n - 1, n + 1, INT32_MAX}) {
    std::vector<MapStateCell> out(1);
    std::vector<unsigned char> b = good; poke<int32_t>(b, 48, v);
    expect("n_cells", split(b, b.size(), &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty());
  }
  { std::vector<MapStateCell> out(1); std::vector<unsigned char> b = good; b[24] ^= 1;
    expect("other sizes", split(b, b.size(), &out, nullptr) == LIODOM_ERR_INVALID_ARG && out.empty()); }
  std::printf("map_state_cells: %d cases, %d failures\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
