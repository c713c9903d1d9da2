// Stand-alone driver of map_state_validate (liodom_amd/csrc/map_state_format.h), built with -fsanitize=address,undefined by
// tests/test_map_state_format.py.  argv[1]: a good blob written by api.build_map_state (3 cells or more, the second larger than
// the first).  Every hostile case is derived from it here, handed over in a heap buffer of exactly its size (so that a read
// beyond `bytes` is a sanitizer error) and checked against the documented return code.  Exit code 0: all as documented.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "map_state_format.h"

using namespace liodom_dev;

static int g_failures = 0, g_cases = 0;
static double g_xy, g_z, g_res;

// validates a copy of b[0, len) that lives in a heap block of exactly len bytes
static int run(const std::vector<unsigned char>& b, size_t len, int max_cells, int cell_cap, double xy, double z, double res) {
  unsigned char* exact = new unsigned char[len];
  if (len) memcpy(exact, b.data(), len);
  const char* why = nullptr;
  const int rc = map_state_validate(exact, (int64_t)len, xy, z, res, max_cells, cell_cap, &why);
  if (!why || (rc != LIODOM_OK && !why[0])) { std::fprintf(stderr, "no reason given for rc %d\n", rc); g_failures++; }
  delete[] exact;
  return rc;
}
static void expect(const char* what, int got, int want) {
  g_cases++;
  if (got != want) { std::fprintf(stderr, "FAIL %s: got %d, want %d\n", what, got, want); g_failures++; }
}
template <typename T> static void poke(std::vector<unsigned char>& b, size_t off, T v) { memcpy(b.data() + off, &v, sizeof(v)); }
template <typename T> static T peek(const std::vector<unsigned char>& b, size_t off) { T v; memcpy(&v, b.data() + off, sizeof(v)); return v; }

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s good_blob\n", argv[0]); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  const std::vector<unsigned char> good((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (good.size() < 64) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  g_xy = peek<double>(good, 24); g_z = peek<double>(good, 32); g_res = peek<double>(good, 40);
  const int n = peek<int32_t>(good, 48);
  if (n < 3) { std::fprintf(stderr, "the good blob needs 3 cells or more\n"); return 2; }
  int max_count = 0;
  for (int c = 0; c < n; c++) max_count = std::max(max_count, peek<int32_t>(good, 64 + 32 * (size_t)c + 24));
  const int MC = n, CC = max_count;      // capacities that fit exactly
  auto ok = [&](const std::vector<unsigned char>& b) { return run(b, b.size(), MC, CC, g_xy, g_z, g_res); };
  const size_t rec1 = 64 + 32;           // the second cell's record

  expect("good blob", ok(good), LIODOM_OK);
  expect("good blob, larger capacities", run(good, good.size(), MC + 100, CC + 100, g_xy, g_z, g_res), LIODOM_OK);
  {
    g_cases++;
    if (map_state_validate(good.data(), (int64_t)good.size(), g_xy, g_z, g_res, MC, CC, nullptr) != LIODOM_OK) { std::fprintf(stderr, "FAIL why == null\n"); g_failures++; }
    g_cases++;
    if (map_state_validate(nullptr, 0, g_xy, g_z, g_res, MC, CC, nullptr) != LIODOM_ERR_INVALID_ARG) { std::fprintf(stderr, "FAIL null blob\n"); g_failures++; }
  }
  { // a blob at an odd address: no alignment is assumed
    std::vector<unsigned char> shifted(good.size() + 1);
    memcpy(shifted.data() + 1, good.data(), good.size());
    expect("unaligned blob", map_state_validate(shifted.data() + 1, (int64_t)good.size(), g_xy, g_z, g_res, MC, CC, nullptr), LIODOM_OK);
  }

  // every truncation length, as it is and with total_bytes patched to the new length (so that the parse goes on to the sizes)
  for (size_t len = 0; len < good.size(); len++) {
    expect("truncation", run(good, len, MC, CC, g_xy, g_z, g_res), LIODOM_ERR_INVALID_ARG);
    if (len >= 64) {
      std::vector<unsigned char> b(good.begin(), good.begin() + (long)len);
      poke<uint64_t>(b, 16, (uint64_t)len);
      expect("truncation, total_bytes patched", ok(b), LIODOM_ERR_INVALID_ARG);
    }
  }
  { std::vector<unsigned char> b = good; b.resize(b.size() + 16, 0); expect("16 bytes too long", ok(b), LIODOM_ERR_INVALID_ARG);
    poke<uint64_t>(b, 16, (uint64_t)b.size()); expect("16 bytes too long, total_bytes patched", ok(b), LIODOM_ERR_INVALID_ARG); }

  // each header field in turn
  for (int i = 0; i < 8; i++) { std::vector<unsigned char> b = good; b[(size_t)i] ^= 0x20; expect("magic", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint32_t v : {0u, 2u, 0xFFFFFFFFu}) { std::vector<unsigned char> b = good; poke<uint32_t>(b, 8, v); expect("version", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint32_t v : {0u, 63u, 65u, 128u, 0xFFFFFFFFu}) { std::vector<unsigned char> b = good; poke<uint32_t>(b, 12, v); expect("header_bytes", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint64_t v : {(uint64_t)0, (uint64_t)good.size() - 1, (uint64_t)good.size() + 1, ~(uint64_t)0}) {
    std::vector<unsigned char> b = good; poke<uint64_t>(b, 16, v); expect("total_bytes", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  for (size_t off : {(size_t)24, (size_t)32, (size_t)40}) {      // the fingerprint: bit for bit
    std::vector<unsigned char> b = good; b[off] ^= 1; expect("fingerprint, one bit", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  expect("other xy", run(good, good.size(), MC, CC, g_xy + 1.0, g_z, g_res), LIODOM_ERR_INVALID_ARG);
  expect("other z", run(good, good.size(), MC, CC, g_xy, g_z + 1.0, g_res), LIODOM_ERR_INVALID_ARG);
  expect("other resolution", run(good, good.size(), MC, CC, g_xy, g_z, g_res * 2.0), LIODOM_ERR_INVALID_ARG);
  for (int32_t v : {-1, INT32_MIN, n - 1, n + 1, 0, INT32_MAX}) { std::vector<unsigned char> b = good; poke<int32_t>(b, 48, v); expect("n_cells", ok(b), LIODOM_ERR_INVALID_ARG); }
  { std::vector<unsigned char> b = good; poke<uint32_t>(b, 52, 0xFFFFFFFFu); expect("status: any bits are a valid blob", ok(b), LIODOM_OK); }
  const int64_t np = peek<int64_t>(good, 56);
  for (int64_t v : {(int64_t)-1, np - 1, np + 1, (int64_t)0, INT64_MAX, INT64_MIN}) { std::vector<unsigned char> b = good; poke<int64_t>(b, 56, v); expect("n_points", ok(b), LIODOM_ERR_INVALID_ARG); }

  // records
  for (int32_t v : {INT32_MAX, -1, INT32_MIN}) {
    for (int c = 0; c < n; c++) {
      std::vector<unsigned char> b = good; poke<int32_t>(b, 64 + 32 * (size_t)c + 24, v); expect("count", ok(b), LIODOM_ERR_INVALID_ARG);
      b = good; poke<int32_t>(b, 64 + 32 * (size_t)c + 28, v); expect("first", ok(b), LIODOM_ERR_INVALID_ARG);
    }
  }
  { // counts that keep their sum but not the prefix; a sum that differs
    std::vector<unsigned char> b = good;
    poke<int32_t>(b, 64 + 24, peek<int32_t>(good, 64 + 24) + 1); poke<int32_t>(b, rec1 + 24, peek<int32_t>(good, rec1 + 24) - 1);
    expect("counts moved between cells", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, 64 + 32 * (size_t)(n - 1) + 24, peek<int32_t>(good, 64 + 32 * (size_t)(n - 1) + 24) + 1);
    expect("last count one more", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  for (int a = 0; a < 3; a++) {
    std::vector<unsigned char> b = good; poke<int32_t>(b, rec1 + 4 * (size_t)a, 1 << 20); expect("key 2^20", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, rec1 + 4 * (size_t)a, -(1 << 20) - 1); expect("key -2^20 - 1", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, rec1 + 4 * (size_t)a, INT32_MAX); expect("key INT32_MAX", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, rec1 + 4 * (size_t)a, INT32_MIN); expect("key INT32_MIN", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  { std::vector<unsigned char> b = good;      // the limits themselves are keys
    poke<int32_t>(b, rec1, -(1 << 20)); poke<int32_t>(b, rec1 + 4, (1 << 20) - 1); expect("keys at the limits", ok(b), LIODOM_OK); }
  for (int c = 1; c < n; c++) {
    std::vector<unsigned char> b = good; memcpy(b.data() + 64 + 32 * (size_t)c, good.data() + 64, 12); expect("duplicate key", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  { std::vector<unsigned char> b = good;      // corner_leaf is not the validator's business
    poke<int32_t>(b, rec1 + 12, INT32_MIN); poke<int32_t>(b, rec1 + 16, INT32_MAX); expect("any corner_leaf", ok(b), LIODOM_OK); }

  // capacities
  expect("max_cells one short", run(good, good.size(), MC - 1, CC, g_xy, g_z, g_res), LIODOM_ERR_CAPACITY);
  expect("cell_capacity one short", run(good, good.size(), MC, CC - 1, g_xy, g_z, g_res), LIODOM_ERR_CAPACITY);
  expect("max_cells 0", run(good, good.size(), 0, CC, g_xy, g_z, g_res), LIODOM_ERR_CAPACITY);
  { // malformed AND too large: malformed wins
    std::vector<unsigned char> b = good; memcpy(b.data() + rec1, good.data() + 64, 12);
    expect("duplicate key, max_cells short", run(b, b.size(), MC - 1, CC, g_xy, g_z, g_res), LIODOM_ERR_INVALID_ARG);
  }
  { // an empty map
    std::vector<unsigned char> b(good.begin(), good.begin() + 64);
    poke<uint64_t>(b, 16, 64); poke<int32_t>(b, 48, 0); poke<int64_t>(b, 56, 0);
    expect("0 cells", run(b, 64, 0, 0, g_xy, g_z, g_res), LIODOM_OK);
  }
  std::printf("map_state_validate: %d cases, %d failures\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
