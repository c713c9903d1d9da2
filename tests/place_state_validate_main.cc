// Stand-alone driver of place_state_validate (liodom_amd/csrc/place_state_format.h), built with -fsanitize=address,undefined by
// tests/test_place_state_format.py.  argv[1]: a good blob written by api.build_place_state (3 places or more, a geometry of 2 words or
// more).  Every hostile case is derived from it here, handed over in a heap buffer of exactly its size (so that a read beyond
// `bytes` is a sanitizer error) and checked against the documented return code.  Exit code 0: all as documented.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <vector>

#include "place_state_format.h"

using namespace liodom_dev;

static int g_failures = 0, g_cases = 0;

static int run(const std::vector<unsigned char>& b, size_t len, const int32_t* nm, const double* rz, int64_t max_places) {
  unsigned char* exact = new unsigned char[len ? len : 1];
  if (len) memcpy(exact, b.data(), len);
  const char* why = nullptr;
  const int rc = place_state_validate(len ? exact : nullptr, (int64_t)len, nm, rz, max_places, &why);
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
  const size_t head = (size_t)kPlaceStateHeaderBytes + (size_t)kPlaceTablesBytes;
  if (good.size() < head) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int32_t nm[2] = {peek<int32_t>(good, 24), peek<int32_t>(good, 28)};
  const double rz[3] = {peek<double>(good, 32), peek<double>(good, 40), peek<double>(good, 48)};
  const int n = peek<int32_t>(good, 56);
  const size_t W = (size_t)nm[0] * (size_t)nm[1];
  if (n < 3 || W < 2) { std::fprintf(stderr, "the good blob needs 3 places and 2 words or more\n"); return 2; }
  const size_t recs = head + 8 * W * (size_t)n;
  auto ok = [&](const std::vector<unsigned char>& b) { return run(b, b.size(), nm, rz, n); };

  expect("good blob", ok(good), LIODOM_OK);
  expect("good blob, larger capacity", run(good, good.size(), nm, rz, n + 100), LIODOM_OK);
  expect("good blob, no geometry given", run(good, good.size(), nullptr, nullptr, n), LIODOM_OK);
  expect("good blob, no capacity check", run(good, good.size(), nm, rz, -1), LIODOM_OK);
  {
    g_cases++;
    if (place_state_validate(good.data(), (int64_t)good.size(), nm, rz, n, nullptr) != LIODOM_OK) { std::fprintf(stderr, "FAIL why == null\n"); g_failures++; }
    g_cases++;
    if (place_state_validate(nullptr, 0, nm, rz, n, nullptr) != LIODOM_ERR_INVALID_ARG) { std::fprintf(stderr, "FAIL null blob\n"); g_failures++; }
  }
  { // a blob at an odd address: no alignment is assumed
    std::vector<unsigned char> shifted(good.size() + 1);
    memcpy(shifted.data() + 1, good.data(), good.size());
    expect("unaligned blob", place_state_validate(shifted.data() + 1, (int64_t)good.size(), nm, rz, n, nullptr), LIODOM_OK);
  }

  // every truncation length, as it is and with total_bytes patched to the new length (so that the parse goes on to the sizes)
  for (size_t len = 0; len < good.size(); len++) {
    expect("truncation", run(good, len, nm, rz, n), LIODOM_ERR_INVALID_ARG);
    if (len >= 64) {
      std::vector<unsigned char> b(good.begin(), good.begin() + (long)len);
      poke<uint64_t>(b, 16, (uint64_t)len);
      expect("truncation, total_bytes patched", ok(b), LIODOM_ERR_INVALID_ARG);
    }
  }
  { std::vector<unsigned char> b = good; b.resize(b.size() + 8, 0); expect("8 bytes too long", ok(b), LIODOM_ERR_INVALID_ARG);
    poke<uint64_t>(b, 16, (uint64_t)b.size()); expect("8 bytes too long, total_bytes patched", ok(b), LIODOM_ERR_INVALID_ARG); }

  // each header field in turn
  for (int i = 0; i < 8; i++) { std::vector<unsigned char> b = good; b[(size_t)i] ^= 0x20; expect("magic", ok(b), LIODOM_ERR_INVALID_ARG); }
  { std::vector<unsigned char> b = good; memcpy(b.data(), "LIODOMMP", 8); expect("a map blob's magic", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint32_t v : {0u, 2u, 0xFFFFFFFFu}) { std::vector<unsigned char> b = good; poke<uint32_t>(b, 8, v); expect("version", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint32_t v : {0u, 63u, 65u, 720u, 0xFFFFFFFFu}) { std::vector<unsigned char> b = good; poke<uint32_t>(b, 12, v); expect("header_bytes", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (uint64_t v : {(uint64_t)0, (uint64_t)good.size() - 1, (uint64_t)good.size() + 1, ~(uint64_t)0}) {
    std::vector<unsigned char> b = good; poke<uint64_t>(b, 16, v); expect("total_bytes", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  // W outside 1 .. 64, and geometries that are none (whatever the tables say)
  for (int32_t v : {0, -1, 65, INT32_MAX, INT32_MIN, 1 << 16}) {
    std::vector<unsigned char> b = good; poke<int32_t>(b, 24, v); expect("n_rings", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, 28, v); expect("n_layers", ok(b), LIODOM_ERR_INVALID_ARG);
    b = good; poke<int32_t>(b, 24, v); poke<int32_t>(b, 28, v); expect("n_rings and n_layers", ok(b), LIODOM_ERR_INVALID_ARG);
  }
  { std::vector<unsigned char> b = good; poke<int32_t>(b, 24, 13); poke<int32_t>(b, 28, 5); expect("W = 65", ok(b), LIODOM_ERR_INVALID_ARG); }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double v : {0.0, -1.0, inf, -inf, nan}) { std::vector<unsigned char> b = good; poke<double>(b, 32, v); expect("r_max", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (double v : {inf, -inf, nan, rz[2], rz[2] + 1.0}) { std::vector<unsigned char> b = good; poke<double>(b, 40, v); expect("z_min", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (double v : {inf, -inf, nan, rz[1], rz[1] - 1.0}) { std::vector<unsigned char> b = good; poke<double>(b, 48, v); expect("z_max", ok(b), LIODOM_ERR_INVALID_ARG); }
  // a valid geometry whose tables are not the blob's: every number one bit off, with and without the database's geometry
  for (size_t off : {(size_t)32, (size_t)40, (size_t)48}) {
    std::vector<unsigned char> b = good; b[off + 5] ^= 1;      // (a mantissa bit high enough to move a float table entry)
    expect("geometry moved, tables stale", ok(b), LIODOM_ERR_INVALID_ARG);
    expect("geometry moved, tables stale, no geometry given", run(b, b.size(), nullptr, nullptr, n), LIODOM_ERR_INVALID_ARG);
  }
  for (size_t i = 0; i < (size_t)kPlaceTablesBytes; i++) {      // every byte of the tables, padding included
    std::vector<unsigned char> b = good; b[(size_t)kPlaceStateHeaderBytes + i] ^= 1;
    expect("a table byte", run(b, b.size(), nullptr, nullptr, n), LIODOM_ERR_INVALID_ARG);
  }
  { // the database's geometry: bit for bit
    int32_t nm2[2] = {nm[0], nm[1]};
    double rz2[3] = {rz[0], rz[1], rz[2]};
    nm2[0] = nm[1]; nm2[1] = nm[0];
    if (nm[0] != nm[1]) expect("rings and layers swapped", run(good, good.size(), nm2, rz, n), LIODOM_ERR_INVALID_ARG);
    for (int a = 0; a < 3; a++) {
      rz2[a] = std::nextafter(rz[a], 1e9);
      expect("another database geometry", run(good, good.size(), nm, rz2, n), LIODOM_ERR_INVALID_ARG);
      rz2[a] = rz[a];
    }
  }
  for (int32_t v : {-1, INT32_MIN, n - 1, n + 1, 0, INT32_MAX}) { std::vector<unsigned char> b = good; poke<int32_t>(b, 56, v); expect("count", ok(b), LIODOM_ERR_INVALID_ARG); }
  for (int32_t v : {1, -1}) { std::vector<unsigned char> b = good; poke<int32_t>(b, 60, v); expect("reserved header word", ok(b), LIODOM_ERR_INVALID_ARG); }

  // records
  for (int p = 0; p < n; p++) {
    const size_t r = recs + (size_t)kPlaceRecordBytes * (size_t)p;
    for (int32_t v : {peek<int32_t>(good, r + 8) + 1, peek<int32_t>(good, r + 8) - 1, -1, INT32_MAX, INT32_MIN}) {
      std::vector<unsigned char> b = good; poke<int32_t>(b, r + 8, v); expect("bit count", ok(b), LIODOM_ERR_INVALID_ARG);
    }
    { std::vector<unsigned char> b = good; b[head + 8 * W * (size_t)p + 3] ^= 0x10; expect("a descriptor bit flipped", ok(b), LIODOM_ERR_INVALID_ARG); }
    { std::vector<unsigned char> b = good; poke<int32_t>(b, r + 12, 7); expect("reserved record word", ok(b), LIODOM_ERR_INVALID_ARG); }
    for (int a = 0; a < 7; a++) {
      for (double v : {inf, -inf, nan}) { std::vector<unsigned char> b = good; poke<double>(b, r + 16 + 8 * (size_t)a, v); expect("non-finite pose", ok(b), LIODOM_ERR_INVALID_ARG); }
    }
    { std::vector<unsigned char> b = good; for (int a = 0; a < 4; a++) poke<double>(b, r + 16 + 8 * (size_t)a, 0.0); expect("zero quaternion", ok(b), LIODOM_ERR_INVALID_ARG); }
    { std::vector<unsigned char> b = good; for (int a = 0; a < 4; a++) poke<double>(b, r + 16 + 8 * (size_t)a, peek<double>(good, r + 16 + 8 * (size_t)a) * 1.00001);
      expect("quaternion of norm 1.00001", ok(b), LIODOM_ERR_INVALID_ARG); }
    { std::vector<unsigned char> b = good; poke<int64_t>(b, r, INT64_MIN); expect("any id", ok(b), LIODOM_OK); }
    { std::vector<unsigned char> b = good; poke<double>(b, r + 16 + 8 * 5, -1e300); expect("any finite translation", ok(b), LIODOM_OK); }
  }
  { // two descriptor bits swapped between places keep the total but not the counts
    std::vector<unsigned char> b = good;
    const uint64_t w0 = peek<uint64_t>(good, head), w1 = peek<uint64_t>(good, head + 8 * W);
    poke<uint64_t>(b, head, w0 | (w0 + 1)); poke<uint64_t>(b, head + 8 * W, w1 & (w1 - 1));
    if (place_popcount64(w0 | (w0 + 1)) != place_popcount64(w0)) expect("a bit moved between places", ok(b), LIODOM_ERR_INVALID_ARG);
  }

  // capacity
  expect("max_places one short", run(good, good.size(), nm, rz, n - 1), LIODOM_ERR_CAPACITY);
  expect("max_places 0", run(good, good.size(), nm, rz, 0), LIODOM_ERR_CAPACITY);
  { // malformed AND too large: malformed wins
    std::vector<unsigned char> b = good; poke<int32_t>(b, recs + 8, -5);
    expect("bad bit count, max_places short", run(b, b.size(), nm, rz, n - 1), LIODOM_ERR_INVALID_ARG);
  }
  { // an empty database
    std::vector<unsigned char> b(good.begin(), good.begin() + (long)head);
    poke<uint64_t>(b, 16, (uint64_t)head); poke<int32_t>(b, 56, 0);
    expect("0 places", run(b, head, nm, rz, 0), LIODOM_OK);
  }
  { // the tables and the pose of a match, against values worked out by hand
    PlaceTables t;
    place_make_tables(16, 4, 80.0, -4.0, 12.0, &t);
    g_cases++;
    if (t.r2[0] != 25.0f || t.r2[15] != 6400.0f || t.z[0] != -4.0f || t.z[4] != 12.0f || t.cs[7] != t.cs[16 + 7] || t.cs[15] != 0.0f || t.r2[16] != 0.0f || t.z[5] != 0.0f) {
      std::fprintf(stderr, "FAIL default tables\n"); g_failures++;
    }
    const double place[7] = {0.0, 0.0, 0.0, 2.0, 1.0, 2.0, 3.0};      // (normalised first)
    double out[7];
    place_match_pose(place, 16, out);                                // a quarter turn
    g_cases++;
    if (std::fabs(out[2] - std::sqrt(0.5)) > 1e-15 || std::fabs(out[3] - std::sqrt(0.5)) > 1e-15 || out[0] != 0.0 || out[1] != 0.0 || out[4] != 1.0 || out[6] != 3.0) {
      std::fprintf(stderr, "FAIL place_match_pose\n"); g_failures++;
    }
  }
  std::printf("place_state_validate: %d cases, %d failures\n", g_cases, g_failures);
  return g_failures ? 1 : 0;
}
