// Stand-alone driver of stream_state_validate (liodom_amd/csrc/stream_state_format.h), built plain and with
// -fsanitize=address,undefined by tests/test_stream_state_format.py.  Every blob is handed over in a heap block of exactly its
// length (so that a read beyond `bytes` is a sanitizer error), and a second time at an odd address: a block of length + 1, the blob
// from byte 1 to the block's end.  The two must agree.
//   judge BLOB p0 .. p5 mapping edge_cap recv_cap   prints "<code> <reason>" for the blob in file BLOB, offered to a handle with the
//                                                   fingerprint p0 .. p5 (the header's order) and these capacities
//   sweep BLOB p0 .. p5 mapping edge_cap recv_cap   BLOB is a good blob for that handle.  Every prefix of it, and it with every single
//                                                   byte of header + record + counts XOR 0xFF: the code is one of the three, a
//                                                   refusal names its reason, a strict prefix is refused as LIODOM_ERR_INVALID_ARG
// Exit code 0: all as stated.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "stream_state_format.h"

using namespace liodom_dev;

struct Taker { StateBlobHeader mine; bool mapping; int edge_cap, recv_cap; };

static int g_failures = 0;

static int offer(const Taker& t, const unsigned char* data, size_t len, const char** why) {
  const char* reason[2] = {nullptr, nullptr};
  int rc[2];
  for (int odd = 0; odd < 2; odd++) {
    unsigned char* block = static_cast<unsigned char*>(std::malloc(len + (size_t)odd));      // (of 0 bytes: a pointer no byte of which may be read)
    if (!block && len + (size_t)odd) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
    if (len) memcpy(block + odd, data, len);
    rc[odd] = stream_state_validate(block + odd, (int64_t)len, t.mine, t.mapping, t.edge_cap, t.recv_cap, &reason[odd]);
    std::free(block);
  }
  if (rc[0] != rc[1] || !reason[0] || !reason[1] || strcmp(reason[0], reason[1]) != 0) {
    std::fprintf(stderr, "FAIL length %zu: %d at an aligned address, %d at an odd one\n", len, rc[0], rc[1]); g_failures++;
  }
  if (rc[0] != LIODOM_OK && rc[0] != LIODOM_ERR_INVALID_ARG && rc[0] != LIODOM_ERR_CAPACITY) {
    std::fprintf(stderr, "FAIL length %zu: code %d is none of the three\n", len, rc[0]); g_failures++;
  }
  if (rc[0] != LIODOM_OK && !(reason[0] && reason[0][0])) { std::fprintf(stderr, "FAIL length %zu: code %d without a reason\n", len, rc[0]); g_failures++; }
  *why = reason[0] ? reason[0] : "";
  return rc[0];
}

int main(int argc, char** argv) {
  if (argc != 12 || (strcmp(argv[1], "judge") != 0 && strcmp(argv[1], "sweep") != 0)) {
    std::fprintf(stderr, "usage: %s judge|sweep BLOB p0 p1 p2 p3 p4 p5 mapping edge_cap recv_cap\n", argv[0]); return 2;
  }
  std::ifstream f(argv[2], std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  const std::vector<unsigned char> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  Taker t;
  memset(&t.mine, 0, sizeof(t.mine));
  uint32_t* fp[6] = {&t.mine.local_map_size, &t.mine.mapping, &t.mine.filter_local_map, &t.mine.use_imu, &t.mine.pose_rotation_mode, &t.mine.lm_apply_step_on_ftol};
  for (int i = 0; i < 6; i++) *fp[i] = (uint32_t)std::strtoul(argv[3 + i], nullptr, 10);
  t.mapping = std::atoi(argv[9]) != 0; t.edge_cap = std::atoi(argv[10]); t.recv_cap = std::atoi(argv[11]);
  const char* why = "";
  if (strcmp(argv[1], "judge") == 0) {
    const int rc = offer(t, blob.data(), blob.size(), &why);
    std::printf("%d %s\n", rc, why);
    return g_failures ? 1 : 0;
  }
  const size_t head = state_points_offset((int)t.mine.local_map_size);
  if (offer(t, blob.data(), blob.size(), &why) != LIODOM_OK || blob.size() < head) { std::fprintf(stderr, "the blob to sweep is not a good one: %s\n", why); return 2; }
  int cases = 0, refused = 0;
  for (size_t len = 0; len < blob.size(); len++, cases++) {
    if (offer(t, blob.data(), len, &why) != LIODOM_ERR_INVALID_ARG) { std::fprintf(stderr, "FAIL prefix of %zu bytes is not refused as an invalid argument\n", len); g_failures++; }
  }
  // the null blob, with and without a length
  for (int64_t len : {(int64_t)0, (int64_t)blob.size(), (int64_t)-1}) {
    cases++;
    if (stream_state_validate(nullptr, len, t.mine, t.mapping, t.edge_cap, t.recv_cap, nullptr) != LIODOM_ERR_INVALID_ARG) { std::fprintf(stderr, "FAIL null blob\n"); g_failures++; }
  }
  { cases++;      // a negative length with bytes behind the pointer
    if (stream_state_validate(blob.data(), -(int64_t)blob.size(), t.mine, t.mapping, t.edge_cap, t.recv_cap, &why) != LIODOM_ERR_INVALID_ARG) { std::fprintf(stderr, "FAIL negative length\n"); g_failures++; } }
  std::vector<unsigned char> b = blob;
  for (size_t i = 0; i < head; i++, cases++) {
    b[i] ^= 0xFF;
    if (offer(t, b.data(), b.size(), &why) != LIODOM_OK) refused++;
    b[i] ^= 0xFF;
  }
  std::printf("stream_state_validate: %d cases, %d flipped bytes refused, %d failures\n", cases, refused, g_failures);
  return g_failures ? 1 : 0;
}
