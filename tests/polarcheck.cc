// polarcheck — the polar projection and blob layout of liodom_amd/csrc/liodom_math.h as a stand-alone host program
// (tests/test_polar_format.py builds it with g++ -ffp-contract=off and compares its output with tests/polarref.py).
//   polarcheck layout H W range_bits intensity_bits        prints: range_offset intensity_offset total_bytes
//   polarcheck project IN OUT                              IN: int32 order H W range_bits intensity_bits T, float32 range_unit
//       beam_origin, float32 cos_alt[H] sin_alt[H] cos_baz[H] sin_baz[H] cos_enc[T] sin_enc[T], then the blob; OUT: float32 [H W][4]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

static std::vector<unsigned char> read_all(const char* path) {
  std::vector<unsigned char> b;
  FILE* f = std::fopen(path, "rb");
  if (!f) return b;
  unsigned char buf[65536];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
  std::fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "layout")) {
    long long r, i, t;
    polar_sections(std::atoll(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), &r, &i, &t);
    std::printf("%lld %lld %lld\n", r, i, t);
    return 0;
  }
  if (argc != 4 || std::strcmp(argv[1], "project")) return 2;
  const std::vector<unsigned char> in = read_all(argv[2]);
  if (in.size() < 32) return 3;
  int32_t hd[6];
  float sc[2];
  std::memcpy(hd, in.data(), 24);
  std::memcpy(sc, in.data() + 24, 8);
  const int order = hd[0], H = hd[1], W = hd[2], rb = hd[3] / 8, ib = hd[4] / 8, T = hd[5];
  const size_t n = (size_t)H * W, tab_floats = 4 * (size_t)H + 2 * (size_t)T;
  long long r_off, i_off, total;
  polar_sections(H, W, hd[3], hd[4], &r_off, &i_off, &total);
  if (in.size() != 32 + 4 * tab_floats + (size_t)total) return 4;
  std::vector<float> tab(tab_floats);
  std::memcpy(tab.data(), in.data() + 32, 4 * tab_floats);
  const float *ca = tab.data(), *sa = ca + H, *cb = sa + H, *sb = cb + H, *ce = sb + H, *se = ce + T;
  const unsigned char* blob = in.data() + 32 + 4 * tab_floats;
  std::vector<float> out(4 * n);
  for (size_t p = 0; p < n; p++) {
    const size_t row = order == 0 ? p % H : p / W, col = order == 0 ? p / H : p % W;
    uint32_t t, c = 0, iv = 0;
    std::memcpy(&t, blob + 4 * col, 4);
    std::memcpy(&c, blob + r_off + p * rb, rb);          // (little-endian host)
    if (ib) std::memcpy(&iv, blob + i_off + p * ib, ib);
    const bool ok = t < (uint32_t)T;
    polar_project_point(c, (float)iv, ok, ok ? ce[t] : 0.f, ok ? se[t] : 0.f, ca[row], sa[row], cb[row], sb[row], sc[0], sc[1], &out[4 * p]);
  }
  FILE* f = std::fopen(argv[3], "wb");
  if (!f) return 5;
  const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
  std::fclose(f);
  return ok ? 0 : 6;
}
