// polarhost — the geometry class of the host C++ mirror (liodom_amd/host/liodom_host.h) without a device:
// PolarGeometry::fromAngles / toC / layout / blobBytes.  tests/test_polar_host.py builds and runs it.
//
//   polarhost <in> <out> H W range_bits intensity_bits
// in : double altitude[H], double encoder[W] (radians; T = W)
// out: float cos_alt[H] sin_alt[H] cos_baz[H] sin_baz[H] cos_enc[W] sin_enc[W]; int64 layout[4] (tick, range, intensity offset, total);
//      int32 refused (fromAngles threw on a table of the wrong length)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../liodom_amd/host/liodom_host.h"

template <class T> static void put(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(sizeof(T) * n)); }

int main(int argc, char** argv) {
  if (argc != 7) { std::fprintf(stderr, "usage: %s <in> <out> H W range_bits intensity_bits\n", argv[0]); return 2; }
  const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), rb = std::atoi(argv[5]), ib = std::atoi(argv[6]);
  try {
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<double> alt((size_t)H), enc((size_t)W), baz((size_t)H, 0.0);
    in.read(reinterpret_cast<char*>(alt.data()), (std::streamsize)(sizeof(double) * alt.size()));
    in.read(reinterpret_cast<char*>(enc.data()), (std::streamsize)(sizeof(double) * enc.size()));
    const liodom::PolarGeometry g = liodom::PolarGeometry::fromAngles(H, W, alt, baz, enc, rb, ib, 0.002f, 0.f);
    const liodom_polar_layout_t lay = g.layout();
    if (g.blobBytes() != (size_t)lay.total_bytes) { std::fprintf(stderr, "polarhost: blobBytes() is not layout()'s total\n"); return 1; }
    if (!in) { std::fprintf(stderr, "polarhost: %s is too short\n", argv[1]); return 1; }

    std::ofstream out(argv[2], std::ios::binary);
    put(out, g.cos_alt.data(), (size_t)H); put(out, g.sin_alt.data(), (size_t)H);
    put(out, g.cos_baz.data(), (size_t)H); put(out, g.sin_baz.data(), (size_t)H);
    put(out, g.cos_enc.data(), (size_t)W); put(out, g.sin_enc.data(), (size_t)W);
    const int64_t lay4[4] = {lay.tick_offset, lay.range_offset, lay.intensity_offset, lay.total_bytes};
    put(out, lay4, 4);
    int32_t refused = 0;
    try {
      std::vector<double> short_alt(alt.begin(), alt.end() - 1);
      (void)liodom::PolarGeometry::fromAngles(H, W, short_alt, baz, enc, rb, ib, 0.002f, 0.f);
    } catch (const std::invalid_argument&) {
      refused = 1;
    }
    put(out, &refused, 1);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "polarhost: %s\n", e.what());
    return 1;
  }
  return 0;
}
