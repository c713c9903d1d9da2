// Stand-alone driver of the candidate grid of liodom_map_search_pose (liodom_amd/csrc/reloc_candidates.h), built plain and with
// -fsanitize=address,undefined by tests/test_reloc_candidates.py.
//   argv: qx qy qz qw tx ty tz step_xy step_z step_yaw nx ny nz nyaw radius [last]
// prints "n <candidates>" and one line per candidate: its index, ix iy ia iz, the 12 doubles of T and the 7 of its pose (%.17g),
// or "refused: <why>" (exit code 3) for a grid the library refuses.  With a 16th argument only the last candidate's line is printed
// (every matrix is still made).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reloc_candidates.h"

int main(int argc, char** argv) {
  if (argc != 16 && argc != 17) { std::fprintf(stderr, "usage: %s qx qy qz qw tx ty tz step_xy step_z step_yaw nx ny nz nyaw radius [last]\n", argv[0]); return 2; }
  liodom_pose_search_t s = {};
  for (int i = 0; i < 7; i++) s.centre[i] = std::strtod(argv[1 + i], nullptr);
  s.step_xy = std::strtod(argv[8], nullptr); s.step_z = std::strtod(argv[9], nullptr); s.step_yaw = std::strtod(argv[10], nullptr);
  s.nx = std::atoi(argv[11]); s.ny = std::atoi(argv[12]); s.nz = std::atoi(argv[13]); s.nyaw = std::atoi(argv[14]); s.radius = std::atoi(argv[15]);
  const char* why = "";
  const int64_t n = liodom_dev::reloc_candidate_count(&s, &why);
  if (n <= 0) { std::printf("refused: %s\n", why); return 3; }
  std::vector<double> T(12 * (size_t)n);
  liodom_dev::reloc_candidates(&s, n, T.data());
  std::printf("n %lld\n", (long long)n);
  for (int64_t i = argc == 17 ? n - 1 : 0; i < n; i++) {
    int ix, iy, ia, iz;
    liodom_dev::reloc_candidate_indices(&s, i, &ix, &iy, &ia, &iz);
    double pose[7];
    liodom_dev::reloc_candidate_pose(&s, i, pose);
    std::printf("%lld %d %d %d %d", (long long)i, ix, iy, ia, iz);
    for (int k = 0; k < 12; k++) std::printf(" %.17g", T[12 * (size_t)i + k]);
    for (int k = 0; k < 7; k++) std::printf(" %.17g", pose[k]);
    std::printf("\n");
  }
  return 0;
}
