// tests/place_policy_main.cc — liodom_amd/csrc/place_policy.h in a program of its own, for tests/test_place_policy.py (built plain
// and under host sanitizers; nothing of it is loaded into Python).
//   place_policy_main <min_dist> <min_yaw> [<qx> <qy> <qz> <qw> <tx> <ty> <tz>]...
// feeds the poses in order to one state and prints, per pose, "<answer>": 1 a key frame / 0 not.
#include <cstdio>
#include <cstdlib>

#include "place_policy.h"

int main(int argc, char** argv) {
  using namespace liodom_dev;
  if (argc < 3 || (argc - 3) % 7 != 0) { std::fprintf(stderr, "usage: %s min_dist min_yaw [qx qy qz qw tx ty tz]...\n", argv[0]); return 2; }
  PlacePolicy p;
  p.min_dist = std::strtod(argv[1], nullptr);
  p.min_yaw = std::strtod(argv[2], nullptr);
  PlacePolicyState s;
  for (int i = 3; i + 6 < argc; i += 7) {
    double pose[7];
    for (int a = 0; a < 7; a++) pose[a] = std::strtod(argv[i + a], nullptr);
    std::printf("%d\n", place_policy_feed(p, &s, pose));
  }
  return 0;
}
