// tests/track_policy_main.cc — liodom_amd/csrc/track_policy.h in a program of its own, for tests/test_track_policy.py (built plain
// and under host sanitizers; nothing of it is loaded into Python).
//   track_policy_main <min_fraction> <lost_after> [<hits_r> <hits_0> <n_edges> <flags>]...
// feeds the records in order to one state and prints, per record, "<answer> <below>": 0 tracking / 1 lost, and the state's streak.
#include <cstdio>
#include <cstdlib>

#include "track_policy.h"

int main(int argc, char** argv) {
  using namespace liodom_dev;
  if (argc < 3 || (argc - 3) % 4 != 0) { std::fprintf(stderr, "usage: %s min_fraction lost_after [hits_r hits_0 n_edges flags]...\n", argv[0]); return 2; }
  TrackPolicy p;
  p.min_fraction = std::strtod(argv[1], nullptr);
  p.lost_after = (int)std::strtol(argv[2], nullptr, 10);
  TrackState s;
  for (int i = 3; i + 3 < argc; i += 4) {
    const int32_t hr = (int32_t)std::strtol(argv[i], nullptr, 10), h0 = (int32_t)std::strtol(argv[i + 1], nullptr, 10), n = (int32_t)std::strtol(argv[i + 2], nullptr, 10);
    const uint32_t flags = (uint32_t)std::strtoul(argv[i + 3], nullptr, 10);
    const TrackAnswer a = track_feed(p, &s, hr, h0, n, flags);
    std::printf("%d %d\n", (int)a, s.below);
  }
  return 0;
}
