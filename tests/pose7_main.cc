// pose7.h in a program of its own (tests/test_pose7.py builds it plain and under ASan + UBSan and runs it).
// argv[1]: a file of poses, one per line, seven doubles as 16 hex digits each (their bits).  Per pose one line goes out: the verdict
// of pose7_check (0 fine, 1 non-finite, 2 not normalised) and, where it is 0, the seven numbers of pose7_normalised as bits.  Each
// pose is handed over in a heap block of exactly 56 bytes, the copy is written into another.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pose7.h"

using namespace liodom_dev;

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s poses.txt\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  for (;;) {
    uint64_t bits[7];
    int got = 0;
    while (got < 7 && std::fscanf(f, "%" SCNx64, &bits[got]) == 1) got++;
    if (got == 0) break;
    if (got != 7) { std::fprintf(stderr, "a line of %d numbers\n", got); return 2; }
    double* pose = static_cast<double*>(std::malloc(7 * sizeof(double)));
    double* out = static_cast<double*>(std::malloc(7 * sizeof(double)));
    if (!pose || !out) return 2;
    std::memcpy(pose, bits, sizeof(bits));
    const Pose7Verdict v = pose7_check(pose);
    std::printf("%d", (int)v);
    if (v == kPose7Ok) {
      pose7_normalised(pose, out);
      std::memcpy(bits, out, sizeof(bits));
      for (int i = 0; i < 7; i++) std::printf(" %016" PRIx64, bits[i]);
      pose7_normalised(pose, pose);      // in place gives the same
      if (std::memcmp(pose, out, 7 * sizeof(double)) != 0) { std::fprintf(stderr, "in place differs\n"); return 1; }
    }
    std::printf("\n");
    std::free(pose);
    std::free(out);
  }
  std::fclose(f);
  return 0;
}
