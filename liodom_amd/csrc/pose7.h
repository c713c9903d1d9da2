// pose7.h — the one rule for a pose handed in as [qx qy qz qw tx ty tz]: seven finite numbers, | |q| - 1 | <= 1e-6, and the copy
// with the quaternion divided by its norm, sqrt(((q0^2 + q1^2) + q2^2) + q3^2) in double (-ffp-contract=off: results are compared
// as bits).  liodom_seed_stream, liodom_places_add, the place-state validator, graph_csr.h and reloc_candidates.h go through it, each
// with its own message and return value.  Plain C++, no HIP include: tests/pose7_main.cc compiles it alone under host sanitizers.
#pragma once
#include <math.h>

#define POSE7_RULE "| |q| - 1 | > 1e-6"      // kPose7NotNormalised in a refusal's text

namespace liodom_dev {

enum Pose7Verdict { kPose7Ok = 0, kPose7NonFinite = 1, kPose7NotNormalised = 2 };
inline double pose7_norm(const double* q) { return sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }
inline Pose7Verdict pose7_check(const double* pose) {
  for (int i = 0; i < 7; i++) if (!isfinite(pose[i])) return kPose7NonFinite;
  return fabs(pose7_norm(pose) - 1.0) <= 1e-6 ? kPose7Ok : kPose7NotNormalised;
}
inline void pose7_normalised(const double* pose, double* out) {      // (after pose7_check has passed; out may be pose)
  const double n = pose7_norm(pose);
  for (int i = 0; i < 4; i++) out[i] = pose[i] / n;
  for (int i = 4; i < 7; i++) out[i] = pose[i];
}

}  // namespace liodom_dev
