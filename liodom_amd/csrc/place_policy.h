// place_policy.h — when a scan becomes a key frame of a place database (DESIGN.md §3 "Finding the place"): by distance from the
// last key frame, nothing else.
// Plain C++, no HIP include: tests/place_policy_main.cc compiles it for the host alone under sanitizers; liodom::PlaceDb and the
// Python binding (liodom_amd/api.py, class PlacePolicy: the same rules, restated) use it.
//
// A pose is [qx qy qz qw tx ty tz].  The first finite pose fed is a key frame.  A later one is a key frame iff it has moved from the
// LAST KEY FRAME's pose by
//   dist  = sqrt(dx dx + dy dy + dz dz)                                >= min_dist, or
//   angle = 2 acos(min(1, |qa . qb| / (|qa| |qb|))) (the rotation between the two) >= min_yaw
// (a threshold that is exactly met counts; min_yaw = infinity switches the angle off).  A pose with a non-finite number, or a
// quaternion of norm 0, is no key frame and changes nothing.
#pragma once
#include <math.h>

namespace liodom_dev {

struct PlacePolicy { double min_dist, min_yaw; };
struct PlacePolicyState { bool has = false; double last[7] = {0, 0, 0, 1, 0, 0, 0}; };

inline double place_policy_dist(const double* a, const double* b) {
  const double dx = a[4] - b[4], dy = a[5] - b[5], dz = a[6] - b[6];
  return sqrt(dx * dx + dy * dy + dz * dz);
}
inline double place_policy_angle(const double* a, const double* b) {
  const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
  const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
  const double dot = fabs(a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]) / (na * nb);
  return 2.0 * acos(dot < 1.0 ? dot : 1.0);
}
// 1: `pose` is a key frame (and becomes the last one); 0: it is not
inline int place_policy_feed(const PlacePolicy& p, PlacePolicyState* s, const double* pose) {
  for (int i = 0; i < 7; i++) if (!isfinite(pose[i])) return 0;
  if (!(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2] + pose[3] * pose[3] > 0.0)) return 0;
  if (s->has && !(place_policy_dist(pose, s->last) >= p.min_dist) && !(place_policy_angle(pose, s->last) >= p.min_yaw)) return 0;
  for (int i = 0; i < 7; i++) s->last[i] = pose[i];
  s->has = true;
  return 1;
}

}  // namespace liodom_dev
