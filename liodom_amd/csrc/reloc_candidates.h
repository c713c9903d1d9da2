// reloc_candidates.h — the candidate grid of liodom_map_search_pose (include/liodom_hip.h): validation of a liodom_pose_search_t,
// the candidates' matrices and the pose of one candidate, all on the host in double.
// Plain C++, no HIP include: tests/reloc_candidates_main.cc compiles it for the host alone under sanitizers.
//
// Candidate (ix, iy, ia, iz), each index from -n to n; index = ((iz + nz) * (2 nyaw + 1) + (ia + nyaw)) * (2 ny + 1) * (2 nx + 1)
// + (iy + ny) * (2 nx + 1) + (ix + nx): ix fastest, then iy, then ia (yaw), iz slowest.
//   T = [ Rz(ia * step_yaw) * R_c | t_c + (ix * step_xy, iy * step_xy, iz * step_z) ]
// R_c: the centre's quaternion divided by its norm in double, then Eigen's toRotationMatrix as iso_from_qt (liodom_math.h) writes
// it — what liodom_seed_stream does to a seed.  Rz(a) * R_c: row 0 = cos a * R0 - sin a * R1, row 1 = sin a * R0 + cos a * R1,
// row 2 = R2.  The pose of a candidate is the quaternion qz(a) * q_c (Hamilton product, then normalised) and the same translation.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/liodom_hip.h"
#include "pose7.h"

namespace liodom_dev {

constexpr int64_t kRelocCandidatesMax = 1 << 20;

inline bool reloc_finite(double x) { return (x - x) == 0.0; }      // (inf - inf and NaN - NaN are NaN)

// Number of candidates of a valid grid; 0 and *why (optional) set for one liodom_map_search_pose refuses.  `limit`: the most
// candidates per axis and in all (liodom_map_search_pose_bnb lifts it to kRelocBnbCandidatesMax, reloc_bnb.h).
inline int64_t reloc_candidate_count(const liodom_pose_search_t* s, const char** why, int64_t limit = kRelocCandidatesMax) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  if (!s) { *why = "null search"; return 0; }
  if (s->radius != 0 && s->radius != 1) { *why = "radius is not 0 or 1"; return 0; }
  if (s->nx < 0 || s->ny < 0 || s->nz < 0 || s->nyaw < 0) { *why = "negative half count"; return 0; }
  if (const Pose7Verdict v = pose7_check(s->centre)) {
    *why = v == kPose7NonFinite ? "non-finite centre" : "the centre's quaternion is not normalised (" POSE7_RULE ")"; return 0;
  }
  // a step is read only where its half count is > 0
  if (((s->nx > 0 || s->ny > 0) && !(s->step_xy > 0.0 && reloc_finite(s->step_xy))) || (s->nz > 0 && !(s->step_z > 0.0 && reloc_finite(s->step_z))) ||
      (s->nyaw > 0 && !(s->step_yaw > 0.0 && reloc_finite(s->step_yaw)))) {
    *why = "non-positive step with a half count > 0"; return 0;
  }
  int64_t n = 1;
  const int32_t half[4] = {s->nx, s->ny, s->nyaw, s->nz};
  for (int a = 0; a < 4; a++) {
    const char* many = limit == kRelocCandidatesMax ? "more than 2^20 candidates" : "more candidates than the call takes";
    if (half[a] > limit) { *why = many; return 0; }
    n *= 2 * (int64_t)half[a] + 1;
    if (n > limit) { *why = many; return 0; }
  }
  return n;
}

struct RelocCentre { double q[4], t[3], R[9]; };

inline RelocCentre reloc_centre(const liodom_pose_search_t* s) {
  RelocCentre c;
  double p[7];
  pose7_normalised(s->centre, p);
  for (int i = 0; i < 4; i++) c.q[i] = p[i];
  for (int i = 0; i < 3; i++) c.t[i] = p[4 + i];
  const double x = c.q[0], y = c.q[1], z = c.q[2], w = c.q[3];      // iso_from_qt
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  c.R[0] = 1 - (tyy + tzz); c.R[1] = txy - twz;       c.R[2] = txz + twy;
  c.R[3] = txy + twz;       c.R[4] = 1 - (txx + tzz); c.R[5] = tyz - twx;
  c.R[6] = txz - twy;       c.R[7] = tyz + twx;       c.R[8] = 1 - (txx + tyy);
  return c;
}

// (ix, iy, ia, iz) of a candidate index of a valid grid
inline void reloc_candidate_indices(const liodom_pose_search_t* s, int64_t index, int* ix, int* iy, int* ia, int* iz) {
  const int64_t wx = 2 * (int64_t)s->nx + 1, wy = 2 * (int64_t)s->ny + 1, wa = 2 * (int64_t)s->nyaw + 1;
  *ix = (int)(index % wx) - s->nx; index /= wx;
  *iy = (int)(index % wy) - s->ny; index /= wy;
  *ia = (int)(index % wa) - s->nyaw; index /= wa;
  *iz = (int)index - s->nz;
}

// the translation of a candidate: what its matrix holds in T[3], T[7], T[11]
inline void reloc_candidate_translation(const liodom_pose_search_t* s, const RelocCentre& c, int ix, int iy, int iz, double* t) {
  t[0] = c.t[0] + (ix ? ix * s->step_xy : 0.0);
  t[1] = c.t[1] + (iy ? iy * s->step_xy : 0.0);
  t[2] = c.t[2] + (iz ? iz * s->step_z : 0.0);
}

inline void reloc_candidate_matrix(const liodom_pose_search_t* s, const RelocCentre& c, int64_t index, double* T) {
  int ix, iy, ia, iz;
  reloc_candidate_indices(s, index, &ix, &iy, &ia, &iz);
  const double a = ia * s->step_yaw;
  const double ca = ia ? cos(a) : 1.0, sa = ia ? sin(a) : 0.0;
  for (int j = 0; j < 3; j++) {
    T[j] = ca * c.R[j] - sa * c.R[3 + j];
    T[4 + j] = sa * c.R[j] + ca * c.R[3 + j];
    T[8 + j] = c.R[6 + j];
  }
  double t[3];
  reloc_candidate_translation(s, c, ix, iy, iz, t);
  T[3] = t[0]; T[7] = t[1]; T[11] = t[2];
}

// every candidate's matrix, in index order: T holds 12 * n doubles, n = reloc_candidate_count(s)
inline void reloc_candidates(const liodom_pose_search_t* s, int64_t n, double* T) {
  const RelocCentre c = reloc_centre(s);
  for (int64_t i = 0; i < n; i++) reloc_candidate_matrix(s, c, i, T + 12 * i);
}

// one candidate as liodom_seed_stream takes it: [qx qy qz qw tx ty tz], the quaternion normalised
inline void reloc_candidate_pose(const liodom_pose_search_t* s, int64_t index, double* pose) {
  const RelocCentre c = reloc_centre(s);
  int ix, iy, ia, iz;
  reloc_candidate_indices(s, index, &ix, &iy, &ia, &iz);
  const double h = 0.5 * (ia * s->step_yaw);
  const double sz = ia ? sin(h) : 0.0, cw = ia ? cos(h) : 1.0;      // qz = (0, 0, sz, cw)
  const double bx = c.q[0], by = c.q[1], bz = c.q[2], bw = c.q[3];
  double q[4] = {cw * bx - sz * by, cw * by + sz * bx, cw * bz + sz * bw, cw * bw - sz * bz};
  const double norm = pose7_norm(q);
  for (int i = 0; i < 4; i++) pose[i] = q[i] / norm;
  pose[4] = c.t[0] + (ix ? ix * s->step_xy : 0.0);
  pose[5] = c.t[1] + (iy ? iy * s->step_xy : 0.0);
  pose[6] = c.t[2] + (iz ? iz * s->step_z : 0.0);
}

}  // namespace liodom_dev
