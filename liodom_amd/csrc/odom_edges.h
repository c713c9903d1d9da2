// odom_edges.h — the plain-C++ half of liodom_chain_odometry_edges / liodom_get_odometry_edges (kernel: kernels_odom_edges.h;
// host entry points in liodom_hip.hip; DESIGN.md §3 "Odometry edges from the scans' covariances"): the options' defaults and
// validation, and the rule an interval of a stream's log must satisfy.  No HIP include: tests/odom_edges_main.cc compiles it
// for the host alone, plain and under sanitizers (tests/test_odom_edges_host.py).
//
// THE RANGE RULE.  An interval (a, b) of a log is served iff  first <= a < b < limit:
//   the public form      first = 0, limit = m, the entries the caller handed in;
//   the handle form      first = the stream's scan count at its last reset, seed or import (the entries below it belong to an
//                        earlier life of the stream), limit = min(scans enqueued, pose_log_capacity): scans beyond the capacity
//                        are not logged.
// A call serves 0 <= n <= kOdomEdgesMax intervals; one interval outside the rule refuses the call.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/liodom_hip.h"

namespace liodom_dev {

constexpr int kOdomEdgesMax = LIODOM_ODOM_EDGES_MAX;      // 2^20 intervals per call

inline void odom_edge_options_default(liodom_odom_edge_options_t* o) {
  o->inflation = 1.0;
  o->floor_rotation = 0.0;
  o->floor_translation = 0.0;
  for (int i = 0; i < 4; i++) o->reserved[i] = 0;
}
// nullptr: fine; otherwise why not (static text)
inline const char* odom_edge_options_refusal(const liodom_odom_edge_options_t* o) {
  if (!isfinite(o->inflation) || !(o->inflation > 0.0)) return "inflation is not a finite number above 0";
  if (!isfinite(o->floor_rotation) || !(o->floor_rotation >= 0.0)) return "floor_rotation is negative or not finite";
  if (!isfinite(o->floor_translation) || !(o->floor_translation >= 0.0)) return "floor_translation is negative or not finite";
  for (int i = 0; i < 4; i++) if (o->reserved[i] != 0) return "a reserved option is not 0";
  return nullptr;
}
// The limit of the handle form (see above); 0 where nothing is logged.
inline int odom_edge_log_limit(int scans_enqueued, int pose_log_capacity) {
  const int lim = scans_enqueued < pose_log_capacity ? scans_enqueued : pose_log_capacity;
  return lim < 0 ? 0 : lim;
}
// nullptr: every interval lies in [first, limit); otherwise why the call is refused.  *bad (optional) = the first refused row.
inline const char* odom_edge_ranges_refusal(const int32_t* from, const int32_t* to, int n, int first, int limit, int* bad) {
  if (bad) *bad = -1;
  if (n < 0) return "a negative count";
  if (n > kOdomEdgesMax) return "more than 2^20 intervals in one call";
  if (n > 0 && (!from || !to)) return "a null list of intervals";
  for (int i = 0; i < n; i++) {
    if (!(first <= from[i] && from[i] < to[i] && to[i] < limit)) {
      if (bad) *bad = i;
      return "an interval outside first <= from < to < limit of the log";
    }
  }
  return nullptr;
}

}  // namespace liodom_dev
