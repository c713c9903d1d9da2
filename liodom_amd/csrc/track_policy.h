// track_policy.h — when a map reader counts as lost (DESIGN.md §3 "Knowing that a reader is lost"): a small policy over the
// per-scan hit records of liodom_set_map_hits (include/liodom_hip.h).
// Plain C++, no HIP include: tests/track_policy_main.cc compiles it for the host alone under sanitizers; liodom_replay and the
// Python binding (liodom_amd/api.py, class TrackPolicy: the same rules, restated) use it.
//
// A record is fed as (hits_r, hits_0, n_edges, flags).  Its fraction is (hits_r + hits_0) / (2 n_edges); a scan is BELOW if
// n_edges <= 0 or the fraction is not >= min_fraction (a fraction exactly equal to min_fraction is not below).  LOST is answered at
// the lost_after-th consecutive valid scan below (lost_after < 1 counts as 1), and the state starts over with it; a scan that is not
// below ends the streak.  A record without LIODOM_HIT_VALID changes nothing and answers TRACKING.
#pragma once
#include <stdint.h>

namespace liodom_dev {

enum TrackAnswer : int { TRACK_TRACKING = 0, TRACK_LOST = 1 };
constexpr uint32_t kTrackHitValid = 1u;      // LIODOM_HIT_VALID

struct TrackPolicy { double min_fraction; int lost_after; };
struct TrackState { int below = 0; };        // consecutive valid scans below, so far

inline double track_fraction(int32_t hits_r, int32_t hits_0, int32_t n_edges) {
  return n_edges > 0 ? ((double)hits_r + (double)hits_0) / (2.0 * (double)n_edges) : 0.0;
}
inline bool track_below(const TrackPolicy& p, int32_t hits_r, int32_t hits_0, int32_t n_edges) {
  return n_edges <= 0 || !(track_fraction(hits_r, hits_0, n_edges) >= p.min_fraction);
}
inline TrackAnswer track_feed(const TrackPolicy& p, TrackState* s, int32_t hits_r, int32_t hits_0, int32_t n_edges, uint32_t flags) {
  if (!(flags & kTrackHitValid)) return TRACK_TRACKING;
  if (!track_below(p, hits_r, hits_0, n_edges)) { s->below = 0; return TRACK_TRACKING; }
  if (++s->below < (p.lost_after < 1 ? 1 : p.lost_after)) return TRACK_TRACKING;
  s->below = 0;
  return TRACK_LOST;
}

}  // namespace liodom_dev
