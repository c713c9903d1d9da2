// stream_state_format.h — a stream's odometry state as one contiguous blob: the layout, the validator of untrusted bytes and what
// else the host knows about the format.  Plain C++: no HIP include, compiles for the host alone (tests/stream_state_validate_main.cc
// does so under host sanitizers).  Included by liodom_kernels.h; the kernels that write and read the blob live in kernels_state.h.
// =============================================================================================
// Blob layout (little endian; every part starts on a 16-byte boundary; DESIGN.md §3 has the same table):
//   [0, 64)      StateBlobHeader   magic "LIODOMST", version, total size, fingerprint of what must match on import
//   [64, 480)    StateBlobRecord   poses, counters and flags, sizes of the parts that follow, last IMU orientation
//   [480, ...)   int32 count[round_up(local_map_size, 4)]   points of window frame j, OLDEST FIRST (LocalMapManager order);
//                                  entries behind n_frames are 0
//   then         float4 points[n_points]   the frames back to back, oldest first: the order of liodom_get_window
//   then         float4 recv[n_recv]       (mapping = 1) the last received ~map cloud
// The blob holds the stream's LOGICAL state only.  What a handle derives from it — cell hash, filtered local map, kNN saves — and
// what only tunes a code path — spec_*, hb_* — does not travel: liodom_import_stream_state rebuilds the former for whichever
// variant the importing handle runs and starts the latter afresh.
// =============================================================================================
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/liodom_hip.h"
#include "liodom_math.h"
#include "pose7.h"

namespace liodom_dev {

constexpr unsigned int kStateBlobVersion = 1u;
constexpr int kStateHeaderBytes = 64;
struct StateBlobHeader {
  char magic[8];                 // "LIODOMST"
  uint32_t version;              // kStateBlobVersion
  uint32_t header_bytes;         // 64
  uint64_t total_bytes;          // of the whole blob
  uint32_t local_map_size, mapping, filter_local_map, use_imu, pose_rotation_mode, lm_apply_step_on_ftol;      // the fingerprint
  uint32_t reserved[4];
};
struct StateBlobRecord {
  double odom[12], prev_odom[12], final_odom[12], param_q[4], param_t[3];      // as in StreamState
  int32_t initialized, append_raw, frame_count, n_frames, scan_counter;
  uint32_t status;               // the sticky LIODOM_STATUS_* bits
  int32_t n_points;              // window points = sum of the frame counts
  int32_t n_recv;                // points of the received ~map cloud (0 unless mapping)
  int32_t has_imu, pad;          // imu_q is meaningful (use_imu handles)
  double imu_q[4];               // last IMU orientation [x y z w]
};
static_assert(sizeof(StateBlobHeader) == kStateHeaderBytes, "blob header is 64 bytes");
static_assert(sizeof(StateBlobRecord) == 416, "blob record is 416 bytes");
constexpr int kStateCountsOffset = kStateHeaderBytes + (int)sizeof(StateBlobRecord);      // 480
LD_HD int state_counts_bytes(int P) { return 4 * ((P + 3) / 4 * 4); }
LD_HD size_t state_points_offset(int P) { return (size_t)kStateCountsOffset + (size_t)state_counts_bytes(P); }
LD_HD size_t state_blob_bytes(int P, long long n_points, long long n_recv) {
  return state_points_offset(P) + 16 * (size_t)(n_points + n_recv);
}

// The one place where untrusted blob bytes are parsed.  Checks `blob` (`bytes` long; no byte beyond is read, no alignment is
// assumed, and no sum or product of its fields can overflow) against the handle that is to take it: `mine` holds that handle's
// fingerprint (nothing else of it is read), mapping / edge_cap / recv_cap are its.  LIODOM_OK, and the blob's record in *rec (optional);
// LIODOM_ERR_INVALID_ARG for anything that is not a well-formed blob of a handle with this fingerprint; LIODOM_ERR_CAPACITY for a
// well-formed one with a frame above edge_cap or a received map above recv_cap.  The first rule that fails decides (DESIGN.md §3
// lists them in this order); *why (optional) names it.  The record's doubles are the caller's business: none is looked at.
inline int stream_state_validate(const void* blob, int64_t bytes, const StateBlobHeader& mine, bool mapping, int edge_cap, int recv_cap,
                                 const char** why, StateBlobRecord* rec = nullptr) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  const int P = (int)mine.local_map_size;
  if (!b || bytes < (int64_t)state_points_offset(P)) { *why = "blob truncated"; return LIODOM_ERR_INVALID_ARG; }
  StateBlobHeader hd;
  memcpy(&hd, b, sizeof(hd));
  if (memcmp(hd.magic, "LIODOMST", 8) != 0 || hd.version != kStateBlobVersion || hd.header_bytes != (uint32_t)kStateHeaderBytes ||
      hd.total_bytes != (uint64_t)bytes) {
    *why = "not a stream-state blob of this version and size"; return LIODOM_ERR_INVALID_ARG;
  }
  if (hd.local_map_size != mine.local_map_size || hd.mapping != mine.mapping || hd.filter_local_map != mine.filter_local_map ||
      hd.use_imu != mine.use_imu || hd.pose_rotation_mode != mine.pose_rotation_mode || hd.lm_apply_step_on_ftol != mine.lm_apply_step_on_ftol) {
    *why = "the blob comes from a handle with other parameters (local_map_size, mapping, filter_local_map, "
           "use_imu, pose_rotation_mode, lm_apply_step_on_ftol must match)";
    return LIODOM_ERR_INVALID_ARG;
  }
  StateBlobRecord r;
  memcpy(&r, b + kStateHeaderBytes, sizeof(r));
  const int nf_want = r.frame_count < P ? r.frame_count : P;
  if (r.frame_count < 0 || r.n_frames != nf_want || r.scan_counter != r.frame_count || r.n_points < 0 || r.n_recv < 0 ||
      (r.n_recv > 0 && !mapping) || (r.initialized != 0 && r.initialized != 1) || (r.append_raw != 0 && r.append_raw != 1) ||
      (uint64_t)state_blob_bytes(P, r.n_points, r.n_recv) != hd.total_bytes) {      // (both >= 0 here: at most 2^36 bytes)
    *why = "inconsistent state record"; return LIODOM_ERR_INVALID_ARG;
  }
  int64_t sum = 0;
  for (int j = 0; j < state_counts_bytes(P) / 4; j++) {
    int32_t c;
    memcpy(&c, b + kStateCountsOffset + 4 * j, sizeof(c));
    if (c < 0 || (j >= r.n_frames && c != 0)) { *why = "bad frame count"; return LIODOM_ERR_INVALID_ARG; }
    if (c > edge_cap) { *why = "a frame is larger than the handle's edge capacity"; return LIODOM_ERR_CAPACITY; }
    sum += c;
  }
  if (sum != r.n_points) { *why = "frame counts do not add up"; return LIODOM_ERR_INVALID_ARG; }
  if (r.n_recv > recv_cap) { *why = "received map larger than recv_capacity"; return LIODOM_ERR_CAPACITY; }
  if (rec) *rec = r;
  return LIODOM_OK;
}

// `fingerprint` (the six parameters set, the rest 0) made the header of a blob of total_bytes bytes.
inline StateBlobHeader state_header(StateBlobHeader fingerprint, uint64_t total_bytes) {
  memcpy(fingerprint.magic, "LIODOMST", 8);
  fingerprint.version = kStateBlobVersion; fingerprint.header_bytes = (uint32_t)kStateHeaderBytes; fingerprint.total_bytes = total_bytes;
  return fingerprint;
}
// The record k_state_pack has written behind the header at `prefix`, and whether its sizes are ones the handle can have produced.
inline bool state_packed_record(const unsigned char* prefix, int P, int edge_cap, int recv_cap, StateBlobRecord* rec) {
  memcpy(rec, prefix + kStateHeaderBytes, sizeof(*rec));
  return rec->n_points >= 0 && rec->n_points <= (long long)P * edge_cap && rec->n_recv >= 0 && rec->n_recv <= recv_cap;
}
// The record of a seeded stream (liodom_seed_stream; pose has passed pose7_check): quaternion normalised in double, the matrix
// by iso_from_qt — what the first scan's queries are transformed with and what its solve starts from, with no arithmetic in
// between (a zero-velocity prediction); no frame, no scan, n_recv 0.
inline StateBlobRecord state_seed_record(const double* pose) {
  StateBlobRecord rec;
  double p[7];
  memset(&rec, 0, sizeof(rec));
  pose7_normalised(pose, p);
  memcpy(rec.param_q, p, sizeof(rec.param_q)); memcpy(rec.param_t, p + 4, sizeof(rec.param_t));
  iso_from_qt(rec.param_q, rec.param_t, rec.odom);
  memcpy(rec.prev_odom, rec.odom, sizeof(rec.odom)); memcpy(rec.final_odom, rec.odom, sizeof(rec.odom));
  rec.initialized = 1; rec.imu_q[3] = 1.0;
  return rec;
}
// A seeded stream's blob up to its points (state_points_offset(P) bytes at `out`): the seed's record with a received map of
// n_recv points, every frame count 0; the header stays 0 (k_state_unpack reads none).
inline void state_seed_prefix(StateBlobRecord seed, int n_recv, int P, unsigned char* out) {
  seed.n_recv = n_recv;
  memset(out, 0, state_points_offset(P));
  memcpy(out + kStateHeaderBytes, &seed, sizeof(seed));
}

}  // namespace liodom_dev
