// place_state_format.h — a place database (liodom_places_t) as one contiguous blob: the descriptor's tables, the layout and the
// validator of untrusted bytes.  Plain C++: no HIP include, compiles for the host alone (tests/place_state_validate_main.cc does
// so under host sanitizers).  Included by liodom_places_host.h; the kernels that read the tables live in kernels_places.h.
// =============================================================================================
// Blob layout (little endian; every part starts on an 8-byte boundary; DESIGN.md §3 has the same table):
//   [0, 64)                    PlaceStateHeader   magic "LIODOMPL", version, header size, total size, the geometry's five numbers,
//                                                 the number of places
//   [64, 720)                  PlaceTables        float cs[32] (C_1..C_15 at 0..14, S_1..S_15 at 16..30), float r2[64] (R2_1..
//                                                 R2_n_rings), float z[68] (Z_0..Z_n_layers); every entry not named is 0.0f
//   [720, 720 + 8 W count)     uint64 desc[count][W]     W = n_rings * n_layers words per place: the bytes the match kernel reads
//   then                       PlaceStateRecord[count]   id, bit count, the pose the key frame was taken at
// The tables travel so that a reader of the blob (tests/place_model.py) compares with the very floats the kernels compare with;
// the validator recomputes them from the five numbers and refuses a blob in which they differ in any bit.
// =============================================================================================
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pose7.h"

#ifndef LIODOM_OK
#define LIODOM_OK 0
#endif
#ifndef LIODOM_ERR_INVALID_ARG
#define LIODOM_ERR_INVALID_ARG (-1)
#endif
#ifndef LIODOM_ERR_CAPACITY
#define LIODOM_ERR_CAPACITY (-3)
#endif

namespace liodom_dev {

constexpr uint32_t kPlaceStateVersion = 1u;
constexpr int kPlaceStateHeaderBytes = 64;
constexpr int kPlaceTablesBytes = 656;
constexpr int kPlaceRecordBytes = 72;
constexpr int kPlaceSectors = 64;          // a sector is a bit of a word
constexpr int kPlaceWordsMax = 64;         // W = n_rings * n_layers
constexpr int kPlacesMax = 1 << 20;        // places of a database, and rows of a call
constexpr int kPlaceKMax = 16;
constexpr double kPlacePi = 3.14159265358979323846;

struct PlaceStateHeader {
  char magic[8];                 // "LIODOMPL"
  uint32_t version;              // kPlaceStateVersion
  uint32_t header_bytes;         // 64
  uint64_t total_bytes;          // of the whole blob
  int32_t n_rings, n_layers;
  double r_max, z_min, z_max;
  int32_t count;                 // places
  int32_t reserved;              // 0
};
struct PlaceTables {
  float cs[32];                  // C_i = cs[i - 1], S_i = cs[16 + i - 1], i = 1 .. 15
  float r2[64];                  // R2_i = r2[i - 1], i = 1 .. n_rings
  float z[68];                   // Z_i = z[i], i = 0 .. n_layers
};
struct PlaceStateRecord {
  int64_t id;                    // the caller's tag
  int32_t bits;                  // popcount of the place's descriptor
  int32_t reserved;              // 0
  double pose[7];                // qx qy qz qw tx ty tz of the key frame
};
static_assert(sizeof(PlaceStateHeader) == kPlaceStateHeaderBytes, "place blob header is 64 bytes");
static_assert(sizeof(PlaceTables) == kPlaceTablesBytes, "place blob tables are 656 bytes");
static_assert(sizeof(PlaceStateRecord) == kPlaceRecordBytes, "place blob record is 72 bytes");

inline int64_t place_state_bytes(int64_t words, int64_t count) {
  return (int64_t)kPlaceStateHeaderBytes + (int64_t)kPlaceTablesBytes + (8 * words + (int64_t)kPlaceRecordBytes) * count;
}

// The five numbers a descriptor can be made with: 1 <= n_rings * n_layers <= 64, r_max > 0, z_min < z_max, all finite.
inline bool place_geometry_ok(int n_rings, int n_layers, double r_max, double z_min, double z_max) {
  if (n_rings < 1 || n_layers < 1 || n_rings > kPlaceWordsMax || n_layers > kPlaceWordsMax || n_rings * n_layers > kPlaceWordsMax) return false;
  if (!isfinite(r_max) || !isfinite(z_min) || !isfinite(z_max)) return false;
  return r_max > 0.0 && z_min < z_max;
}

// The tables of a geometry: made in double, rounded to float once.
inline void place_make_tables(int n_rings, int n_layers, double r_max, double z_min, double z_max, PlaceTables* t) {
  memset(t, 0, sizeof(*t));
  for (int i = 1; i <= 15; i++) {
    t->cs[i - 1] = (float)cos((double)i * kPlacePi / 32.0);
    t->cs[16 + i - 1] = (float)sin((double)i * kPlacePi / 32.0);
  }
  for (int i = 1; i <= n_rings; i++) {
    const double r = (double)i * r_max / (double)n_rings;
    t->r2[i - 1] = (float)(r * r);
  }
  for (int i = 0; i <= n_layers; i++) t->z[i] = (float)(z_min + (double)i * (z_max - z_min) / (double)n_layers);
}

inline int place_popcount64(uint64_t v) {
  int n = 0;
  for (; v; v &= v - 1) n++;
  return n;
}

// The one place where untrusted blob bytes are parsed.  Checks `blob` (`bytes` long; no byte beyond is read, and no alignment is
// assumed).  geom (optional: five numbers as n_rings, n_layers, r_max, z_min, z_max of the database that is to take the blob) must
// match the blob's bit for bit; max_places < 0: no capacity check.  LIODOM_OK; LIODOM_ERR_INVALID_ARG for anything that is not a
// well-formed blob (of that geometry); LIODOM_ERR_CAPACITY for a well-formed one with more places than max_places.  *why
// (optional) names the reason.
inline int place_state_validate(const void* blob, int64_t bytes, const int32_t* geom_nm, const double* geom_rz, int64_t max_places,
                                const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  if (!b || bytes < (int64_t)kPlaceStateHeaderBytes) { *why = "place-state blob truncated"; return LIODOM_ERR_INVALID_ARG; }
  PlaceStateHeader hd;
  memcpy(&hd, b, sizeof(hd));
  if (memcmp(hd.magic, "LIODOMPL", 8) != 0) { *why = "not a place-state blob (bad magic)"; return LIODOM_ERR_INVALID_ARG; }
  if (hd.version != kPlaceStateVersion || hd.header_bytes != (uint32_t)kPlaceStateHeaderBytes) {
    *why = "place-state blob of another version"; return LIODOM_ERR_INVALID_ARG;
  }
  if (hd.total_bytes != (uint64_t)bytes) { *why = "place-state blob: total_bytes is not the blob's size"; return LIODOM_ERR_INVALID_ARG; }
  if (bytes < (int64_t)kPlaceStateHeaderBytes + (int64_t)kPlaceTablesBytes) { *why = "place-state blob truncated"; return LIODOM_ERR_INVALID_ARG; }
  if (!place_geometry_ok(hd.n_rings, hd.n_layers, hd.r_max, hd.z_min, hd.z_max)) {
    *why = "place-state blob: not a geometry (1 <= n_rings * n_layers <= 64, r_max > 0, z_min < z_max, all finite)"; return LIODOM_ERR_INVALID_ARG;
  }
  if (hd.reserved != 0) { *why = "place-state blob: reserved header word is not 0"; return LIODOM_ERR_INVALID_ARG; }
  const int64_t words = (int64_t)hd.n_rings * hd.n_layers;
  // sizes, without ever forming a product that could overflow
  const int64_t rest = bytes - (int64_t)kPlaceStateHeaderBytes - (int64_t)kPlaceTablesBytes, per_place = 8 * words + (int64_t)kPlaceRecordBytes;
  if (hd.count < 0 || rest % per_place != 0 || (int64_t)hd.count != rest / per_place) {
    *why = "place-state blob: sizes do not add up"; return LIODOM_ERR_INVALID_ARG;
  }
  PlaceTables want, have;
  place_make_tables(hd.n_rings, hd.n_layers, hd.r_max, hd.z_min, hd.z_max, &want);
  memcpy(&have, b + kPlaceStateHeaderBytes, sizeof(have));
  if (memcmp(&want, &have, sizeof(want)) != 0) {
    *why = "place-state blob: the tables are not the ones its geometry gives"; return LIODOM_ERR_INVALID_ARG;
  }
  if (geom_nm && geom_rz) {
    const double theirs[3] = {hd.r_max, hd.z_min, hd.z_max};
    if (geom_nm[0] != hd.n_rings || geom_nm[1] != hd.n_layers || memcmp(geom_rz, theirs, sizeof(theirs)) != 0) {
      *why = "place-state blob comes from a database with another geometry (the five numbers must match bit for bit)";
      return LIODOM_ERR_INVALID_ARG;
    }
  }
  const unsigned char* desc = b + kPlaceStateHeaderBytes + kPlaceTablesBytes;
  const unsigned char* recs = desc + 8 * words * (int64_t)hd.count;
  for (int64_t p = 0; p < (int64_t)hd.count; p++) {
    PlaceStateRecord r;
    memcpy(&r, recs + p * (int64_t)kPlaceRecordBytes, sizeof(r));
    int bits = 0;
    for (int64_t w = 0; w < words; w++) {
      uint64_t v;
      memcpy(&v, desc + 8 * (p * words + w), sizeof(v));
      bits += place_popcount64(v);
    }
    if (r.bits != bits) { *why = "place-state blob: a bit count is not the popcount of its descriptor"; return LIODOM_ERR_INVALID_ARG; }
    if (r.reserved != 0) { *why = "place-state blob: reserved record word is not 0"; return LIODOM_ERR_INVALID_ARG; }
    if (pose7_check(r.pose) != kPose7Ok) { *why = "place-state blob: a pose is non-finite or its quaternion is not normalised"; return LIODOM_ERR_INVALID_ARG; }
  }
  if (max_places >= 0 && (int64_t)hd.count > max_places) { *why = "place-state blob holds more places than max_places"; return LIODOM_ERR_CAPACITY; }
  return LIODOM_OK;
}

// The pose a match stands for: place_pose o Rz(shift * 2 pi / 64), in double: the place's quaternion normalised as
// liodom_seed_stream normalises a seed, times (0, 0, sin(a / 2), cos(a / 2)); the translation is the place's.
inline void place_match_pose(const double* place_pose, int shift, double* out) {
  const double norm = pose7_norm(place_pose);
  const double ax = place_pose[0] / norm, ay = place_pose[1] / norm, az = place_pose[2] / norm, aw = place_pose[3] / norm;
  const double a = (double)shift * (2.0 * kPlacePi / 64.0);
  const double bz = sin(a / 2.0), bw = cos(a / 2.0);
  out[0] = ax * bw + ay * bz;       // quaternion product a * (0, 0, bz, bw)
  out[1] = ay * bw - ax * bz;
  out[2] = aw * bz + az * bw;
  out[3] = aw * bw - az * bz;
  for (int i = 0; i < 3; i++) out[4 + i] = place_pose[4 + i];
}

}  // namespace liodom_dev
