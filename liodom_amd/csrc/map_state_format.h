// map_state_format.h — the device map (liodom_map_t) as one contiguous blob: layout and the validator of untrusted bytes.
// Plain C++: no HIP include, compiles for the host alone (tests/map_state_validate_main.cc does so under host sanitizers).
// Included by liodom_map.h; the kernels that write and read the blob (k_map_pack_plan / k_map_pack / k_map_unpack) live there.
// =============================================================================================
// Blob layout (little endian; every part starts on a 16-byte boundary; DESIGN.md §3 has the same table):
//   [0, 64)                  MapStateHeader   magic "LIODOMMP", version, total size, the fingerprint (voxel sizes and resolution:
//                                             must match bit for bit on import), n_cells, sticky status bits, n_points
//   [64, 64 + 32 n_cells)    MapStateRecord   one per cell IN CREATION ORDER (cells_vector_ order = cell id): key, leaf coordinates
//                                             of the cell's lower corner, points in the cell, index of its first point below
//   then                     float4 points[n_points]   the cells' current clouds back to back in creation order: exactly the
//                                             bytes liodom_map_get_all returns
// The blob holds the LOGICAL map only.  Which of the two slabs of a cell is current, hash-slot positions, the margin of the dense
// leaf grid and all update scratch do not travel, so a blob fits any map with the same three sizes, whatever its capacities.
// corner_leaf is stored and not recomputed on import: a stored centroid can round onto a cell face, so the corner cannot be
// derived safely from the points.
// =============================================================================================
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

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

constexpr uint32_t kMapStateVersion = 1u;
constexpr int kMapStateHeaderBytes = 64;
constexpr int kMapStateRecordBytes = 32;
constexpr int kMapKeyLimit = 1 << 20;      // cell keys live in [-2^20, 2^20): 21 bits each in the packed hash key

struct MapStateHeader {
  char magic[8];                 // "LIODOMMP"
  uint32_t version;              // kMapStateVersion
  uint32_t header_bytes;         // 64
  uint64_t total_bytes;          // of the whole blob
  double voxel_xysize, voxel_zsize, resolution;      // the fingerprint
  int32_t n_cells;
  uint32_t status;               // the sticky LIODOM_MAP_* bits as liodom_map_status reports them
  int64_t n_points;              // sum of the cells' counts
};
struct MapStateRecord {
  int32_t key[3];                // voxel_x, voxel_y, voxel_z as the reference computes them (map.cc:103-105)
  int32_t corner_leaf[3];        // leaf coordinates of the cell's lower corner
  int32_t count;                 // points in the cell
  int32_t first;                 // index of the cell's first point in the point section: exclusive prefix sum of count
};
static_assert(sizeof(MapStateHeader) == kMapStateHeaderBytes, "map blob header is 64 bytes");
static_assert(sizeof(MapStateRecord) == kMapStateRecordBytes, "map blob cell record is 32 bytes");

inline int64_t map_state_bytes(int64_t n_cells, int64_t n_points) {
  return (int64_t)kMapStateHeaderBytes + (int64_t)kMapStateRecordBytes * n_cells + 16 * n_points;
}

// The one place where untrusted blob bytes are parsed.  Checks `blob` (`bytes` long; no byte beyond is read, and no alignment is
// assumed) against the three sizes and the capacities of the map that is to take it.  LIODOM_OK; LIODOM_ERR_INVALID_ARG for
// anything that is not a well-formed blob of a map with these sizes; LIODOM_ERR_CAPACITY for a well-formed one this map cannot
// hold.  *why (optional) names the reason.
inline int map_state_validate(const void* blob, int64_t bytes, double xy, double z, double res, int max_cells, int cell_capacity,
                              const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  if (!b || bytes < (int64_t)kMapStateHeaderBytes) { *why = "map-state blob truncated"; return LIODOM_ERR_INVALID_ARG; }
  MapStateHeader hd;
  memcpy(&hd, b, sizeof(hd));
  if (memcmp(hd.magic, "LIODOMMP", 8) != 0) { *why = "not a map-state blob (bad magic)"; return LIODOM_ERR_INVALID_ARG; }
  if (hd.version != kMapStateVersion || hd.header_bytes != (uint32_t)kMapStateHeaderBytes) {
    *why = "map-state blob of another version"; return LIODOM_ERR_INVALID_ARG;
  }
  if (hd.total_bytes != (uint64_t)bytes) { *why = "map-state blob: total_bytes is not the blob's size"; return LIODOM_ERR_INVALID_ARG; }
  // sizes, without ever forming a product that could overflow
  int64_t rest = bytes - (int64_t)kMapStateHeaderBytes;
  if (hd.n_cells < 0 || hd.n_points < 0 || (int64_t)hd.n_cells > rest / kMapStateRecordBytes) {
    *why = "map-state blob: sizes do not add up"; return LIODOM_ERR_INVALID_ARG;
  }
  rest -= (int64_t)kMapStateRecordBytes * hd.n_cells;
  if (rest % 16 != 0 || hd.n_points != rest / 16) { *why = "map-state blob: sizes do not add up"; return LIODOM_ERR_INVALID_ARG; }
  const double mine[3] = {xy, z, res}, theirs[3] = {hd.voxel_xysize, hd.voxel_zsize, hd.resolution};
  if (memcmp(mine, theirs, sizeof(mine)) != 0) {
    *why = "map-state blob comes from a map with other sizes (voxel_xysize, voxel_zsize, resolution must match bit for bit)";
    return LIODOM_ERR_INVALID_ARG;
  }
  const int n = hd.n_cells;
  std::vector<uint64_t> keys((size_t)n);
  int64_t run = 0;
  int max_count = 0;
  for (int c = 0; c < n; c++) {
    MapStateRecord r;
    memcpy(&r, b + kMapStateHeaderBytes + (size_t)c * kMapStateRecordBytes, sizeof(r));
    if (r.count < 0) { *why = "map-state blob: negative cell count"; return LIODOM_ERR_INVALID_ARG; }
    if ((int64_t)r.first != run) { *why = "map-state blob: first is not the prefix sum of the counts"; return LIODOM_ERR_INVALID_ARG; }
    run += r.count;
    for (int a = 0; a < 3; a++) {
      if (r.key[a] < -kMapKeyLimit || r.key[a] >= kMapKeyLimit) { *why = "map-state blob: cell key beyond +-2^20"; return LIODOM_ERR_INVALID_ARG; }
    }
    keys[(size_t)c] = ((uint64_t)(uint32_t)(r.key[0] + kMapKeyLimit) << 42) | ((uint64_t)(uint32_t)(r.key[1] + kMapKeyLimit) << 21) |
                      (uint64_t)(uint32_t)(r.key[2] + kMapKeyLimit);
    max_count = std::max(max_count, r.count);
  }
  if (run != hd.n_points) { *why = "map-state blob: cell counts do not add up to n_points"; return LIODOM_ERR_INVALID_ARG; }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) { *why = "map-state blob: duplicate cell key"; return LIODOM_ERR_INVALID_ARG; }
  if (n > max_cells) { *why = "map-state blob holds more cells than max_cells"; return LIODOM_ERR_CAPACITY; }
  if (max_count > cell_capacity) { *why = "map-state blob holds a cell larger than cell_capacity"; return LIODOM_ERR_CAPACITY; }
  return LIODOM_OK;
}

}  // namespace liodom_dev
