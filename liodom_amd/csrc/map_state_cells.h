// map_state_cells.h — a map-state blob (map_state_format.h) taken apart into cells and put together from cells: what a host-side
// store of paged-out cells needs (liodom::MapPager in host/liodom_host.cc; liodom_amd/pager.py does the same in Python).
// Plain C++, no HIP include: tests/map_state_cells_main.cc compiles it for the host alone under sanitizers.
#pragma once
#include <limits.h>

#include <array>
#include <vector>

#include "map_state_format.h"

namespace liodom_dev {

// One cell as it travels in a blob.  corner_leaf is kept as given: it cannot be re-derived from the points (map_state_format.h).
struct MapStateCell {
  std::array<int32_t, 3> key{};
  std::array<int32_t, 3> corner_leaf{};
  std::vector<float> xyzi;               // 4 floats per point, the cell's cloud in its order
  int count() const { return (int)(xyzi.size() / 4); }
};

// Splits `blob` (`bytes` long, untrusted) into its cells, in blob order.  The bytes go through map_state_validate first — against
// the three sizes given, without capacity limits — and nothing is read before it has accepted them.  Returns its code; *why
// (optional) names the reason.  `cells` is cleared first and stays empty on failure.
inline int map_state_split(const void* blob, int64_t bytes, double xy, double z, double res, std::vector<MapStateCell>* cells,
                           uint32_t* status, const char** why) {
  if (cells) cells->clear();
  const int rc = map_state_validate(blob, bytes, xy, z, res, INT_MAX, INT_MAX, why);
  if (rc != LIODOM_OK) return rc;
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  MapStateHeader hd;
  memcpy(&hd, b, sizeof(hd));
  if (status) *status = hd.status;
  if (!cells) return LIODOM_OK;
  const unsigned char* pts = b + map_state_bytes(hd.n_cells, 0);
  cells->resize((size_t)hd.n_cells);
  for (int c = 0; c < hd.n_cells; c++) {
    MapStateRecord r;
    memcpy(&r, b + kMapStateHeaderBytes + (size_t)c * kMapStateRecordBytes, sizeof(r));
    MapStateCell& out = (*cells)[(size_t)c];
    for (int a = 0; a < 3; a++) { out.key[(size_t)a] = r.key[a]; out.corner_leaf[(size_t)a] = r.corner_leaf[a]; }
    out.xyzi.resize(4 * (size_t)r.count);      // (the validator has checked first / count against the blob's size)
    if (r.count > 0) memcpy(out.xyzi.data(), pts + 16 * (size_t)r.first, 16 * (size_t)r.count);
  }
  return LIODOM_OK;
}

// Writes the blob of `cells` (pointers, in the order given) for a map of the three sizes: `first` is recomputed, everything else
// travels as it is.  The caller sees to it that the keys are distinct.
inline std::vector<unsigned char> map_state_join(double xy, double z, double res, const std::vector<const MapStateCell*>& cells, uint32_t status) {
  int64_t n_points = 0;
  for (const MapStateCell* c : cells) n_points += c->count();
  const int64_t total = map_state_bytes((int64_t)cells.size(), n_points);
  std::vector<unsigned char> out((size_t)total);
  MapStateHeader hd;
  memset(&hd, 0, sizeof(hd));
  memcpy(hd.magic, "LIODOMMP", 8);
  hd.version = kMapStateVersion; hd.header_bytes = (uint32_t)kMapStateHeaderBytes; hd.total_bytes = (uint64_t)total;
  hd.voxel_xysize = xy; hd.voxel_zsize = z; hd.resolution = res;
  hd.n_cells = (int32_t)cells.size(); hd.status = status; hd.n_points = n_points;
  memcpy(out.data(), &hd, sizeof(hd));
  unsigned char* pts = out.data() + map_state_bytes((int64_t)cells.size(), 0);
  int64_t first = 0;
  for (size_t c = 0; c < cells.size(); c++) {
    MapStateRecord r;
    for (int a = 0; a < 3; a++) { r.key[a] = cells[c]->key[(size_t)a]; r.corner_leaf[a] = cells[c]->corner_leaf[(size_t)a]; }
    r.count = cells[c]->count();
    r.first = (int32_t)first;
    memcpy(out.data() + kMapStateHeaderBytes + c * (size_t)kMapStateRecordBytes, &r, sizeof(r));
    if (r.count > 0) memcpy(pts + 16 * (size_t)first, cells[c]->xyzi.data(), 16 * (size_t)r.count);
    first += r.count;
  }
  return out;
}

}  // namespace liodom_dev
