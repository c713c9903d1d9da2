// map_register.h — the plain-C++ half of liodom_map_register_poses (kernels in kernels_register.h, host entry point in
// liodom_map_host.h): the options' defaults and validation, and the sizes and byte offsets of the map's registration workspace,
// overflow-checked.  (The verdict that ends a row as converged is register_pass_converged in liodom_math.h.)  No HIP include:
// tests/map_register_main.cc compiles this file and that function, plain and under host sanitizers (tests/test_map_register_host.py).
//
// The workspace of a call with `rows` start poses, `local_cap` local-map points per row and room for `edge_cap` edges (the map's
// max_update_points: the edge staging is the map's d_in), one hipMalloc cut into sections, each 16-byte aligned, each [rows][...]:
//   pose      double[8]      the start pose, quaternion normalised (7 used)
//   T         double[12]     its matrix (iso_from_qt): what the row's local map is fetched around
//   count     int32[2 rows]  points written per row, then the full sizes (as liodom_map_get_local_batch keeps them)
//   pts       float4[local_cap]      the row's local map, in liodom_map_get_local order
//   order     int32[local_cap]       point indices grouped by 1 m voxel, ascending inside a voxel
//   slot      int32[local_cap]       table slot of point i (-1: not in the grid)
//   key       uint64[table]          open-addressing table of packed voxel keys; table = table_size(local_cap)
//   first     int32[table]           start of the slot's voxel in `order`
//   fill      int32[table]           points in the slot's voxel
//   corr      int32[2 edge_cap]      the current pass's (a, b) per edge
//   out       liodom_map_registration_t
// A row's grid uses the first table_size(points of the row) slots of its sections.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/liodom_hip.h"

namespace liodom_dev {

constexpr int kRegisterRowsMax = 64;
constexpr int kRegisterPassesMax = 16;
constexpr int kRegisterLocalDefault = 65536;
constexpr int kRegisterTableMin = 8;      // slots of the smallest table

inline void map_register_default(liodom_map_register_t* o) {
  memset(o, 0, sizeof(*o));
  o->cells_xy = 2; o->cells_z = 1;
  o->max_passes = 10;
  o->min_matches = 6;
  o->local_capacity = 0;
  o->stop_translation = 1e-4;
  o->stop_rotation = 1e-5;
  o->min_range = 3.0; o->max_range = 75.0;
}

// nullptr: the options are good.  Else the reason they are refused (LIODOM_ERR_INVALID_ARG).
inline const char* map_register_check(const liodom_map_register_t* o) {
  if (o->reserved != 0) return "reserved must be 0";
  if (o->cells_xy < 0 || o->cells_z < 0) return "negative extents";
  if (o->max_passes < 1 || o->max_passes > kRegisterPassesMax) return "max_passes outside 1 .. 16";
  if (o->min_matches < 1) return "min_matches below 1";
  if (o->local_capacity < 0) return "negative local_capacity";
  if (!(o->stop_translation >= 0.0) || !(o->stop_rotation >= 0.0) || !isfinite(o->stop_translation) || !isfinite(o->stop_rotation))
    return "negative or non-finite stop thresholds";
  if (!isfinite(o->min_range) || !isfinite(o->max_range) || !(o->min_range >= 0.0) || !(o->max_range > o->min_range))
    return "min_range / max_range are not 0 <= min < max";
  return nullptr;
}
inline int map_register_local_cap(const liodom_map_register_t* o) { return o->local_capacity == 0 ? kRegisterLocalDefault : o->local_capacity; }

// Slots of the table of a row of n points: the power of two >= 2 n, at least kRegisterTableMin.  n <= 2^29.
inline int64_t map_register_table_size(int64_t n) {
  int64_t t = kRegisterTableMin;
  while (t < 2 * n) t <<= 1;
  return t;
}

struct RegisterLayout {
  int rows, local_cap, edge_cap;
  int64_t table;                 // slots per row
  // byte offsets of the sections
  int64_t pose, T, count, pts, order, slot, key, first, fill, corr, out;
  int64_t bytes;
};

// false: a size does not fit (a row beyond 2^29 points — its table's slots are counted in an int on the device —, rows * local_cap
// beyond 2^31 - 1 points, or the bytes beyond 2^40): nothing is allocated.
inline bool map_register_layout(int rows, int local_cap, int edge_cap, RegisterLayout* L) {
  if (rows < 1 || rows > kRegisterRowsMax || local_cap < 1 || local_cap > (1 << 29) || edge_cap < 0) return false;
  if ((int64_t)rows * local_cap > 0x7fffffffll) return false;
  L->rows = rows; L->local_cap = local_cap; L->edge_cap = edge_cap;
  L->table = map_register_table_size(local_cap);
  int64_t at = 0;
  auto cut = [&](int64_t per_row) { const int64_t o = at; at += (((int64_t)rows * per_row) + 15) & ~(int64_t)15; return o; };
  L->pose = cut(8 * 8);
  L->T = cut(12 * 8);
  L->count = cut(2 * 4);
  L->pts = cut((int64_t)local_cap * 16);
  L->order = cut((int64_t)local_cap * 4);
  L->slot = cut((int64_t)local_cap * 4);
  L->key = cut(L->table * 8);
  L->first = cut(L->table * 4);
  L->fill = cut(L->table * 4);
  L->corr = cut((int64_t)(edge_cap > 0 ? edge_cap : 1) * 8);
  L->out = cut((int64_t)sizeof(liodom_map_registration_t));
  L->bytes = at;
  return at <= ((int64_t)1 << 40);
}

}  // namespace liodom_dev
