// Host side of the device map (C-ABI liodom_map_* of include/liodom_hip.h).  Included by
// liodom_hip.hip (same translation unit: shares HIP_TRY / g_last_error).
#pragma once
#include <chrono>

#include "liodom_map.h"
#include "map_attach.h"
#include "reloc_candidates.h"
#include "reloc_bnb.h"
#include "map_register.h"

struct liodom_map {
  liodom_map_config_t cfg;
  liodom_dev::MapView m{};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int device = 0;
  std::vector<void*> allocs;
  // staging of the host entry points
  float4* d_in = nullptr;
  int* d_n = nullptr;
  double* d_T = nullptr;
  float4* d_out = nullptr;
  int out_cap = 0;
  int* d_out_n = nullptr;
  unsigned char* d_head = nullptr;   // header + max_cells cell records of a map-state blob (first export / import allocates it)
  liodom_dev::MapPruneMove* d_prune = nullptr;   // max_cells + 1 move records of a prune (the first prune, or an attach with auto-prune, allocates it)
  unsigned char* d_batch = nullptr;  // liodom_map_get_local_batch: n poses, then 2 n counts (the first call allocates it, a larger one regrows it)
  size_t batch_bytes = 0;
  unsigned int* d_occ = nullptr;     // liodom_map_score_poses / _search_pose: leaf occupancy [occ_cells][words] (the first call allocates it for
  int occ_cells = 0;                 // the cells the map holds then, a map that has grown since regrows it)
  // the kept occupancy of the per-scan hit records (liodom_set_map_hits): every entry point and enqueue that can change the cells
  // bumps `gen`; d_occ holds the occupancy of the map as it was at generation occ_gen (0: of none).  Host-side, under the caller's
  // threading rule for the map.
  unsigned long long gen = 1, occ_gen = 0;
  unsigned long long* d_blocks = nullptr;   // liodom_map_search_pose_bnb / _bound_nodes: the block tables of the levels a call uses (the
  size_t blocks_entries = 0;               // first call allocates them, a call that needs more regrows them)
  unsigned char* h_pin = nullptr;          // liodom_map_search_pose_bnb: pinned host staging of a round's nodes, candidates and counts
  size_t pin_bytes = 0;
  unsigned char* d_reg = nullptr;          // liodom_map_register_poses: the workspace map_register.h lays out (the first call allocates
  size_t reg_bytes = 0;                    // it, a call whose n x local_capacity needs more regrows it)
  // attachments to a handle's streams (liodom_attach_mapper* / liodom_attach_map_reader, map_attach.h): the map runs on the
  // handle's HIP stream while link.n_attached > 0 and gets one of its own again when the last attachment goes
  liodom_dev::MapLink link;
};

namespace {

using liodom_dev::MapView;

int map_alloc(liodom_map* mp, void** out, size_t bytes) {
  void* raw = nullptr;
  HIP_TRY(hipMalloc(&raw, bytes ? bytes : 16));
  mp->allocs.push_back(raw);
  *out = raw;
  return LIODOM_OK;
}
#define MAP_ALLOC(ptr, count)                                                                  \
  do {                                                                                         \
    void* _raw = nullptr;                                                                      \
    int _rc = map_alloc(mp, &_raw, sizeof(*(ptr)) * (size_t)(count));                          \
    if (_rc) return _rc;                                                                       \
    (ptr) = reinterpret_cast<decltype(ptr)>(_raw);                                             \
  } while (0)

int map_build(liodom_map* mp, const liodom_map_config_t* c, hipStream_t stream) {
  mp->cfg = *c;
  MapView& m = mp->m;
  m.xy = c->voxel_xysize; m.inv_xy = 1.0 / c->voxel_xysize; m.half_xy = c->voxel_xysize / 2.0;     // map.cc:71-73
  m.z = c->voxel_zsize;   m.inv_z = 1.0 / c->voxel_zsize;   m.half_z = c->voxel_zsize / 2.0;       // :74-76
  const float leaf = (float)c->resolution;               // setLeafSize(float, float, float), :80
  m.leaf_inv = 1.0f / leaf;                              // PCL inverse_leaf_size_
  m.gx = m.gy = (int)std::ceil((float)c->voxel_xysize * m.leaf_inv) + 1 + 2 * liodom_dev::kMapLeafMargin;
  m.gz = (int)std::ceil((float)c->voxel_zsize * m.leaf_inv) + 1 + 2 * liodom_dev::kMapLeafMargin;
  const long long leaves = (long long)m.gx * m.gy * m.gz;
  if (leaves > (1ll << 28)) { g_last_error = "liodom_map_create: voxel size / resolution gives more than 2^28 leaves per cell"; return LIODOM_ERR_INVALID_ARG; }
  m.words = (int)((leaves + 31) / 32);
  m.max_cells = c->max_cells; m.cell_cap = c->cell_capacity; m.upd_cap = c->max_update_points; m.mod_cap = c->max_modified_cells;
  int ct = 64;
  while (ct < 4 * m.max_cells) ct <<= 1;
  m.ctable = ct;
  if (stream) { mp->stream = stream; mp->own_stream = false; }
  else { HIP_TRY(hipStreamCreateWithFlags(&mp->stream, hipStreamNonBlocking)); mp->own_stream = true; }
  MAP_ALLOC(m.st, 1);
  MAP_ALLOC(m.ckey, m.ctable); MAP_ALLOC(m.cslot_cell, m.ctable); MAP_ALLOC(m.cfirst, m.ctable);
  MAP_ALLOC(m.cell_key, 3 * (size_t)m.max_cells); MAP_ALLOC(m.cell_org, 3 * (size_t)m.max_cells);
  MAP_ALLOC(m.cell_n, m.max_cells); MAP_ALLOC(m.cell_buf, m.max_cells);
  MAP_ALLOC(m.slab, 2 * (size_t)m.max_cells * m.cell_cap);
  MAP_ALLOC(m.new_pts, m.upd_cap); MAP_ALLOC(m.new_cell, m.upd_cap); MAP_ALLOC(m.new_mi, m.upd_cap);
  MAP_ALLOC(m.new_pos, m.upd_cap); MAP_ALLOC(m.new_rank, m.upd_cap);
  MAP_ALLOC(m.mod_list, m.mod_cap); MAP_ALLOC(m.mod_of_cell, m.max_cells); MAP_ALLOC(m.mod_out_n, m.mod_cap);
  MAP_ALLOC(m.bitmap, (size_t)m.mod_cap * m.words); MAP_ALLOC(m.wprefix, (size_t)m.mod_cap * m.words);
  MAP_ALLOC(m.old_pos, (size_t)m.mod_cap * m.cell_cap); MAP_ALLOC(m.old_rank, (size_t)m.mod_cap * m.cell_cap);
  MAP_ALLOC(m.leaf_cnt, (size_t)m.mod_cap * m.cell_cap); MAP_ALLOC(m.leaf_start, (size_t)m.mod_cap * m.cell_cap);
  // Member lists of one update.  k_map_alloc advances `cursor` by leaf_cnt for every output leaf with more than one point and
  // counts such a leaf in n_multi.  Every item of the update — an old point of a modified cell or a new point — is counted into
  // at most one leaf_cnt (k_map_count), so cursor <= items <= sum over the n_mod modified cells of cell_n + n_new
  // <= mod_cap * cell_cap + upd_cap: old AND new points, e.g. a full cell of single-point leaves that each receive one more
  // point.  A leaf in `multi` holds at least two items, so n_multi <= that / 2.  The three factors are the dimensions of the
  // arrays the items are read from (mod_list, a slab, new_pts): the bound holds whatever an update contains and whichever
  // status bits it raises, and needs no relation between max_update_points and the other capacities.
  const size_t items_max = (size_t)m.mod_cap * m.cell_cap + (size_t)m.upd_cap;
  MAP_ALLOC(m.members, items_max);
  MAP_ALLOC(m.multi, (items_max + 1) / 2);
  MAP_ALLOC(m.entries, liodom_dev::kMapLocalEntriesMax);
  const int n_init = std::max(m.ctable, m.max_cells);
  hipLaunchKernelGGL(liodom_dev::k_map_init, dim3((n_init + 255) / 256), dim3(256), 0, mp->stream, m);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// Map::updateMap enqueued on `q`: points, their count and the pose are read from device memory.
// d_T == nullptr: the points are in the world frame already and enter the map as they are (the lagged mapper).
int map_enqueue_update(liodom_map* mp, const float4* d_pts, const int* d_n, const double* d_T, hipStream_t q) {
  using namespace liodom_dev;
  const MapView& m = mp->m;
  mp->gen++;
  const int xb_old = (m.cell_cap + 255) / 256, xb_new = (m.upd_cap + 255) / 256;
  const int xb = std::max(xb_old, xb_new);
  if (d_T) hipLaunchKernelGGL(k_map_assign<true>, dim3(1), dim3(1024), 0, q, m, d_pts, d_n, d_T);
  else hipLaunchKernelGGL(k_map_assign<false>, dim3(1), dim3(1024), 0, q, m, d_pts, d_n, d_T);
  hipLaunchKernelGGL(k_map_clear, dim3(std::min(64, std::max((m.words + 255) / 256, xb_old)), m.mod_cap), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_setbits, dim3(xb, m.mod_cap + 1), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_prefix, dim3(m.mod_cap), dim3(1024), 0, q, m);
  hipLaunchKernelGGL(k_map_count, dim3(xb, m.mod_cap + 1), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_alloc, dim3(xb_old, m.mod_cap), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_emit, dim3(xb, m.mod_cap + 1), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_centroid, dim3(512), dim3(256), 0, q, m);
  hipLaunchKernelGGL(k_map_commit, dim3(1), dim3(256), 0, q, m);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// Map::getLocalMap enqueued on `q`: result and its size stay on the device.
int map_enqueue_local(liodom_map* mp, const double* d_T, int cells_xy, int cells_z, float4* d_out, int out_cap,
                      int* d_out_n, hipStream_t q, int sticky_overflow) {
  using namespace liodom_dev;
  hipLaunchKernelGGL(k_map_local_plan, dim3(1), dim3(64), 0, q, mp->m, d_T, cells_xy, cells_z, out_cap, d_out_n, sticky_overflow);
  hipLaunchKernelGGL(k_map_gather, dim3((mp->m.cell_cap + 255) / 256 > 64 ? 64 : (mp->m.cell_cap + 255) / 256, 64), dim3(256), 0, q, mp->m, d_out, out_cap);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// Whether the visit of getLocalMap(., cells_xy, cells_z) fits the LDS plan of k_map_local_rows for EVERY pose.  With both sizes
// >= 1 a loop variable advances by at least floor(size) per iteration ((int)(i + size) >= i + floor(size) on either side of 0),
// and a loop's ends lie at most 2 * cells * xy + 2 apart (each end is truncated once).  So the square visits at most nx * nx keys
// and the column nz, with the bounds below; anything else takes k_map_local_plan + k_map_gather.
bool map_rows_fit(const liodom_map* mp, int cells_xy, int cells_z) {
  const double xy = mp->cfg.voxel_xysize, z = mp->cfg.voxel_zsize;
  if (!(xy >= 1.0) || !(z >= 1.0) || cells_xy < 0 || cells_z < 0) return false;
  const double nx = std::floor((2.0 * cells_xy * xy + 2.0) / std::floor(xy)) + 1.0;
  const double nz = std::floor((2.0 * cells_z * xy + 2.0) / std::floor(z)) + 1.0;
  return nx * nx + nz <= (double)liodom_dev::kMapRowsKeysMax;
}

// x extent of a k_map_local_rows launch over `rows` rows of up to `cap` points: a row's copy is dealt to at most kMapRowsGridX
// workgroups, the launch stays within kMapRowsGridMax, and no workgroup is launched for less than one round of its threads.
int map_rows_grid_x(int rows, int cap) {
  using namespace liodom_dev;
  const int by_cap = std::max(1, (cap + kMapRowsThreads - 1) / kMapRowsThreads);
  return std::max(1, std::min(std::min(kMapRowsGridX, by_cap), kMapRowsGridMax / std::max(1, rows)));
}

int map_ensure_out(liodom_map* mp, int64_t cap) {
  if (cap > 0x7fffffff) cap = 0x7fffffff;
  if (mp->d_out && mp->out_cap >= cap) return LIODOM_OK;
  if (mp->d_out) { (void)hipFree(mp->d_out); mp->d_out = nullptr; }
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mp->d_out), sizeof(float4) * (size_t)std::max<int64_t>(cap, 1)));
  mp->out_cap = (int)cap;
  return LIODOM_OK;
}

// d_batch with room for `need` bytes: n poses, then per-pose ints (liodom_map_get_local_batch, liodom_map_score_poses)
int map_ensure_batch(liodom_map* mp, size_t need) {
  if (mp->batch_bytes >= need) return LIODOM_OK;
  HIP_TRY(hipStreamSynchronize(mp->stream));
  if (mp->d_batch) { (void)hipFree(mp->d_batch); mp->d_batch = nullptr; mp->batch_bytes = 0; }
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mp->d_batch), need));
  mp->batch_bytes = need;
  return LIODOM_OK;
}

void map_free(liodom_map* mp) {
  if (!mp) return;
  (void)hipSetDevice(mp->device);
  if (mp->stream) (void)hipStreamSynchronize(mp->stream);
  for (void* p : mp->allocs) (void)hipFree(p);
  if (mp->d_out) (void)hipFree(mp->d_out);
  if (mp->d_batch) (void)hipFree(mp->d_batch);
  if (mp->d_occ) (void)hipFree(mp->d_occ);
  if (mp->d_blocks) (void)hipFree(mp->d_blocks);
  if (mp->h_pin) (void)hipHostFree(mp->h_pin);
  if (mp->d_reg) (void)hipFree(mp->d_reg);
  if (mp->own_stream && mp->stream) (void)hipStreamDestroy(mp->stream);
  delete mp;
}

int map_fetch_result(liodom_map* mp, float* xyzi, int64_t cap, int64_t* n_points) {
  int n = 0;
  HIP_TRY(hipMemcpyAsync(&n, mp->d_out_n, sizeof(int), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  liodom_dev::MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  if (n_points) *n_points = st.n_result;
  if ((int64_t)st.n_result > cap) { g_last_error = "liodom_map: output buffer too small"; return LIODOM_ERR_CAPACITY; }
  if (n > 0 && xyzi) HIP_TRY(hipMemcpy(xyzi, mp->d_out, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}


// ---- the map as a blob (map_state_format.h; kernels at the end of liodom_map.h) ----
int map_ensure_head(liodom_map* mp) {
  if (mp->d_head) return LIODOM_OK;
  void* raw = nullptr;
  int rc = map_alloc(mp, &raw, (size_t)liodom_dev::map_state_bytes(mp->m.max_cells, 0));
  if (rc) return rc;
  mp->d_head = static_cast<unsigned char*>(raw);
  return LIODOM_OK;
}

// ---- pruning (kernels at the end of liodom_map.h) ----
int map_ensure_prune(liodom_map* mp) {
  if (mp->d_prune) return LIODOM_OK;
  void* raw = nullptr;
  int rc = map_alloc(mp, &raw, sizeof(liodom_dev::MapPruneMove) * ((size_t)mp->m.max_cells + 1));
  if (rc) return rc;
  mp->d_prune = static_cast<liodom_dev::MapPruneMove*>(raw);
  return LIODOM_OK;
}

// Drops every cell outside the keep box around the pose at d_T (device memory), enqueued on `q`; map_ensure_prune has run.
int map_enqueue_prune(liodom_map* mp, const double* d_T, int keep_xy, int keep_z, hipStream_t q) {
  using namespace liodom_dev;
  const MapView& m = mp->m;
  mp->gen++;
  const int clear_blocks = std::min(64, (m.ctable + kMapPruneThreads - 1) / kMapPruneThreads);
  hipLaunchKernelGGL(k_map_prune_plan, dim3(1 + clear_blocks), dim3(kMapPruneThreads), 0, q, m, d_T, keep_xy, keep_z, mp->d_prune);
  hipLaunchKernelGGL(k_map_prune_move, dim3(std::min(16, (m.cell_cap + 255) / 256), std::min(m.max_cells, 256)), dim3(256), 0, q, m, mp->d_prune);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// LIODOM_MAP_STATE_TIMING=1: export and import report the HIP-event time of their kernels on stderr (the figures of DESIGN.md §3)
struct MapStateTimer {
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t q;
  const char* what;
  MapStateTimer(hipStream_t q_, const char* what_) : q(q_), what(what_) {
    const char* e = std::getenv("LIODOM_MAP_STATE_TIMING");
    if (e && e[0] == '1' && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(a, q);
  }
  bool stopped = false;
  void stop() { if (b) { (void)hipEventRecord(b, q); stopped = true; } }
  ~MapStateTimer() {
    float ms = 0.f;
    // (a call that returned early never recorded `b`: asking for its time would leave a HIP error for the next launch check to find)
    if (stopped && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) std::fprintf(stderr, "%s: kernels %.3f ms\n", what, ms);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// Plans a blob of the map as it is now: the cell records into d_head, the header's n_cells / status / n_points to the host.
int map_state_plan(liodom_map* mp, liodom_dev::MapStateHeader* hd, const char* who) {
  int rc = map_ensure_head(mp);
  if (rc) return rc;
  hipLaunchKernelGGL(liodom_dev::k_map_pack_plan, dim3(1), dim3(1024), 0, mp->stream, mp->m, mp->d_head);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hd, mp->d_head, sizeof(*hd), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  if (hd->n_cells < 0 || hd->n_cells > mp->m.max_cells || hd->n_points < 0 || hd->n_points > (int64_t)hd->n_cells * mp->m.cell_cap) {
    g_last_error = std::string(who) + ": inconsistent map state"; return LIODOM_ERR_HIP;
  }
  if (hd->n_points > 0x7fffffff) { g_last_error = std::string(who) + ": more than 2^31 - 1 points do not fit the blob format"; return LIODOM_ERR_CAPACITY; }
  return LIODOM_OK;
}

// The empty map of liodom_map_create (k_map_init), then — with a validated blob — its cells and points (k_map_unpack).
int map_install_state(liodom_map* mp, const unsigned char* blob, const liodom_dev::MapStateHeader* hd) {
  using namespace liodom_dev;
  const MapView& m = mp->m;
  const int n_cells = hd ? hd->n_cells : 0, n_points = hd ? (int)hd->n_points : 0;
  mp->gen++;
  if (n_cells > 0) {
    // everything that can fail comes before the map is touched
    int rc = map_ensure_head(mp);
    if (rc) return rc;
    if ((rc = map_ensure_out(mp, n_points))) return rc;
    HIP_TRY(hipMemcpyAsync(mp->d_head, blob, (size_t)map_state_bytes(n_cells, 0), hipMemcpyHostToDevice, mp->stream));
    if (n_points > 0)
      HIP_TRY(hipMemcpyAsync(mp->d_out, blob + map_state_bytes(n_cells, 0), sizeof(float4) * (size_t)n_points, hipMemcpyHostToDevice, mp->stream));
  }
  {
    MapStateTimer tm(mp->stream, hd ? "liodom_map_import_state" : "liodom_map_reset");
    const int n_init = std::max(m.ctable, m.max_cells);
    hipLaunchKernelGGL(k_map_init, dim3((n_init + 255) / 256), dim3(256), 0, mp->stream, m);
    if (n_cells > 0) {
      const int xb = std::min(16, (m.cell_cap + 255) / 256), yb = std::min(n_cells, 256);
      hipLaunchKernelGGL(k_map_unpack, dim3(xb, yb), dim3(256), 0, mp->stream, m, mp->d_head, mp->d_out, n_cells, n_points, (int)hd->status);
    } else if (hd && hd->status) {
      HIP_TRY(hipMemcpyAsync(&m.st->status, &hd->status, sizeof(int), hipMemcpyHostToDevice, mp->stream));
    }
    tm.stop();
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(mp->stream));      // the caller's blob must not be read after the call returns
  return LIODOM_OK;
}

// ---- relocalising (kernels_reloc.h) ----
// The occupancy buffer with a row for each of n_cells cells.
int map_ensure_occ(liodom_map* mp, int n_cells) {
  if (mp->d_occ && mp->occ_cells >= n_cells) return LIODOM_OK;
  HIP_TRY(hipStreamSynchronize(mp->stream));
  if (mp->d_occ) { (void)hipFree(mp->d_occ); mp->d_occ = nullptr; mp->occ_cells = 0; }
  mp->occ_gen = 0;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mp->d_occ), sizeof(unsigned int) * std::max<size_t>((size_t)n_cells * (size_t)mp->m.words, 4)));
  mp->occ_cells = n_cells;
  return LIODOM_OK;
}

int map_score_check(const liodom_map* mp, const float* edges, int n_edges, const char* who) {
  if (!mp || n_edges < 0 || (n_edges > 0 && !edges)) { g_last_error = std::string(who) + ": null map or edges, or a negative count"; return LIODOM_ERR_INVALID_ARG; }
  if (n_edges > mp->cfg.max_update_points) { g_last_error = std::string(who) + ": more edges than the map's max_update_points"; return LIODOM_ERR_INVALID_ARG; }
  return LIODOM_OK;
}

// Occupancy of the map as it is now, the two counts of each of the n >= 1 candidates T (host memory) and — with `best` — the best
// candidate {index, hits_r, hits_0, n}, on the map's current stream; synchronises.  The arguments have been validated.
// LIODOM_MAP_STATE_TIMING=1 reports the three parts' kernel times (tools/relocalize_cost.py reads them).
int map_score(liodom_map* mp, const float* edges, int n_edges, const double* T, int n, int radius, int32_t* hits, int32_t* best) {
  using namespace liodom_dev;
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  const MapView& m = mp->m;
  const int n_cells = std::max(0, std::min(st.n_cells, m.max_cells));
  const size_t t_bytes = sizeof(double) * 12 * (size_t)n, h_bytes = sizeof(int) * 2 * (size_t)n;
  int rc = map_ensure_occ(mp, n_cells);
  if (rc || (rc = map_ensure_batch(mp, t_bytes + h_bytes + sizeof(int) * 4))) return rc;
  double* d_T = reinterpret_cast<double*>(mp->d_batch);
  int* d_best = reinterpret_cast<int*>(mp->d_batch + t_bytes);      // the best candidate's record (16 bytes, 16-byte aligned), then
  int* d_hits = d_best + 4;                                         // the counts [n][2]
  if (n_edges > 0) HIP_TRY(hipMemcpyAsync(mp->d_in, edges, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_T, T, t_bytes, hipMemcpyHostToDevice, mp->stream));
  if (n_cells > 0) {
    MapStateTimer tm(mp->stream, "liodom_map_score_poses occupancy");
    const size_t n16 = ((size_t)n_cells * (size_t)m.words + 3) / 4;
    hipLaunchKernelGGL(k_map_occ_clear, dim3((unsigned)std::min<size_t>(2048, (n16 + 255) / 256)), dim3(256), 0, mp->stream, m, mp->d_occ, mp->occ_cells);
    hipLaunchKernelGGL(k_map_occ_build, dim3(std::min(16, (m.cell_cap + 255) / 256), std::min(n_cells, 256)), dim3(256), 0, mp->stream, m, mp->d_occ, mp->occ_cells);
    tm.stop();
    mp->occ_gen = mp->gen;      // (what the step path's hit records would build: it need not build it again)
  }
  {
    MapStateTimer tm(mp->stream, "liodom_map_score_poses score");
    hipLaunchKernelGGL(k_map_score_poses, dim3((n + kRelocWaves - 1) / kRelocWaves), dim3(kRelocThreads), 0, mp->stream, m, mp->d_occ, mp->occ_cells, mp->d_in,
                       n_edges, d_T, n, radius, (float)mp->cfg.resolution, d_hits);
    tm.stop();
  }
  if (best) {
    MapStateTimer tm(mp->stream, "liodom_map_score_poses best");
    hipLaunchKernelGGL(k_map_score_best, dim3(1), dim3(kRelocBestThreads), 0, mp->stream, d_hits, n, d_best);
    tm.stop();
  }
  HIP_TRY(hipGetLastError());
  if (hits) HIP_TRY(hipMemcpyAsync(hits, d_hits, h_bytes, hipMemcpyDeviceToHost, mp->stream));
  if (best) HIP_TRY(hipMemcpyAsync(best, d_best, sizeof(int) * 4, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));      // (the staged edges and poses are the caller's memory)
  return LIODOM_OK;
}

// ---- relocalising over a wide window (kernels_reloc_bnb.h, reloc_bnb.h) ----
// The cells the map holds now and the points in them (the sum of cell_n); synchronises the map's stream.
int map_count_points(liodom_map* mp, int* n_cells, int64_t* n_points) {
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  liodom_dev::MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  *n_cells = std::max(0, std::min(st.n_cells, mp->m.max_cells));
  std::vector<int> cnt((size_t)*n_cells);
  if (*n_cells > 0) HIP_TRY(hipMemcpy(cnt.data(), mp->m.cell_n, sizeof(int) * (size_t)*n_cells, hipMemcpyDeviceToHost));
  *n_points = 0;
  for (int c : cnt) *n_points += std::max(0, std::min(c, mp->m.cell_cap));
  return LIODOM_OK;
}

// The leaf occupancy of the map as it is now, as map_score builds it (n_cells > 0), on the map's stream.
int map_build_occ(liodom_map* mp, int n_cells) {
  using namespace liodom_dev;
  const MapView& m = mp->m;
  int rc = map_ensure_occ(mp, n_cells);
  if (rc) return rc;
  const size_t n16 = ((size_t)n_cells * (size_t)m.words + 3) / 4;
  hipLaunchKernelGGL(k_map_occ_clear, dim3((unsigned)std::min<size_t>(2048, (n16 + 255) / 256)), dim3(256), 0, mp->stream, m, mp->d_occ, mp->occ_cells);
  hipLaunchKernelGGL(k_map_occ_build, dim3(std::min(16, (m.cell_cap + 255) / 256), std::min(n_cells, 256)), dim3(256), 0, mp->stream, m, mp->d_occ, mp->occ_cells);
  HIP_TRY(hipGetLastError());
  mp->occ_gen = mp->gen;
  return LIODOM_OK;
}

// ---- per-scan hit records (kernels_map_hits.h) ----
// The kept occupancy: d_occ with a row for each of max_cells cells, so that no step ever has to regrow it (a synchronising
// re-allocation); called when a stream that reads the map has its hits switched on, never from a step.
int map_keep_occ(liodom_map* mp) { return map_ensure_occ(mp, mp->m.max_cells); }

// The occupancy of the map as it is now on `q`, without asking the device how many cells it holds (the two kernels clamp to
// n_cells themselves): enqueued only if a cell may have changed since d_occ was last built.  map_keep_occ has run.
// LIODOM_MAP_STATE_TIMING=1 reports each build on stderr, so a build can be counted.
int map_refresh_occ(liodom_map* mp, hipStream_t q) {
  using namespace liodom_dev;
  if (mp->occ_cells < mp->m.max_cells) { const int rc = map_keep_occ(mp); if (rc) return rc; }      // (never on the documented paths)
  if (mp->occ_gen == mp->gen) return LIODOM_OK;
  const MapView& m = mp->m;
  const size_t n16 = ((size_t)mp->occ_cells * (size_t)m.words + 3) / 4;
  MapStateTimer tm(q, "liodom map_hits occupancy");
  hipLaunchKernelGGL(k_map_occ_clear, dim3((unsigned)std::min<size_t>(2048, (n16 + 255) / 256)), dim3(256), 0, q, m, mp->d_occ, mp->occ_cells);
  hipLaunchKernelGGL(k_map_occ_build, dim3(std::min(16, (m.cell_cap + 255) / 256), std::min(mp->occ_cells, 256)), dim3(256), 0, q, m, mp->d_occ, mp->occ_cells);
  tm.stop();
  HIP_TRY(hipGetLastError());
  mp->occ_gen = mp->gen;
  return LIODOM_OK;
}

// The block tables of the levels whose bit is set in `levels`, built from the map as it is now, on the map's stream: each a power
// of two >= 2 * n_points (and >= 64) entries, zeroed and filled by this call.
int map_build_blocks(liodom_map* mp, unsigned int levels, int n_cells, int64_t n_points, liodom_dev::BlockTables* bt) {
  using namespace liodom_dev;
  size_t entries = 64;
  while ((int64_t)entries < 2 * n_points) entries <<= 1;
  int n_levels = 0;
  for (int h = 0; h <= kRelocBnbLevelMax; h++) bt->slot[h] = (h >= 1 && ((levels >> h) & 1u)) ? n_levels++ : -1;
  const size_t total = entries * (size_t)std::max(n_levels, 1);
  if (mp->blocks_entries < total) {
    HIP_TRY(hipStreamSynchronize(mp->stream));
    if (mp->d_blocks) { (void)hipFree(mp->d_blocks); mp->d_blocks = nullptr; mp->blocks_entries = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mp->d_blocks), sizeof(unsigned long long) * total));
    mp->blocks_entries = total;
  }
  bt->base = mp->d_blocks;
  bt->mask = (unsigned int)(entries - 1);
  hipLaunchKernelGGL(k_map_blocks_clear, dim3((unsigned)std::min<size_t>(2048, (total / 2 + 255) / 256)), dim3(256), 0, mp->stream, mp->d_blocks, total);
  if (n_cells > 0 && n_levels > 0)
    hipLaunchKernelGGL(k_map_blocks_build, dim3(std::min(16, (mp->m.cell_cap + 255) / 256), std::min(n_cells, 256)), dim3(256), 0, mp->stream, mp->m, *bt);
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

// LIODOM_MAP_STATE_TIMING=1: liodom_map_search_pose_bnb reports where its time went (tools/relocalize_bnb_cost.py reads the line).
// A host clock around work that ends in a synchronise of the map's stream.
struct MapBnbClock {
  bool on;
  double build = 0.0, bound = 0.0, exact = 0.0;
  std::chrono::steady_clock::time_point t0;
  MapBnbClock() { const char* e = std::getenv("LIODOM_MAP_STATE_TIMING"); on = e && e[0] == '1'; t0 = std::chrono::steady_clock::now(); }
  double ms_since(std::chrono::steady_clock::time_point a) const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); }
};

}  // namespace

extern "C" {

void liodom_map_config_default(liodom_map_config_t* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->device = 0;
  c->max_cells = 1024;
  c->voxel_xysize = 40.0; c->voxel_zsize = 50.0; c->resolution = 0.4;     // liodom_mapping_node.cc:115-125
  c->cell_capacity = 65536;
  c->max_update_points = 16384;
  c->max_modified_cells = 128;
}

int liodom_map_create(const liodom_map_config_t* config, liodom_map_t** out) {
  if (!config || !out) { g_last_error = "liodom_map_create: null argument"; return LIODOM_ERR_INVALID_ARG; }
  *out = nullptr;
  if (!(config->voxel_xysize > 0) || !(config->voxel_zsize > 0) || !(config->resolution > 0) || config->max_cells < 1 ||
      config->cell_capacity < 1 || config->max_update_points < 1 || config->max_modified_cells < 1 ||
      config->max_modified_cells > liodom_dev::kMapNewCellsMax) {
    g_last_error = "liodom_map_create: invalid configuration";
    return LIODOM_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "liodom_map_create: no HIP device available (this library has no CPU fallback)";
    return LIODOM_ERR_NO_DEVICE;
  }
  if (config->device < 0 || config->device >= ndev) { g_last_error = "liodom_map_create: device ordinal out of range"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(config->device));
  liodom_map* mp = new liodom_map();
  mp->device = config->device;
  int rc = map_build(mp, config, nullptr);
  if (rc == LIODOM_OK) {
    void* raw = nullptr;
    rc = map_alloc(mp, &raw, sizeof(float4) * (size_t)config->max_update_points);
    mp->d_in = reinterpret_cast<float4*>(raw);
    if (rc == LIODOM_OK) { rc = map_alloc(mp, &raw, sizeof(int) * 4); mp->d_n = reinterpret_cast<int*>(raw); mp->d_out_n = mp->d_n + 1; }
    if (rc == LIODOM_OK) { rc = map_alloc(mp, &raw, sizeof(double) * 12); mp->d_T = reinterpret_cast<double*>(raw); }
  }
  if (rc == LIODOM_OK && hipStreamSynchronize(mp->stream) != hipSuccess) { g_last_error = "liodom_map_create: initialisation failed"; rc = LIODOM_ERR_HIP; }
  if (rc != LIODOM_OK) { map_free(mp); return rc; }
  *out = mp;
  return LIODOM_OK;
}

void liodom_map_destroy(liodom_map_t* m) { map_free(m); }

int liodom_map_update(liodom_map_t* mp, const float* xyzi, int64_t n, const double* T) {
  if (!mp || !T || (n > 0 && !xyzi) || n < 0) { g_last_error = "liodom_map_update: invalid argument"; return LIODOM_ERR_INVALID_ARG; }
  if (n > mp->cfg.max_update_points) { g_last_error = "liodom_map_update: more points than max_update_points"; return LIODOM_ERR_CAPACITY; }
  HIP_TRY(hipSetDevice(mp->device));
  const int ni = (int)n;
  if (n) HIP_TRY(hipMemcpyAsync(mp->d_in, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(mp->d_n, &ni, sizeof(int), hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(mp->d_T, T, sizeof(double) * 12, hipMemcpyHostToDevice, mp->stream));
  int rc = map_enqueue_update(mp, mp->d_in, mp->d_n, mp->d_T, mp->stream);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(mp->stream));      // the staged host values must not be overwritten early
  return LIODOM_OK;
}

int liodom_map_get_local(liodom_map_t* mp, const double* T, int cells_xy, int cells_z, float* xyzi, int64_t cap,
                         int64_t* n_points) {
  if (!mp || !T || cap < 0 || (cap > 0 && !xyzi)) { g_last_error = "liodom_map_get_local: invalid argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  int rc = map_ensure_out(mp, cap);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(mp->d_T, T, sizeof(double) * 12, hipMemcpyHostToDevice, mp->stream));
  rc = map_enqueue_local(mp, mp->d_T, cells_xy, cells_z, mp->d_out, mp->out_cap, mp->d_out_n, mp->stream, 0);
  if (rc) return rc;
  return map_fetch_result(mp, xyzi, cap, n_points);
}

int liodom_map_get_local_batch(liodom_map_t* mp, const double* T, int n, int cells_xy, int cells_z, float* xyzi, int64_t cap_per_row,
                               int64_t* n_points) {
  using namespace liodom_dev;
  if (!mp || n < 0 || (n > 0 && (!T || !n_points)) || cap_per_row < 0 || (cap_per_row > 0 && n > 0 && !xyzi) || cells_xy < 0 || cells_z < 0) {
    g_last_error = "liodom_map_get_local_batch: invalid argument"; return LIODOM_ERR_INVALID_ARG;
  }
  if (n == 0) return LIODOM_OK;
  if (cap_per_row > 0x7fffffff || (int64_t)n * std::max<int64_t>(cap_per_row, 1) > 0x7fffffff) {
    g_last_error = "liodom_map_get_local_batch: n * cap_per_row beyond 2^31 - 1 points"; return LIODOM_ERR_CAPACITY;
  }
  HIP_TRY(hipSetDevice(mp->device));
  const int cap = (int)cap_per_row;
  int rc = map_ensure_out(mp, (int64_t)n * std::max(cap, 1));
  if (rc) return rc;
  const size_t t_bytes = sizeof(double) * 12 * (size_t)n;
  if ((rc = map_ensure_batch(mp, t_bytes + sizeof(int) * 2 * (size_t)n))) return rc;
  double* d_T = reinterpret_cast<double*>(mp->d_batch);
  int* d_n = reinterpret_cast<int*>(mp->d_batch + t_bytes);      // [n] points written, [n] sizes
  HIP_TRY(hipMemcpyAsync(d_T, T, t_bytes, hipMemcpyHostToDevice, mp->stream));
  if (map_rows_fit(mp, cells_xy, cells_z)) {
    MapRows r{};
    r.T = d_T; r.T_stride = 12; r.out = mp->d_out; r.out_stride = cap; r.n_out = d_n; r.n_stride = 1; r.total = d_n + n;
    r.sel = nullptr; r.list = nullptr; r.tag = 0; r.s0 = 0; r.cap = cap; r.cells_xy = cells_xy; r.cells_z = cells_z; r.sticky = 0;
    // (rows beyond the grid's y limit: launches of 32768 rows)
    for (int first = 0; first < n; first += 32768) {
      const int rows = std::min(32768, n - first);
      r.s0 = first;
      hipLaunchKernelGGL(k_map_local_rows<false>, dim3(map_rows_grid_x(rows, cap), rows), dim3(kMapRowsThreads), 0, mp->stream, mp->m, r);
    }
    HIP_TRY(hipGetLastError());
  } else {
    // a visit the LDS plan cannot hold: the two launches of liodom_map_get_local, row after row (one plan scratch: stream order)
    for (int i = 0; i < n; i++) {
      rc = map_enqueue_local(mp, d_T + 12 * (size_t)i, cells_xy, cells_z, mp->d_out + (size_t)i * cap, cap, d_n + i, mp->stream, 0);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(d_n + n + i, &mp->m.st->n_result, sizeof(int), hipMemcpyDeviceToDevice, mp->stream));
    }
  }
  std::vector<int> cnt(2 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_n, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));      // (the staged poses are the caller's memory)
  bool fits = true;
  for (int i = 0; i < n; i++) { n_points[i] = cnt[(size_t)n + i]; fits = fits && cnt[(size_t)n + i] <= cap; }
  if (!fits) { g_last_error = "liodom_map_get_local_batch: a row is larger than cap_per_row"; return LIODOM_ERR_CAPACITY; }
  for (int i = 0; i < n; i++)
    if (cnt[(size_t)i] > 0) HIP_TRY(hipMemcpy(xyzi + 4 * (size_t)i * (size_t)cap, mp->d_out + (size_t)i * cap, sizeof(float4) * (size_t)cnt[(size_t)i], hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

// Map::getMap (map.cc:131-139): every cell in cells_vector_ order — a blob's point section.  Planned and copied by the export's
// kernels, which hold any number of cells (the plan entries of getLocalMap hold kMapLocalEntriesMax).
int liodom_map_get_all(liodom_map_t* mp, float* xyzi, int64_t cap, int64_t* n_points) {
  using namespace liodom_dev;
  if (!mp || cap < 0 || (cap > 0 && !xyzi)) { g_last_error = "liodom_map_get_all: invalid argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  MapStateHeader hd;
  int rc = map_state_plan(mp, &hd, "liodom_map_get_all");      // (synchronises the stream the map's work is enqueued on)
  if (rc) return rc;
  if (n_points) *n_points = hd.n_points;
  if (hd.n_points > cap) { g_last_error = "liodom_map: output buffer too small"; return LIODOM_ERR_CAPACITY; }
  const int n = (int)hd.n_points;
  if (n == 0) return LIODOM_OK;
  if ((rc = map_ensure_out(mp, n))) return rc;
  const int xb = std::min(16, (mp->m.cell_cap + 255) / 256), yb = std::min(hd.n_cells, 256);
  hipLaunchKernelGGL(k_map_pack, dim3(xb, yb), dim3(256), 0, mp->stream, mp->m, mp->d_head, mp->d_out, mp->out_cap);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(xyzi, mp->d_out, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  return LIODOM_OK;
}

int liodom_map_num_cells(liodom_map_t* mp, int* n_cells) {
  if (!mp || !n_cells) { g_last_error = "liodom_map_num_cells: null argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  liodom_dev::MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  *n_cells = st.n_cells;
  return LIODOM_OK;
}

int liodom_map_status(liodom_map_t* mp, uint32_t* status) {
  if (!mp || !status) { g_last_error = "liodom_map_status: null argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  liodom_dev::MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  *status = (uint32_t)st.status;
  return LIODOM_OK;
}

int liodom_map_state_size(liodom_map_t* mp, int64_t* bytes) {
  if (!mp || !bytes) { g_last_error = "liodom_map_state_size: null argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  liodom_dev::MapStateHeader hd;
  int rc = map_state_plan(mp, &hd, "liodom_map_state_size");
  if (rc) return rc;
  *bytes = liodom_dev::map_state_bytes(hd.n_cells, hd.n_points);
  return LIODOM_OK;
}

int liodom_map_export_state(liodom_map_t* mp, void* blob, int64_t cap, int64_t* bytes) {
  using namespace liodom_dev;
  if (!mp || !bytes || cap < 0 || (cap > 0 && !blob)) { g_last_error = "liodom_map_export_state: invalid argument"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  MapStateHeader hd;
  MapStateTimer tm(mp->stream, "liodom_map_export_state");
  int rc = map_state_plan(mp, &hd, "liodom_map_export_state");      // (synchronises the stream the map's work is enqueued on)
  if (rc) return rc;
  const int64_t need = map_state_bytes(hd.n_cells, hd.n_points);
  *bytes = need;
  if (need > cap) { g_last_error = "liodom_map_export_state: blob buffer too small"; return LIODOM_ERR_CAPACITY; }
  unsigned char* out = static_cast<unsigned char*>(blob);
  const int n_points = (int)hd.n_points;
  if (n_points > 0) {
    if ((rc = map_ensure_out(mp, n_points))) return rc;
    const int xb = std::min(16, (mp->m.cell_cap + 255) / 256), yb = std::min(hd.n_cells, 256);
    hipLaunchKernelGGL(k_map_pack, dim3(xb, yb), dim3(256), 0, mp->stream, mp->m, mp->d_head, mp->d_out, mp->out_cap);
    HIP_TRY(hipGetLastError());
  }
  tm.stop();
  if (hd.n_cells > 0)
    HIP_TRY(hipMemcpyAsync(out + kMapStateHeaderBytes, mp->d_head + kMapStateHeaderBytes, (size_t)kMapStateRecordBytes * (size_t)hd.n_cells,
                           hipMemcpyDeviceToHost, mp->stream));
  if (n_points > 0)
    HIP_TRY(hipMemcpyAsync(out + map_state_bytes(hd.n_cells, 0), mp->d_out, sizeof(float4) * (size_t)n_points, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  // the header is the host's
  std::memset(hd.magic, 0, sizeof(hd.magic));
  std::memcpy(hd.magic, "LIODOMMP", 8);
  hd.version = kMapStateVersion; hd.header_bytes = (uint32_t)kMapStateHeaderBytes; hd.total_bytes = (uint64_t)need;
  hd.voxel_xysize = mp->cfg.voxel_xysize; hd.voxel_zsize = mp->cfg.voxel_zsize; hd.resolution = mp->cfg.resolution;
  std::memcpy(out, &hd, sizeof(hd));
  return LIODOM_OK;
}

int liodom_map_import_state(liodom_map_t* mp, const void* blob, int64_t bytes) {
  if (!mp || !blob) { g_last_error = "liodom_map_import_state: null argument"; return LIODOM_ERR_INVALID_ARG; }
  if (!mp->own_stream) { g_last_error = "liodom_map_import_state: the map is attached to a handle: detach it (liodom_attach_mapper with NULL), import, attach"; return LIODOM_ERR_BUSY; }
  // every rejection comes before anything is launched
  const char* why = "";
  int rc = liodom_dev::map_state_validate(blob, bytes, mp->cfg.voxel_xysize, mp->cfg.voxel_zsize, mp->cfg.resolution, mp->m.max_cells,
                                          mp->m.cell_cap, &why);
  if (rc) { g_last_error = std::string("liodom_map_import_state: ") + why; return rc; }
  liodom_dev::MapStateHeader hd;
  std::memcpy(&hd, blob, sizeof(hd));
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  return map_install_state(mp, static_cast<const unsigned char*>(blob), &hd);
}

int liodom_map_prune(liodom_map_t* mp, const double* T, int keep_cells_xy, int keep_cells_z, int* n_removed) {
  if (!mp || !T || keep_cells_xy < 0 || keep_cells_z < 0) { g_last_error = "liodom_map_prune: null map or pose, or a negative keep extent"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(mp->device));
  int rc = map_ensure_prune(mp);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(mp->d_T, T, sizeof(double) * 12, hipMemcpyHostToDevice, mp->stream));
  if ((rc = map_enqueue_prune(mp, mp->d_T, keep_cells_xy, keep_cells_z, mp->stream))) return rc;
  liodom_dev::MapPruneMove info{};
  HIP_TRY(hipMemcpyAsync(&info, mp->d_prune + mp->m.max_cells, sizeof(info), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));      // (the staged pose and `info` are this frame's)
  if (n_removed) *n_removed = info.src;
  return LIODOM_OK;
}

int liodom_map_evict(liodom_map_t* mp, const double* T, int keep_cells_xy, int keep_cells_z, void* blob, int64_t cap, int64_t* bytes,
                     int* n_evicted) {
  using namespace liodom_dev;
  if (!mp || !T || !bytes || keep_cells_xy < 0 || keep_cells_z < 0 || cap < 0 || (cap > 0 && !blob)) {
    g_last_error = "liodom_map_evict: null map, pose or bytes, a negative keep extent, or a capacity without a buffer"; return LIODOM_ERR_INVALID_ARG;
  }
  HIP_TRY(hipSetDevice(mp->device));
  // everything that can fail comes before the map is touched: the plan is read-only, and it gives the size
  int rc = map_ensure_head(mp);
  if (rc || (rc = map_ensure_prune(mp))) return rc;
  const MapView& m = mp->m;
  int* d_src = reinterpret_cast<int*>(mp->d_prune);
  MapStateHeader hd;
  MapStateTimer tm(mp->stream, "liodom_map_evict");
  HIP_TRY(hipMemcpyAsync(mp->d_T, T, sizeof(double) * 12, hipMemcpyHostToDevice, mp->stream));
  hipLaunchKernelGGL(k_map_evict_plan, dim3(1), dim3(1024), 0, mp->stream, m, mp->d_T, keep_cells_xy, keep_cells_z, mp->d_head, d_src);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(&hd, mp->d_head, sizeof(hd), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  if (hd.n_cells < 0 || hd.n_cells > m.max_cells || hd.n_points < 0 || hd.n_points > (int64_t)hd.n_cells * m.cell_cap) {
    g_last_error = "liodom_map_evict: inconsistent map state"; return LIODOM_ERR_HIP;
  }
  if (hd.n_points > 0x7fffffff) { g_last_error = "liodom_map_evict: more than 2^31 - 1 points do not fit the blob format"; return LIODOM_ERR_CAPACITY; }
  const int64_t need = map_state_bytes(hd.n_cells, hd.n_points);
  *bytes = need;
  if (need > cap) { g_last_error = "liodom_map_evict: blob buffer too small"; return LIODOM_ERR_CAPACITY; }
  unsigned char* out = static_cast<unsigned char*>(blob);
  const int n_points = (int)hd.n_points;
  if (n_points > 0 && (rc = map_ensure_out(mp, n_points))) return rc;
  if (n_points > 0) {
    const int xb = std::min(16, (m.cell_cap + 255) / 256), yb = std::min(hd.n_cells, 256);
    hipLaunchKernelGGL(k_map_evict_pack, dim3(xb, yb), dim3(256), 0, mp->stream, m, mp->d_head, d_src, mp->d_out, mp->out_cap);
  }
  if ((rc = map_enqueue_prune(mp, mp->d_T, keep_cells_xy, keep_cells_z, mp->stream))) return rc;
  tm.stop();
  if (hd.n_cells > 0)
    HIP_TRY(hipMemcpyAsync(out + kMapStateHeaderBytes, mp->d_head + kMapStateHeaderBytes, (size_t)kMapStateRecordBytes * (size_t)hd.n_cells,
                           hipMemcpyDeviceToHost, mp->stream));
  if (n_points > 0)
    HIP_TRY(hipMemcpyAsync(out + map_state_bytes(hd.n_cells, 0), mp->d_out, sizeof(float4) * (size_t)n_points, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  // the header is the host's
  std::memset(hd.magic, 0, sizeof(hd.magic));
  std::memcpy(hd.magic, "LIODOMMP", 8);
  hd.version = kMapStateVersion; hd.header_bytes = (uint32_t)kMapStateHeaderBytes; hd.total_bytes = (uint64_t)need;
  hd.voxel_xysize = mp->cfg.voxel_xysize; hd.voxel_zsize = mp->cfg.voxel_zsize; hd.resolution = mp->cfg.resolution;
  hd.status = 0u;
  std::memcpy(out, &hd, sizeof(hd));
  if (n_evicted) *n_evicted = hd.n_cells;
  return LIODOM_OK;
}

int liodom_map_merge_state(liodom_map_t* mp, const void* blob, int64_t bytes, int32_t* taken, int* n_added) {
  using namespace liodom_dev;
  if (!mp || !blob) { g_last_error = "liodom_map_merge_state: null argument"; return LIODOM_ERR_INVALID_ARG; }
  // every rejection comes before anything is launched
  const char* why = "";
  int rc = map_state_validate(blob, bytes, mp->cfg.voxel_xysize, mp->cfg.voxel_zsize, mp->cfg.resolution, mp->m.max_cells, mp->m.cell_cap, &why);
  if (rc) { g_last_error = std::string("liodom_map_merge_state: ") + why; return rc; }
  MapStateHeader hd;
  std::memcpy(&hd, blob, sizeof(hd));
  if (n_added) *n_added = 0;
  if (hd.n_cells == 0) return LIODOM_OK;
  if (hd.n_points > 0x7fffffff) { g_last_error = "liodom_map_merge_state: more than 2^31 - 1 points"; return LIODOM_ERR_CAPACITY; }
  HIP_TRY(hipSetDevice(mp->device));
  const MapView& m = mp->m;
  const unsigned char* src = static_cast<const unsigned char*>(blob);
  const int n_cells = hd.n_cells, n_points = (int)hd.n_points;
  if ((rc = map_ensure_head(mp)) || (rc = map_ensure_prune(mp)) || (rc = map_ensure_out(mp, n_points))) return rc;
  MapMergeInfo* d_info = reinterpret_cast<MapMergeInfo*>(mp->d_prune);      // the prune scratch: 4 ints per max_cells + 1
  int* d_rank = reinterpret_cast<int*>(mp->d_prune) + 4;
  HIP_TRY(hipMemcpyAsync(mp->d_head, src, (size_t)map_state_bytes(n_cells, 0), hipMemcpyHostToDevice, mp->stream));
  if (n_points > 0)
    HIP_TRY(hipMemcpyAsync(mp->d_out, src + map_state_bytes(n_cells, 0), sizeof(float4) * (size_t)n_points, hipMemcpyHostToDevice, mp->stream));
  MapStateTimer tm(mp->stream, "liodom_map_merge_state");
  hipLaunchKernelGGL(k_map_merge_plan, dim3(1), dim3(1024), 0, mp->stream, m, mp->d_head, n_cells, d_info, d_rank);
  HIP_TRY(hipGetLastError());
  MapMergeInfo info{};
  std::vector<int> rank((size_t)n_cells);
  HIP_TRY(hipMemcpyAsync(&info, d_info, sizeof(info), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipMemcpyAsync(rank.data(), d_rank, sizeof(int) * (size_t)n_cells, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  if (info.n_taken < 0 || info.n_taken > n_cells || info.n_before < 0 || info.n_before > m.max_cells) {
    g_last_error = "liodom_map_merge_state: inconsistent map state"; return LIODOM_ERR_HIP;
  }
  if (info.n_before + info.n_taken > m.max_cells) {
    g_last_error = "liodom_map_merge_state: not enough free cells for the blob's cells (max_cells)"; return LIODOM_ERR_CAPACITY;
  }
  if (info.n_taken > 0 || hd.status) {
    mp->gen++;
    const int xb = std::min(16, (m.cell_cap + 255) / 256), yb = std::min(n_cells, 256);
    hipLaunchKernelGGL(k_map_merge, dim3(xb, yb), dim3(256), 0, mp->stream, m, mp->d_head, mp->d_out, n_cells, n_points, d_info, d_rank, (int)hd.status);
    HIP_TRY(hipGetLastError());
  }
  tm.stop();
  HIP_TRY(hipStreamSynchronize(mp->stream));      // the caller's blob must not be read after the call returns
  if (taken) for (int i = 0; i < n_cells; i++) taken[i] = rank[(size_t)i] >= 0 ? 1 : 0;
  if (n_added) *n_added = info.n_taken;
  return LIODOM_OK;
}

int liodom_map_score_poses(liodom_map_t* mp, const float* edges_xyzi, int n_edges, const double* T, int n, int radius, int32_t* hits) {
  int rc = map_score_check(mp, edges_xyzi, n_edges, "liodom_map_score_poses");
  if (rc) return rc;
  if (n < 0 || n > liodom_dev::kRelocCandidatesMax || (n > 0 && (!T || !hits)) || (radius != 0 && radius != 1)) {
    g_last_error = "liodom_map_score_poses: null poses or hits, a count that is negative or above 2^20, or a radius that is not 0 or 1"; return LIODOM_ERR_INVALID_ARG;
  }
  if (n == 0) return LIODOM_OK;
  return map_score(mp, edges_xyzi, n_edges, T, n, radius, hits, nullptr);
}

int liodom_map_hit_rows(liodom_map_t* mp, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges, const double* T, int n, int radius,
                        int32_t* hits) {
  using namespace liodom_dev;
  if (!mp || n < 0 || n > kRelocCandidatesMax || (n > 0 && (!n_edges || !T || !hits)) || (radius != 0 && radius != 1) || edge_stride_points < 0) {
    g_last_error = "liodom_map_hit_rows: null map, counts, poses or hits, a count that is negative or above 2^20, a negative stride, or a radius that is not 0 or 1";
    return LIODOM_ERR_INVALID_ARG;
  }
  if (edge_stride_points > mp->cfg.max_update_points) { g_last_error = "liodom_map_hit_rows: a row stride above the map's max_update_points"; return LIODOM_ERR_INVALID_ARG; }
  bool any = false;
  for (int i = 0; i < n; i++) {
    if (n_edges[i] < 0 || n_edges[i] > edge_stride_points) { g_last_error = "liodom_map_hit_rows: a row's edge count is negative or above the row stride"; return LIODOM_ERR_INVALID_ARG; }
    any = any || n_edges[i] > 0;
  }
  if (any && !edges_xyzi) { g_last_error = "liodom_map_hit_rows: null edges"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  if (!any) { std::memset(hits, 0, sizeof(int32_t) * 2 * (size_t)n); return LIODOM_OK; }
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  MapState st;
  HIP_TRY(hipMemcpy(&st, mp->m.st, sizeof(st), hipMemcpyDeviceToHost));
  const int n_cells = std::max(0, std::min(st.n_cells, mp->m.max_cells));
  // staging: the rows' clouds back to back at the caller's stride, then the poses, the edge counts and the counts
  const size_t e_bytes = sizeof(float4) * (size_t)n * (size_t)edge_stride_points, t_bytes = sizeof(double) * 12 * (size_t)n, c_bytes = sizeof(int) * (size_t)n;
  const size_t t_off = (e_bytes + 15) / 16 * 16, c_off = t_off + t_bytes, h_off = (c_off + c_bytes + 7) / 8 * 8;
  int rc = map_ensure_occ(mp, n_cells);
  if (rc || (rc = map_ensure_batch(mp, h_off + sizeof(int) * 2 * (size_t)n))) return rc;
  float4* d_edges = reinterpret_cast<float4*>(mp->d_batch);
  double* d_T = reinterpret_cast<double*>(mp->d_batch + t_off);
  int* d_cnt = reinterpret_cast<int*>(mp->d_batch + c_off);
  int* d_hits = reinterpret_cast<int*>(mp->d_batch + h_off);
  HIP_TRY(hipMemcpyAsync(d_edges, edges_xyzi, e_bytes, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_T, T, t_bytes, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_cnt, n_edges, c_bytes, hipMemcpyHostToDevice, mp->stream));
  if (n_cells > 0 && (rc = map_build_occ(mp, n_cells))) return rc;
  MapHitRows r{};
  r.edges = d_edges; r.edge_stride = edge_stride_points; r.n_edges = d_cnt; r.n_stride = 1; r.T = d_T; r.T_stride = 12;
  r.edge_cap = (int)edge_stride_points; r.radius = radius; r.hits = d_hits;
  hipLaunchKernelGGL(k_map_hit_rows<false>, dim3((unsigned)n), dim3(kMapHitThreads), 0, mp->stream, mp->m, mp->d_occ, mp->occ_cells, (float)mp->cfg.resolution, r);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(hits, d_hits, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));      // (the staged clouds, poses and counts are the caller's memory)
  return LIODOM_OK;
}

void liodom_pose_search_default(liodom_pose_search_t* s) {
  if (!s) return;
  std::memset(s, 0, sizeof(*s));
  s->centre[3] = 1.0;
  s->step_xy = 0.4; s->step_z = 0.4; s->step_yaw = 0.02;
  s->radius = 1;
}

int liodom_map_search_pose(liodom_map_t* mp, const float* edges_xyzi, int n_edges, const liodom_pose_search_t* s, liodom_pose_search_result_t* out,
                           double* T_out, int32_t* hits_out) {
  int rc = map_score_check(mp, edges_xyzi, n_edges, "liodom_map_search_pose");
  if (rc) return rc;
  if (!s || !out) { g_last_error = "liodom_map_search_pose: null search or result"; return LIODOM_ERR_INVALID_ARG; }
  const char* why = "";
  const int64_t n = liodom_dev::reloc_candidate_count(s, &why);
  if (n <= 0) { g_last_error = std::string("liodom_map_search_pose: ") + why; return LIODOM_ERR_INVALID_ARG; }
  std::vector<double> T(12 * (size_t)n);
  liodom_dev::reloc_candidates(s, n, T.data());
  int32_t best[4] = {0, 0, 0, 0};
  if ((rc = map_score(mp, edges_xyzi, n_edges, T.data(), (int)n, s->radius, hits_out, best))) return rc;
  if (best[0] < 0 || best[0] >= n) { g_last_error = "liodom_map_search_pose: inconsistent result"; return LIODOM_ERR_HIP; }
  out->best_index = best[0]; out->hits_r = best[1]; out->hits_0 = best[2]; out->n_candidates = (int32_t)n;
  liodom_dev::reloc_candidate_pose(s, best[0], out->pose);
  std::memcpy(out->T, &T[12 * (size_t)best[0]], sizeof(double) * 12);
  if (T_out) std::memcpy(T_out, T.data(), sizeof(double) * 12 * (size_t)n);
  return LIODOM_OK;
}

void liodom_pose_search_bnb_default(liodom_pose_search_bnb_t* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->batch = liodom_dev::kRelocBnbBatchDefault;
}

int liodom_map_bound_nodes(liodom_map_t* mp, const float* edges_xyzi, int n_edges, const double* T_lo, const double* t_hi, int n, int level, int radius,
                           int32_t* ub) {
  using namespace liodom_dev;
  int rc = map_score_check(mp, edges_xyzi, n_edges, "liodom_map_bound_nodes");
  if (rc) return rc;
  if (n < 0 || n > kRelocCandidatesMax || (n > 0 && (!T_lo || !t_hi || !ub)) || (radius != 0 && radius != 1) || level < 1 || level > kRelocBnbLevelMax) {
    g_last_error = "liodom_map_bound_nodes: null nodes or bounds, a count that is negative or above 2^20, a level outside 1 .. 21, or a radius that is not 0 or 1";
    return LIODOM_ERR_INVALID_ARG;
  }
  if (n == 0) return LIODOM_OK;
  int n_cells = 0;
  int64_t n_points = 0;
  if ((rc = map_count_points(mp, &n_cells, &n_points))) return rc;
  const size_t lo_bytes = sizeof(double) * 12 * (size_t)n, hi_bytes = sizeof(double) * 2 * (size_t)n, ub_bytes = sizeof(int) * 2 * (size_t)n;
  if ((rc = map_ensure_batch(mp, lo_bytes + hi_bytes + ub_bytes))) return rc;
  double* d_lo = reinterpret_cast<double*>(mp->d_batch);
  double* d_hi = reinterpret_cast<double*>(mp->d_batch + lo_bytes);
  int* d_ub = reinterpret_cast<int*>(mp->d_batch + lo_bytes + hi_bytes);
  BlockTables bt;
  if ((rc = map_build_blocks(mp, 1u << level, n_cells, n_points, &bt))) return rc;
  if (n_edges > 0) HIP_TRY(hipMemcpyAsync(mp->d_in, edges_xyzi, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_lo, T_lo, lo_bytes, hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_hi, t_hi, hi_bytes, hipMemcpyHostToDevice, mp->stream));
  hipLaunchKernelGGL(k_map_bound_nodes, dim3((n + kRelocWaves - 1) / kRelocWaves), dim3(kRelocThreads), 0, mp->stream, mp->m, bt, mp->d_in, n_edges, d_lo, d_hi,
                     (const int*)nullptr, level, n, radius, (float)mp->cfg.resolution, d_ub);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(ub, d_ub, ub_bytes, hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  return LIODOM_OK;
}

int liodom_map_search_pose_bnb(liodom_map_t* mp, const float* edges_xyzi, int n_edges, const liodom_pose_search_t* s, const liodom_pose_search_bnb_t* opt,
                               liodom_pose_search_result_t* out, liodom_pose_search_stats_t* stats) {
  using namespace liodom_dev;
  int rc = map_score_check(mp, edges_xyzi, n_edges, "liodom_map_search_pose_bnb");
  if (rc) return rc;
  if (!s || !out) { g_last_error = "liodom_map_search_pose_bnb: null search or result"; return LIODOM_ERR_INVALID_ARG; }
  int batch = opt ? opt->batch : 0;
  if (batch == 0) batch = kRelocBnbBatchDefault;
  if (batch < 1 || batch > kRelocBnbBatchMax) { g_last_error = "liodom_map_search_pose_bnb: batch outside 1 .. 65536"; return LIODOM_ERR_INVALID_ARG; }
  const char* why = "";
  const int64_t n = reloc_candidate_count(s, &why, kRelocBnbCandidatesMax);
  if (n <= 0) { g_last_error = std::string("liodom_map_search_pose_bnb: ") + why; return LIODOM_ERR_INVALID_ARG; }
  MapBnbClock clk;
  const RelocCentre centre = reloc_centre(s);
  const RelocBnbGrid grid = reloc_bnb_grid(s);
  int n_cells = 0;
  int64_t n_points = 0;
  if ((rc = map_count_points(mp, &n_cells, &n_points))) return rc;
  RelocBnbResult res{0, 0, 0, 0, 0, 0};
  int levels_built = 0;
  if (n_edges > 0 && n_points > 0) {      // (otherwise every candidate scores 0: the lowest index wins)
    const MapView& m = mp->m;
    // One round's staging, the same layout in pinned host memory and in the batch buffer: the nodes to bound ([cnt x 12] T_lo,
    // [cnt x 2] t_hi, [cnt] levels: one upload), their bounds, the candidates to score ([cnt x 12] T) and their counts.
    const size_t nb = (size_t)batch, nk = 4 * nb;      // candidates scored, nodes bounded in one round at the most
    const size_t node_bytes = sizeof(double) * 14 + sizeof(int);
    const size_t off_ub = (nk * node_bytes + 15) / 16 * 16, off_T = off_ub + sizeof(int) * 2 * nk, off_hits = off_T + sizeof(double) * 12 * nb;
    const size_t stage_bytes = off_hits + sizeof(int) * 2 * nb;
    if ((rc = map_ensure_batch(mp, stage_bytes))) return rc;
    if (mp->pin_bytes < stage_bytes) {
      if (mp->h_pin) { (void)hipHostFree(mp->h_pin); mp->h_pin = nullptr; mp->pin_bytes = 0; }
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&mp->h_pin), stage_bytes, hipHostMallocDefault));
      mp->pin_bytes = stage_bytes;
    }
    unsigned char* hp = mp->h_pin;
    unsigned char* dp = mp->d_batch;
    // the level of a node 2^k wide, and the tables of the levels the tree has (a root is never bounded: k < K)
    int level_of_k[32];
    unsigned int levels = 0;
    for (int k = 0; k < grid.K; k++) { level_of_k[k] = reloc_bnb_level((int64_t)1 << k, s->step_xy, mp->cfg.resolution, s->radius); levels |= 1u << level_of_k[k]; }
    for (int h = 1; h <= kRelocBnbLevelMax; h++) levels_built += (int)((levels >> h) & 1u);
    const auto t_build = std::chrono::steady_clock::now();
    BlockTables bt;
    if ((rc = map_build_occ(mp, n_cells)) || (rc = map_build_blocks(mp, levels, n_cells, n_points, &bt))) return rc;
    HIP_TRY(hipMemcpyAsync(mp->d_in, edges_xyzi, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, mp->stream));
    if (clk.on) { HIP_TRY(hipStreamSynchronize(mp->stream)); clk.build = clk.ms_since(t_build); }
    const float leaf = (float)mp->cfg.resolution;
    auto bound_fn = [&](const RelocBnbNode* nodes, size_t cnt, int32_t* ub) -> int {
      const auto t = std::chrono::steady_clock::now();
      const size_t hi_at = sizeof(double) * 12 * cnt, lv_at = sizeof(double) * 14 * cnt;
      double* h_lo = reinterpret_cast<double*>(hp);
      double* h_hi = reinterpret_cast<double*>(hp + hi_at);
      int* h_lv = reinterpret_cast<int*>(hp + lv_at);
      for (size_t i = 0; i < cnt; i++) {
        reloc_bnb_extremes(s, centre, grid, nodes[i], h_lo + 12 * i, h_hi + 2 * i);
        h_lv[i] = level_of_k[nodes[i].k];
      }
      HIP_TRY(hipMemcpyAsync(dp, hp, node_bytes * cnt, hipMemcpyHostToDevice, mp->stream));
      hipLaunchKernelGGL(k_map_bound_nodes, dim3((unsigned)((cnt + kRelocWaves - 1) / kRelocWaves)), dim3(kRelocThreads), 0, mp->stream, m, bt, mp->d_in, n_edges,
                         reinterpret_cast<const double*>(dp), reinterpret_cast<const double*>(dp + hi_at), reinterpret_cast<const int*>(dp + lv_at), 0, (int)cnt,
                         s->radius, leaf, reinterpret_cast<int*>(dp + off_ub));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hp + off_ub, dp + off_ub, sizeof(int) * 2 * cnt, hipMemcpyDeviceToHost, mp->stream));
      HIP_TRY(hipStreamSynchronize(mp->stream));
      std::memcpy(ub, hp + off_ub, sizeof(int) * 2 * cnt);
      if (clk.on) clk.bound += clk.ms_since(t);
      return LIODOM_OK;
    };
    auto exact_fn = [&](const int64_t* index, size_t cnt, int32_t* hits) -> int {
      const auto t = std::chrono::steady_clock::now();
      double* h_T = reinterpret_cast<double*>(hp + off_T);
      for (size_t i = 0; i < cnt; i++) reloc_candidate_matrix(s, centre, index[i], h_T + 12 * i);
      HIP_TRY(hipMemcpyAsync(dp + off_T, h_T, sizeof(double) * 12 * cnt, hipMemcpyHostToDevice, mp->stream));
      hipLaunchKernelGGL(k_map_score_poses, dim3((unsigned)((cnt + kRelocWaves - 1) / kRelocWaves)), dim3(kRelocThreads), 0, mp->stream, m, mp->d_occ, mp->occ_cells,
                         mp->d_in, n_edges, reinterpret_cast<const double*>(dp + off_T), (int)cnt, s->radius, leaf, reinterpret_cast<int*>(dp + off_hits));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(hp + off_hits, dp + off_hits, sizeof(int) * 2 * cnt, hipMemcpyDeviceToHost, mp->stream));
      HIP_TRY(hipStreamSynchronize(mp->stream));
      std::memcpy(hits, hp + off_hits, sizeof(int) * 2 * cnt);
      if (clk.on) clk.exact += clk.ms_since(t);
      return LIODOM_OK;
    };
    const int32_t max_score = (int32_t)std::min<int64_t>(2 * (int64_t)n_edges, 0x7fffffff);
    if ((rc = reloc_bnb_search(grid, max_score, batch, bound_fn, exact_fn, &res))) return rc;
    if (res.best_index < 0 || res.best_index >= n) { g_last_error = "liodom_map_search_pose_bnb: inconsistent result"; return LIODOM_ERR_HIP; }
  }
  out->best_index = (int32_t)res.best_index; out->hits_r = res.hits_r; out->hits_0 = res.hits_0; out->n_candidates = (int32_t)n;
  reloc_candidate_pose(s, res.best_index, out->pose);
  reloc_candidate_matrix(s, centre, res.best_index, out->T);
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n_candidates = n; stats->nodes_bounded = res.nodes_bounded; stats->candidates_scored = res.candidates_scored;
    stats->rounds = (int32_t)std::min<int64_t>(res.rounds, 0x7fffffff); stats->levels_built = levels_built;
  }
  if (clk.on) {
    const double total = clk.ms_since(clk.t0);
    std::fprintf(stderr, "liodom_map_search_pose_bnb: build %.3f ms, bound %.3f ms, exact %.3f ms, host %.3f ms, total %.3f ms\n", clk.build, clk.bound,
                 clk.exact, total - clk.build - clk.bound - clk.exact, total);
  }
  return LIODOM_OK;
}

// ---- registering a scan to the map (kernels_register.h, map_register.h) ----
void liodom_map_register_default(liodom_map_register_t* o) {
  if (o) liodom_dev::map_register_default(o);
}

int liodom_map_register_poses(liodom_map_t* mp, const float* edges, int n_edges, const double* poses, int n, const liodom_map_register_t* opt,
                              liodom_map_registration_t* out, int32_t* corr) {
  using namespace liodom_dev;
  // every refusal comes before anything is allocated, staged or launched
  if (!mp || !poses || !out || (n_edges > 0 && !edges)) { g_last_error = "liodom_map_register_poses: null map, poses, out or edges"; return LIODOM_ERR_INVALID_ARG; }
  if (n < 1 || n > kRegisterRowsMax) { g_last_error = "liodom_map_register_poses: n outside 1 .. 64"; return LIODOM_ERR_INVALID_ARG; }
  if (n_edges < 0 || n_edges > mp->cfg.max_update_points) { g_last_error = "liodom_map_register_poses: n_edges negative or above the map's max_update_points"; return LIODOM_ERR_INVALID_ARG; }
  liodom_map_register_t o;
  if (opt) o = *opt; else map_register_default(&o);
  if (const char* why = map_register_check(&o)) { g_last_error = std::string("liodom_map_register_poses: ") + why; return LIODOM_ERR_INVALID_ARG; }
  for (int i = 0; i < n; i++) {
    if (pose7_check(poses + 7 * (size_t)i) != kPose7Ok) {
      g_last_error = "liodom_map_register_poses: non-finite pose, or the quaternion is not normalised (" POSE7_RULE ")"; return LIODOM_ERR_INVALID_ARG;
    }
  }
  const int cap = map_register_local_cap(&o);
  RegisterLayout L;
  if (!map_register_layout(n, cap, mp->cfg.max_update_points, &L)) { g_last_error = "liodom_map_register_poses: n x local_capacity does not fit a workspace"; return LIODOM_ERR_CAPACITY; }
  HIP_TRY(hipSetDevice(mp->device));
  if (mp->reg_bytes < (size_t)L.bytes) {
    HIP_TRY(hipStreamSynchronize(mp->stream));
    if (mp->d_reg) { (void)hipFree(mp->d_reg); mp->d_reg = nullptr; mp->reg_bytes = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&mp->d_reg), (size_t)L.bytes));
    mp->reg_bytes = (size_t)L.bytes;
  }
  unsigned char* ws = mp->d_reg;
  double* d_pose = reinterpret_cast<double*>(ws + L.pose);
  double* d_T = reinterpret_cast<double*>(ws + L.T);
  int* d_cnt = reinterpret_cast<int*>(ws + L.count);
  float4* d_pts = reinterpret_cast<float4*>(ws + L.pts);
  // the start poses as liodom_seed_stream makes its own: quaternion normalised in double, the matrix by iso_from_qt
  std::vector<double> h_pose(8 * (size_t)n, 0.0), h_T(12 * (size_t)n);
  for (int i = 0; i < n; i++) {
    pose7_normalised(poses + 7 * (size_t)i, h_pose.data() + 8 * (size_t)i);
    iso_from_qt(h_pose.data() + 8 * (size_t)i, h_pose.data() + 8 * (size_t)i + 4, h_T.data() + 12 * (size_t)i);
  }
  HIP_TRY(hipMemcpyAsync(d_pose, h_pose.data(), sizeof(double) * h_pose.size(), hipMemcpyHostToDevice, mp->stream));
  HIP_TRY(hipMemcpyAsync(d_T, h_T.data(), sizeof(double) * h_T.size(), hipMemcpyHostToDevice, mp->stream));
  if (n_edges > 0) HIP_TRY(hipMemcpyAsync(mp->d_in, edges, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, mp->stream));
  // 1. the rows' local maps, fetched once (content and order of liodom_map_get_local)
  if (map_rows_fit(mp, o.cells_xy, o.cells_z)) {
    MapRows r{};
    r.T = d_T; r.T_stride = 12; r.out = d_pts; r.out_stride = cap; r.n_out = d_cnt; r.n_stride = 1; r.total = d_cnt + n;
    r.sel = nullptr; r.list = nullptr; r.tag = 0; r.s0 = 0; r.cap = cap; r.cells_xy = o.cells_xy; r.cells_z = o.cells_z; r.sticky = 0;
    hipLaunchKernelGGL(k_map_local_rows<false>, dim3(map_rows_grid_x(n, cap), n), dim3(kMapRowsThreads), 0, mp->stream, mp->m, r);
    HIP_TRY(hipGetLastError());
  } else {
    // a visit the LDS plan cannot hold: the two launches of liodom_map_get_local, row after row, as readers do
    for (int i = 0; i < n; i++) {
      int rc = map_enqueue_local(mp, d_T + 12 * (size_t)i, o.cells_xy, o.cells_z, d_pts + (size_t)i * cap, cap, d_cnt + i, mp->stream, 0);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(d_cnt + n + i, &mp->m.st->n_result, sizeof(int), hipMemcpyDeviceToDevice, mp->stream));
    }
  }
  std::vector<int> cnt(2 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost, mp->stream));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  bool fits = true;
  for (int i = 0; i < n; i++) fits = fits && cnt[(size_t)n + i] <= cap;
  if (!fits) {
    for (int i = 0; i < n; i++) out[i].local_points = cnt[(size_t)n + i];
    g_last_error = "liodom_map_register_poses: a row's local map is larger than local_capacity"; return LIODOM_ERR_CAPACITY;
  }
  // 2. a 1 m grid per row, 3. every pass and every LM iteration of every row in one launch
  RegisterView v{};
  v.pose = d_pose; v.count = d_cnt; v.pts = d_pts;
  v.order = reinterpret_cast<int*>(ws + L.order); v.slot = reinterpret_cast<int*>(ws + L.slot);
  v.key = reinterpret_cast<unsigned long long*>(ws + L.key); v.first = reinterpret_cast<int*>(ws + L.first); v.fill = reinterpret_cast<int*>(ws + L.fill);
  v.corr = reinterpret_cast<int2*>(ws + L.corr); v.out = reinterpret_cast<liodom_map_registration_t*>(ws + L.out);
  v.edges = mp->d_in; v.n_edges = n_edges; v.local_cap = cap; v.edge_cap = std::max(L.edge_cap, 1); v.table = L.table;
  v.max_passes = o.max_passes; v.min_matches = o.min_matches;
  v.stop_t = o.stop_translation; v.stop_r = o.stop_rotation; v.min_range = o.min_range; v.max_range = o.max_range;
  {
    MapStateTimer tm(mp->stream, "liodom_map_register_poses");
    hipLaunchKernelGGL(k_map_register_grid, dim3(n), dim3(kRegThreads), 0, mp->stream, v);
    hipLaunchKernelGGL(k_map_register, dim3(n), dim3(kRegThreads), 0, mp->stream, v);
    tm.stop();
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, v.out, sizeof(liodom_map_registration_t) * (size_t)n, hipMemcpyDeviceToHost, mp->stream));
  if (corr && n_edges > 0) {
    for (int i = 0; i < n; i++)
      HIP_TRY(hipMemcpyAsync(corr + 2 * (size_t)i * (size_t)n_edges, v.corr + (size_t)i * v.edge_cap, sizeof(int2) * (size_t)n_edges, hipMemcpyDeviceToHost, mp->stream));
  }
  HIP_TRY(hipStreamSynchronize(mp->stream));      // (the staged edges and poses are the caller's memory)
  return LIODOM_OK;
}

int liodom_map_reset(liodom_map_t* mp) {
  if (!mp) { g_last_error = "liodom_map_reset: null argument"; return LIODOM_ERR_INVALID_ARG; }
  if (!mp->own_stream) { g_last_error = "liodom_map_reset: the map is attached to a handle: detach it first (liodom_attach_mapper with NULL)"; return LIODOM_ERR_BUSY; }
  HIP_TRY(hipSetDevice(mp->device));
  HIP_TRY(hipStreamSynchronize(mp->stream));
  return map_install_state(mp, nullptr, nullptr);
}

}  // extern "C"
