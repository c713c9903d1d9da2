// Host side of the place database (C-ABI liodom_places_* of include/liodom_hip.h).  Included by liodom_hip.hip (same translation
// unit: shares HIP_TRY / g_last_error).  A database touches no handle and no map: it has a HIP stream and a mutex of its own, and
// every call synchronises that stream before it returns.
#pragma once
#include <mutex>
#include <vector>

#include "kernels_places.h"

struct liodom_places {
  liodom_place_geometry_t geom;
  int W = 0, max_places = 0, max_edges = 0, device = 0;
  hipStream_t stream = nullptr;
  std::mutex mx;
  std::vector<void*> allocs;
  liodom_dev::PlaceTables tables;              // what d_tables holds
  liodom_dev::PlaceTables* d_tables = nullptr;
  unsigned long long* d_desc = nullptr;        // [max_places][W]: the places' descriptors, the first `count` rows in use
  int* d_bits = nullptr;                       // [rows_cap + 1]: bit counts of the rows of a call (the last: liodom_places_add's)
  // the places, host side: what a match is joined with and what the blob is written from
  int count = 0;
  std::vector<unsigned long long> h_desc;      // [count][W]
  std::vector<liodom_dev::PlaceStateRecord> recs;
  // staging of the calls, grown on demand (freed with the database)
  float4* d_edges = nullptr;   size_t edges_points = 0;      // rows of a chunk at the device pitch
  int* d_n = nullptr;          size_t n_rows = 0;
  unsigned long long* d_q = nullptr; size_t q_rows = 0;      // [rows][W] query descriptors of a chunk
  unsigned int* d_keys = nullptr;    size_t keys_entries = 0; // [rows][count] match keys of a chunk
  int4* d_top = nullptr;       size_t top_entries = 0;       // [rows][k]
};

namespace {

void places_free(liodom_places* db) {
  if (!db) return;
  hipSetDevice(db->device);
  if (db->stream) { hipStreamSynchronize(db->stream); hipStreamDestroy(db->stream); }
  for (void* p : db->allocs) hipFree(p);
  delete db;
}

// *ptr with room for `need` elements (a larger request frees and regrows; the stream is idle between calls)
template <typename T>
int places_ensure(liodom_places* db, T** ptr, size_t* have, size_t need) {
  if (*ptr && *have >= need) return LIODOM_OK;
  if (*ptr) {
    for (size_t i = 0; i < db->allocs.size(); i++) if (db->allocs[i] == *ptr) { db->allocs.erase(db->allocs.begin() + (long)i); break; }
    HIP_TRY(hipFree(*ptr));
    *ptr = nullptr; *have = 0;
  }
  void* raw = nullptr;
  HIP_TRY(hipMalloc(&raw, sizeof(T) * std::max<size_t>(need, 1)));
  db->allocs.push_back(raw);
  *ptr = static_cast<T*>(raw);
  *have = need;
  return LIODOM_OK;
}

constexpr int kPlaceChunkRowsMax = 32768;               // rows of one launch (grid y of k_place_match)
constexpr long long kPlaceChunkKeys = 1ll << 24;        // match keys of one chunk: 64 MiB
constexpr long long kPlaceChunkPoints = 1ll << 22;      // staged edge points of one chunk: 64 MiB

void places_fill_empty(liodom_place_match_t* out, size_t n) {
  std::memset(out, 0, sizeof(liodom_place_match_t) * n);
  for (size_t i = 0; i < n; i++) out[i].index = -1;
}

// The rows of a call, chunk by chunk: described from `edges` (or taken from `desc_in`), then — with k > 0 — matched against the
// places and ranked.  desc_out / bits_out / out are optional.  Arguments have been checked.
int places_run(liodom_places* db, const float* edges, int64_t stride, const int32_t* n_edges, const uint64_t* desc_in, int n, int k,
               uint64_t* desc_out, int32_t* bits_out, liodom_place_match_t* out) {
  using namespace liodom_dev;
  const int W = db->W, count = db->count;
  const bool match = k > 0 && count > 0 && out;
  if (out) places_fill_empty(out, (size_t)n * (size_t)k);
  const long long pitch = edges ? std::min<long long>(stride, db->max_edges) : 0;      // device row pitch, in points
  long long rows_cap = kPlaceChunkRowsMax;
  if (match) rows_cap = std::min(rows_cap, kPlaceChunkKeys / count);
  if (pitch > 0) rows_cap = std::min(rows_cap, kPlaceChunkPoints / pitch);
  rows_cap = std::max<long long>(1, std::min<long long>(rows_cap, n));
  int rc;
  if ((rc = places_ensure(db, &db->d_q, &db->q_rows, (size_t)rows_cap * (size_t)W))) return rc;
  if (edges) {
    if ((rc = places_ensure(db, &db->d_edges, &db->edges_points, (size_t)rows_cap * (size_t)std::max<long long>(pitch, 1)))) return rc;
    if ((rc = places_ensure(db, &db->d_n, &db->n_rows, (size_t)rows_cap))) return rc;
  }
  if (match) {
    if ((rc = places_ensure(db, &db->d_keys, &db->keys_entries, (size_t)rows_cap * (size_t)count))) return rc;
    if ((rc = places_ensure(db, &db->d_top, &db->top_entries, (size_t)rows_cap * (size_t)k))) return rc;
  }
  std::vector<int4> top;
  for (long long r0 = 0; r0 < n; r0 += rows_cap) {
    const int rows = (int)std::min<long long>(rows_cap, n - r0);
    if (edges) {
      if (pitch > 0) {
        HIP_TRY(hipMemcpy2DAsync(db->d_edges, sizeof(float4) * (size_t)pitch, edges + 4 * (size_t)r0 * (size_t)stride, sizeof(float4) * (size_t)stride,
                                 sizeof(float4) * (size_t)pitch, (size_t)rows, hipMemcpyHostToDevice, db->stream));
      }
      HIP_TRY(hipMemcpyAsync(db->d_n, n_edges + r0, sizeof(int) * (size_t)rows, hipMemcpyHostToDevice, db->stream));
      hipLaunchKernelGGL(k_place_describe, dim3((unsigned)rows), dim3(kPlaceDescThreads), 0, db->stream, db->d_tables, db->geom.n_rings,
                         db->geom.n_layers, db->d_edges, pitch, db->d_n, (int)pitch, db->d_q, db->d_bits);
      HIP_TRY(hipGetLastError());
      if (desc_out) HIP_TRY(hipMemcpyAsync(desc_out + (size_t)r0 * (size_t)W, db->d_q, sizeof(uint64_t) * (size_t)rows * (size_t)W, hipMemcpyDeviceToHost, db->stream));
      if (bits_out) HIP_TRY(hipMemcpyAsync(bits_out + r0, db->d_bits, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, db->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(db->d_q, desc_in + (size_t)r0 * (size_t)W, sizeof(uint64_t) * (size_t)rows * (size_t)W, hipMemcpyHostToDevice, db->stream));
    }
    if (match) {
      const int gx = std::max(1, std::min(cdiv(count, kPlaceMatchWaves), 2048));
      hipLaunchKernelGGL(k_place_match, dim3((unsigned)gx, (unsigned)rows), dim3(kPlaceMatchThreads), sizeof(uint64_t) * 64 * (size_t)W, db->stream,
                         db->d_desc, count, W, db->d_q, db->d_keys);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_place_topk, dim3((unsigned)rows), dim3(kPlaceTopkThreads), 0, db->stream, db->d_keys, count, k, db->d_top);
      HIP_TRY(hipGetLastError());
      top.resize((size_t)rows * (size_t)k);
      HIP_TRY(hipMemcpyAsync(top.data(), db->d_top, sizeof(int4) * top.size(), hipMemcpyDeviceToHost, db->stream));
    }
    HIP_TRY(hipStreamSynchronize(db->stream));      // (the staged rows are the caller's memory; the next chunk reuses the staging)
    if (match) {
      for (size_t i = 0; i < top.size(); i++) {
        const int4 t = top[i];
        if (t.x < 0 || t.x >= count) continue;       // (a rank beyond the places: the -1 row stands)
        liodom_place_match_t& m = out[(size_t)r0 * (size_t)k + i];
        const PlaceStateRecord& rec = db->recs[(size_t)t.x];
        m.index = t.x; m.distance = t.y; m.shift = t.z; m.bits_place = rec.bits; m.id = rec.id;
        std::memcpy(m.place_pose, rec.pose, sizeof(rec.pose));
        place_match_pose(rec.pose, t.z, m.pose);
      }
    }
  }
  return LIODOM_OK;
}

int places_check_rows(const liodom_places* db, const float* edges, int64_t stride, const int32_t* n_edges, int n, const char* who) {
  if (!db || n < 0 || n > liodom_dev::kPlacesMax || stride < 0 || (n > 0 && !n_edges)) {
    g_last_error = std::string(who) + ": null database or counts, a row count that is negative or above 2^20, or a negative stride"; return LIODOM_ERR_INVALID_ARG;
  }
  bool any = false;
  for (int i = 0; i < n; i++) {
    if (n_edges[i] < 0 || n_edges[i] > stride || n_edges[i] > db->max_edges) {
      g_last_error = std::string(who) + ": a row's edge count is negative, above the row stride or above max_edges"; return LIODOM_ERR_INVALID_ARG;
    }
    any = any || n_edges[i] > 0;
  }
  if (any && !edges) { g_last_error = std::string(who) + ": null edges"; return LIODOM_ERR_INVALID_ARG; }
  return LIODOM_OK;
}

}  // namespace

extern "C" {

void liodom_place_geometry_default(liodom_place_geometry_t* g) {
  if (!g) return;
  std::memset(g, 0, sizeof(*g));
  g->n_rings = 16; g->n_layers = 4;
  g->r_max = 80.0; g->z_min = -4.0; g->z_max = 12.0;
}

int liodom_places_create(const liodom_place_geometry_t* geom, int max_places, int max_edges, liodom_places_t** out) {
  using namespace liodom_dev;
  if (!geom || !out) { g_last_error = "liodom_places_create: null argument"; return LIODOM_ERR_INVALID_ARG; }
  *out = nullptr;
  if (!place_geometry_ok(geom->n_rings, geom->n_layers, geom->r_max, geom->z_min, geom->z_max)) {
    g_last_error = "liodom_places_create: not a geometry (1 <= n_rings * n_layers <= 64, r_max > 0, z_min < z_max, all finite)"; return LIODOM_ERR_INVALID_ARG;
  }
  if (max_places < 1 || max_places > kPlacesMax || max_edges < 1 || max_edges > (1 << 24)) {
    g_last_error = "liodom_places_create: max_places outside 1 .. 2^20 or max_edges outside 1 .. 2^24"; return LIODOM_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "liodom_places_create: no HIP device available (this library has no CPU fallback)";
    return LIODOM_ERR_NO_DEVICE;
  }
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  liodom_places* db = new liodom_places();
  db->geom = *geom;
  db->geom.reserved = 0;
  db->W = geom->n_rings * geom->n_layers;
  db->max_places = max_places; db->max_edges = max_edges; db->device = dev;
  place_make_tables(geom->n_rings, geom->n_layers, geom->r_max, geom->z_min, geom->z_max, &db->tables);
  auto build = [&]() -> int {
    HIP_TRY(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    size_t have = 0;
    int rc;
    if ((rc = places_ensure(db, &db->d_tables, &have, 1))) return rc;
    have = 0;
    if ((rc = places_ensure(db, &db->d_desc, &have, (size_t)max_places * (size_t)db->W))) return rc;
    have = 0;
    if ((rc = places_ensure(db, &db->d_bits, &have, (size_t)kPlaceChunkRowsMax + 1))) return rc;
    HIP_TRY(hipMemcpyAsync(db->d_tables, &db->tables, sizeof(db->tables), hipMemcpyHostToDevice, db->stream));
    HIP_TRY(hipStreamSynchronize(db->stream));
    return LIODOM_OK;
  };
  const int rc = build();
  if (rc != LIODOM_OK) { places_free(db); return rc; }
  *out = db;
  return LIODOM_OK;
}

void liodom_places_destroy(liodom_places_t* db) { places_free(db); }

int liodom_places_count(liodom_places_t* db, int32_t* count) {
  if (!db || !count) { g_last_error = "liodom_places_count: null argument"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  *count = db->count;
  return LIODOM_OK;
}

int liodom_places_reset(liodom_places_t* db) {
  if (!db) { g_last_error = "liodom_places_reset: null database"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  HIP_TRY(hipSetDevice(db->device));
  HIP_TRY(hipStreamSynchronize(db->stream));
  db->count = 0;
  db->h_desc.clear();
  db->recs.clear();
  return LIODOM_OK;
}

int liodom_places_describe(liodom_places_t* db, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges, int n,
                           uint64_t* desc_out, int32_t* bits_out) {
  int rc = places_check_rows(db, edges_xyzi, edge_stride_points, n_edges, n, "liodom_places_describe");
  if (rc) return rc;
  if (n > 0 && !desc_out) { g_last_error = "liodom_places_describe: null desc_out"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  std::lock_guard<std::mutex> lk(db->mx);
  HIP_TRY(hipSetDevice(db->device));
  // (a null cloud with all counts 0 still runs: the kernel writes the all-zero descriptors)
  static const float none[4] = {0.f, 0.f, 0.f, 0.f};
  return places_run(db, edges_xyzi ? edges_xyzi : none, edges_xyzi ? edge_stride_points : 0, n_edges, nullptr, n, 0, desc_out, bits_out, nullptr);
}

int liodom_places_add(liodom_places_t* db, const float* edges_xyzi, int n_edges, const double* pose, int64_t id, int32_t* index) {
  using namespace liodom_dev;
  if (!db || !pose || n_edges < 0 || (n_edges > 0 && !edges_xyzi)) { g_last_error = "liodom_places_add: null database, pose or edges, or a negative count"; return LIODOM_ERR_INVALID_ARG; }
  if (n_edges > db->max_edges) { g_last_error = "liodom_places_add: more edges than max_edges"; return LIODOM_ERR_INVALID_ARG; }
  if (pose7_check(pose) != kPose7Ok) { g_last_error = "liodom_places_add: non-finite pose, or the quaternion is not normalised (" POSE7_RULE ")"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  if (db->count >= db->max_places) { g_last_error = "liodom_places_add: the database holds max_places places"; return LIODOM_ERR_CAPACITY; }
  HIP_TRY(hipSetDevice(db->device));
  const int W = db->W;
  int rc;
  if ((rc = places_ensure(db, &db->d_edges, &db->edges_points, (size_t)std::max(n_edges, 1)))) return rc;
  if ((rc = places_ensure(db, &db->d_n, &db->n_rows, 1))) return rc;
  if (n_edges) HIP_TRY(hipMemcpyAsync(db->d_edges, edges_xyzi, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, db->stream));
  HIP_TRY(hipMemcpyAsync(db->d_n, &n_edges, sizeof(int), hipMemcpyHostToDevice, db->stream));
  // described straight into the place's row: it is not a place until count says so
  unsigned long long* row = db->d_desc + (size_t)db->count * (size_t)W;
  int* d_bit = db->d_bits + kPlaceChunkRowsMax;
  hipLaunchKernelGGL(k_place_describe, dim3(1), dim3(kPlaceDescThreads), 0, db->stream, db->d_tables, db->geom.n_rings, db->geom.n_layers,
                     db->d_edges, 0ll, db->d_n, n_edges, row, d_bit);
  HIP_TRY(hipGetLastError());
  std::vector<unsigned long long> words((size_t)W);
  int bits = 0;
  HIP_TRY(hipMemcpyAsync(words.data(), row, sizeof(uint64_t) * (size_t)W, hipMemcpyDeviceToHost, db->stream));
  HIP_TRY(hipMemcpyAsync(&bits, d_bit, sizeof(int), hipMemcpyDeviceToHost, db->stream));
  HIP_TRY(hipStreamSynchronize(db->stream));
  PlaceStateRecord rec;
  std::memset(&rec, 0, sizeof(rec));
  rec.id = id; rec.bits = bits;
  std::memcpy(rec.pose, pose, sizeof(rec.pose));
  db->h_desc.insert(db->h_desc.end(), words.begin(), words.end());
  db->recs.push_back(rec);
  if (index) *index = db->count;
  db->count++;
  return LIODOM_OK;
}

int liodom_places_query(liodom_places_t* db, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges, int n, int k,
                        liodom_place_match_t* out, int32_t* bits_query) {
  int rc = places_check_rows(db, edges_xyzi, edge_stride_points, n_edges, n, "liodom_places_query");
  if (rc) return rc;
  if (k < 1 || k > liodom_dev::kPlaceKMax || (n > 0 && !out)) { g_last_error = "liodom_places_query: k outside 1 .. 16, or null out"; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  std::lock_guard<std::mutex> lk(db->mx);
  if (db->count == 0 && !bits_query) { places_fill_empty(out, (size_t)n * (size_t)k); return LIODOM_OK; }
  HIP_TRY(hipSetDevice(db->device));
  static const float none[4] = {0.f, 0.f, 0.f, 0.f};
  return places_run(db, edges_xyzi ? edges_xyzi : none, edges_xyzi ? edge_stride_points : 0, n_edges, nullptr, n, k, nullptr, bits_query, out);
}

int liodom_places_query_desc(liodom_places_t* db, const uint64_t* desc, int n, int k, liodom_place_match_t* out) {
  if (!db || n < 0 || n > liodom_dev::kPlacesMax || k < 1 || k > liodom_dev::kPlaceKMax || (n > 0 && (!desc || !out))) {
    g_last_error = "liodom_places_query_desc: null database, descriptors or out, a row count that is negative or above 2^20, or k outside 1 .. 16";
    return LIODOM_ERR_INVALID_ARG;
  }
  if (n == 0) return LIODOM_OK;
  std::lock_guard<std::mutex> lk(db->mx);
  if (db->count == 0) { places_fill_empty(out, (size_t)n * (size_t)k); return LIODOM_OK; }
  HIP_TRY(hipSetDevice(db->device));
  return places_run(db, nullptr, 0, nullptr, desc, n, k, nullptr, nullptr, out);
}

int liodom_places_state_size(liodom_places_t* db, int64_t* bytes) {
  if (!db || !bytes) { g_last_error = "liodom_places_state_size: null argument"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  *bytes = liodom_dev::place_state_bytes(db->W, db->count);
  return LIODOM_OK;
}

int liodom_places_export_state(liodom_places_t* db, void* blob, int64_t cap, int64_t* bytes) {
  using namespace liodom_dev;
  if (!db || !bytes) { g_last_error = "liodom_places_export_state: null argument"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  HIP_TRY(hipSetDevice(db->device));
  HIP_TRY(hipStreamSynchronize(db->stream));
  const int64_t need = place_state_bytes(db->W, db->count);
  *bytes = need;
  if (!blob || cap < need) { g_last_error = "liodom_places_export_state: the buffer is smaller than the blob"; return LIODOM_ERR_CAPACITY; }
  PlaceStateHeader hd;
  std::memset(&hd, 0, sizeof(hd));
  std::memcpy(hd.magic, "LIODOMPL", 8);
  hd.version = kPlaceStateVersion; hd.header_bytes = (uint32_t)kPlaceStateHeaderBytes; hd.total_bytes = (uint64_t)need;
  hd.n_rings = db->geom.n_rings; hd.n_layers = db->geom.n_layers;
  hd.r_max = db->geom.r_max; hd.z_min = db->geom.z_min; hd.z_max = db->geom.z_max;
  hd.count = db->count;
  unsigned char* b = static_cast<unsigned char*>(blob);
  std::memcpy(b, &hd, sizeof(hd));
  std::memcpy(b + kPlaceStateHeaderBytes, &db->tables, sizeof(db->tables));
  unsigned char* desc = b + kPlaceStateHeaderBytes + kPlaceTablesBytes;
  if (db->count) {
    std::memcpy(desc, db->h_desc.data(), sizeof(uint64_t) * db->h_desc.size());
    std::memcpy(desc + sizeof(uint64_t) * db->h_desc.size(), db->recs.data(), sizeof(PlaceStateRecord) * db->recs.size());
  }
  return LIODOM_OK;
}

int liodom_places_import_state(liodom_places_t* db, const void* blob, int64_t bytes) {
  using namespace liodom_dev;
  if (!db || !blob || bytes < 0) { g_last_error = "liodom_places_import_state: null argument or a negative size"; return LIODOM_ERR_INVALID_ARG; }
  std::lock_guard<std::mutex> lk(db->mx);
  const int32_t nm[2] = {db->geom.n_rings, db->geom.n_layers};
  const double rz[3] = {db->geom.r_max, db->geom.z_min, db->geom.z_max};
  const char* why = "";
  const int rc = place_state_validate(blob, bytes, nm, rz, db->max_places, &why);
  if (rc != LIODOM_OK) { g_last_error = std::string("liodom_places_import_state: ") + why; return rc; }
  PlaceStateHeader hd;
  std::memcpy(&hd, blob, sizeof(hd));
  const unsigned char* desc = static_cast<const unsigned char*>(blob) + kPlaceStateHeaderBytes + kPlaceTablesBytes;
  const size_t words = (size_t)hd.count * (size_t)db->W;
  std::vector<unsigned long long> h_desc(words);
  std::vector<PlaceStateRecord> recs((size_t)hd.count);
  if (hd.count) {
    std::memcpy(h_desc.data(), desc, sizeof(uint64_t) * words);
    std::memcpy(recs.data(), desc + sizeof(uint64_t) * words, sizeof(PlaceStateRecord) * recs.size());
  }
  HIP_TRY(hipSetDevice(db->device));
  // the device rows first: while `count` stands, rows at and beyond it are nobody's — but rows below it are, so on a failed
  // upload the old places are written back from the host's copy
  if (words) {
    hipError_t e = hipMemcpyAsync(db->d_desc, h_desc.data(), sizeof(uint64_t) * words, hipMemcpyHostToDevice, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) {
      if (!db->h_desc.empty()) {
        hipMemcpyAsync(db->d_desc, db->h_desc.data(), sizeof(uint64_t) * db->h_desc.size(), hipMemcpyHostToDevice, db->stream);
        hipStreamSynchronize(db->stream);
      }
      g_last_error = std::string("liodom_places_import_state: upload failed: ") + hipGetErrorString(e);
      return LIODOM_ERR_HIP;
    }
  } else {
    HIP_TRY(hipStreamSynchronize(db->stream));
  }
  db->h_desc.swap(h_desc);
  db->recs.swap(recs);
  db->count = hd.count;
  return LIODOM_OK;
}

}  // extern "C"
