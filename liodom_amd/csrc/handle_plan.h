// handle_plan.h — what a handle will be, decided before anything is allocated: every code path it takes and every capacity, as a
// pure function of the caller's parameters, the environment switches and three facts about the device.  Plain C++17 without a
// HIP include, so the arithmetic that host and kernels must agree on runs under g++ and host sanitizers
// (tests/handle_plan_main.cc, tests/test_handle_plan.py).  liodom_create (liodom_hip.hip) gathers HandleCaps, calls
// read_handle_env and plan_handle, and then only allocates, uploads and probes what the plan says.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/liodom_hip.h"
#include "liodom_sizes.h"

namespace liodom_dev {

// The environment switches of handle creation, parsed and clamped once (read_handle_env).  This is the list of the switches.
struct HandleEnv {
  bool pipe_flags = true;        // LIODOM_PIPE_FLAGS=0: events instead of flags between the extraction and the odometry stream
  bool map_rows = true;          // LIODOM_MAP_ROWS=0: map readers take the two launches of liodom_map_get_local per stream (equality test, cost tool)
  int hash_build = -1;           // LIODOM_HASH_BUILD: 0 "global" (three global-atomic kernels), 1 anything else (k_hash_build, LDS); -1 unset: by stream count
  int lds_cells_max = kLdsCellsMax;   // LIODOM_LDS_CELLS_MAX: occupied-cell limit of the LDS-built table, in [1, kLdsCellsMax] (lowered by tests)
  bool early_rebuild = true;     // LIODOM_EARLY_REBUILD=0: never the streamed rebuild
  bool safe_mode = false;        // LIODOM_SAFE_MODE=1: no in-kernel waits from the start (plan_enter_safe_mode)
  int debug_clocks = 0;          // LIODOM_DEBUG_CLOCKS (instrumented builds only): in-kernel phase timestamps / histograms, tools/gpu_debug.py
  bool ring_split = true;        // LIODOM_RING_SPLIT=0: always k_classify + k_ring_scatter
  bool ring_split_lb = true;     // LIODOM_RING_SPLIT_LB=0: lock-step batches take k_classify + k_ring_scatter instead of k_ring_split_lb
  int ring_pitch = 0;            // LIODOM_RING_PITCH: points a ring may hold in the pitched layout, at least 8 (tests: a pitch that real rings outgrow); 0 unset
  bool hash_incr = true;         // LIODOM_HASH_INCR=0: k_hash_build every scan, no k_hash_append
  float rebuild_delta = 0.25f;   // LIODOM_REBUILD_DELTA: DevView::rebuild_delta, accepted only in (0, 0.45]
  bool knn8 = true;              // LIODOM_KNN8=0: lock-step batches keep k_knn<128>
  int hb_slack = kHbSlackMin;    // LIODOM_HB_SLACK: DevView::hb_slack_min, at least 0 (tests: cells that run out of room)
  int hb_new_room = kHbNewRoom;  // LIODOM_HB_NEW_ROOM: DevView::hb_new_room, at least 1
  int knn_save = 2;              // LIODOM_KNN_SAVE: 2 the second kNN pass re-ranks the first pass's kept candidates and prunes with its fifth
                                 // distance; 1: pruning bound only; 0: the second pass searches like the first (all three give the same results)
  bool knn_exact_only = false;   // LIODOM_KNN_EXACT_ONLY=1 (test switch): every kNN query takes the exact list path
  int knn_overlap = 1;           // LIODOM_KNN_OVERLAP: 0 no overlapped second pass and no chain mode; 2: also where the pass takes more than a third of the wave slots
  bool chain = true;             // LIODOM_CHAIN=0: no chain mode
  int speculate = 1;             // LIODOM_SPECULATE in [0, 7]: speculative hand-over 0 off, 1 by the model's predicted cost change, 2 (tests) as early as
                                 // possible; 4 / 5 (debugging): only the first / only the finalising solve's hand-over
  double spec_theta = 0.8;       // LIODOM_SPEC_THETA: the predictor's threshold (fraction of the function tolerance)
  double wait_ms = 50.0;         // LIODOM_WAIT_MS: wall-clock bound of every in-kernel wait, accepted only in [1, 10000]
  bool serialised = false;       // a known kernel serialiser is set (AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, ROCPROFILER_PMC, ROCPROF_COUNTERS):
                                 // kernels of different streams never run side by side, in-kernel waits could only time out
};

// The only getenv site of handle creation.
inline HandleEnv read_handle_env() {
  HandleEnv e;
  auto num = [](const char* name, int dflt) { const char* s = std::getenv(name); return s ? std::atoi(s) : dflt; };
  e.pipe_flags = num("LIODOM_PIPE_FLAGS", 1) != 0;
  e.map_rows = num("LIODOM_MAP_ROWS", 1) != 0;
  if (const char* s = std::getenv("LIODOM_HASH_BUILD")) e.hash_build = std::strcmp(s, "global") != 0 ? 1 : 0;
  e.lds_cells_max = std::max(1, std::min(kLdsCellsMax, num("LIODOM_LDS_CELLS_MAX", kLdsCellsMax)));
  e.early_rebuild = num("LIODOM_EARLY_REBUILD", 1) != 0;
  e.safe_mode = num("LIODOM_SAFE_MODE", 0) != 0;
  e.debug_clocks = num("LIODOM_DEBUG_CLOCKS", 0);
  e.ring_split = num("LIODOM_RING_SPLIT", 1) != 0;
  e.ring_split_lb = num("LIODOM_RING_SPLIT_LB", 1) != 0;
  if (const char* s = std::getenv("LIODOM_RING_PITCH")) e.ring_pitch = std::max(8, std::atoi(s));
  e.hash_incr = num("LIODOM_HASH_INCR", 1) != 0;
  if (const char* s = std::getenv("LIODOM_REBUILD_DELTA")) { const float d = (float)std::atof(s); if (d > 0.0f && d <= 0.45f) e.rebuild_delta = d; }
  e.knn8 = num("LIODOM_KNN8", 1) != 0;
  if (const char* s = std::getenv("LIODOM_HB_SLACK")) e.hb_slack = std::max(0, std::atoi(s));
  if (const char* s = std::getenv("LIODOM_HB_NEW_ROOM")) e.hb_new_room = std::max(1, std::atoi(s));
  e.knn_save = num("LIODOM_KNN_SAVE", 2);
  e.knn_exact_only = num("LIODOM_KNN_EXACT_ONLY", 0) != 0;
  e.knn_overlap = num("LIODOM_KNN_OVERLAP", 1);
  e.chain = num("LIODOM_CHAIN", 1) != 0;
  e.speculate = std::max(0, std::min(7, num("LIODOM_SPECULATE", 1)));
  if (const char* s = std::getenv("LIODOM_SPEC_THETA")) e.spec_theta = std::atof(s);
  if (const char* s = std::getenv("LIODOM_WAIT_MS")) { const double x = std::atof(s); if (x >= 1.0 && x <= 10000.0) e.wait_ms = x; }
  for (const char* name : {"AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING", "ROCPROFILER_PMC", "ROCPROF_COUNTERS"}) {
    const char* s = std::getenv(name);
    if (s && s[0] && std::strcmp(s, "0") != 0) e.serialised = true;
  }
  return e;
}

// What the device contributes; liodom_create gathers it once, before planning.
struct HandleCaps {
  int cus = 0;                    // compute units
  int ring_split_wgs_per_cu = 0;  // k_ring_split<> workgroups resident per CU at its LDS size; 0: the attribute or the occupancy call failed
  bool instrumented = false;      // the build carries the in-kernel instrumentation (kInstrument)
};

struct HandlePlan {
  // ---- code paths (host only) ----
  bool lockstep = false;        // n_streams >= 16: a lock-step batch (throughput-bound; picks the hash build, the kNN kernels, events between the streams)
  bool lds_hash_build = false;  // k_hash_build (one workgroup per stream, LDS) instead of the 3 global-atomic kernels
  bool use_flags = false;       // pipelined replay: dependencies between the two streams through flags in device memory instead of events
  bool flag_gate = false;       // ... polled by a one-wave gate launch in front of the scan's first k_knn launch instead of by that launch itself
  bool ring_split = true;       // ring split in one pass (k_ring_split) where every workgroup of the launch is resident at once
  int ring_split_max_wgs = 0;   // ... i.e. launches of at most this many workgroups (occupancy of k_ring_split x CUs, with headroom for the odometry chain's kernels)
  bool ring_split_lb = false;   // lock-step batches: k_ring_split_lb (one pass, rings at a fixed pitch, predecessors' counts summed as they appear)
  bool knn8 = false;            // lock-step batches: k_knn8 (eight lanes per query) instead of k_knn<128>
  int knn8_grid = 1;            // k_knn8 workgroups per stream (each walks the blocks b, b + grid, ... of 32 queries)
  bool ov_ok = false;           // the handle qualifies for the overlapped second kNN pass (one stream, streamed rebuild, the pass leaves 2/3 of the wave slots free)
  bool chain_ok = false;        // the handle qualifies for chain mode (one stream, streamed rebuild, no IMU override; the passes' waiting workgroups
                                // may take up to half of the wave slots)
  bool safe_mode = false;       // no in-kernel waits at all: events between the streams, one workgroup per solve, three-kernel hash rebuild
  bool map_rows = true;         // map readers go through k_map_local_rows
  size_t ring_lds_bytes = 0;    // dynamic LDS of k_ring_extract
  // ---- optional buffers ----
  int knn_save = 2;             // 0 none / 1 knn_save_q / 2 + knn_save_pos, knn_save_g
  bool pose_covariance = false; // cov_raw, cov_log, cov_host
  unsigned long long wait_ticks = 0;   // g_wait_ticks: bound of every in-kernel wait in 100 MHz ticks
  // ---- the scalar members of DevView, under their names there (plan_to_view copies them) ----
  double min_range = 0, max_range = 0;
  int lidar_type = 0, scan_lines = 0, scan_regions = 0, edges_per_region = 0;
  long long min_points_per_scan = 0;
  int prev_frames = 0, apply_on_ftol = 0, rotation_mode = 0, filter_local_map = 0, lm_groups = 1;
  float vox_inv = 0;
  int n_streams = 0, max_points = 0, ring_cap = 0, slots_per_ring = 0, edge_cap = 0, map_cap = 0, table_size = 0;
  int pose_log_cap = 0, debug = 0;
  size_t ring_id_stride = 0;
  int tile_cap = 0, split_pad = 0, lb_hpad = 0, ring_pitch = 0;
  size_t ring_stride = 0;
  int use_imu = 0, mapping = 0, recv_cap = 0, lds_cells_max = 0;
  int mask_stride = 0, knn_partials = 0, knn_queries = 0;
  int used_cap = 0, sorted_cap = 0, ovf_base = 0;
  float rebuild_delta = 0;
  int hb_spill_base = 0, hb_slack_min = 0, hb_new_room = 0, hash_incr = 0;
  int early_rebuild = 0, knn_grid = 0, knn_exact_only = 0, knn_blocks = 0;
  double spec_theta = 0;
  int spec_backoff = 0, speculate = 0;
};

// Copies the plan's DevView scalars into a DevView (a template: this header does not know the device types).  The only writer of
// those members of a handle's view; the pointers, laser_to_base and the host-mapped records are liodom_create's.
template <typename View>
void plan_to_view(const HandlePlan& p, View* v) {
  v->min_range = p.min_range; v->max_range = p.max_range;
  v->lidar_type = p.lidar_type; v->scan_lines = p.scan_lines; v->scan_regions = p.scan_regions; v->edges_per_region = p.edges_per_region;
  v->min_points_per_scan = p.min_points_per_scan;
  v->prev_frames = p.prev_frames; v->apply_on_ftol = p.apply_on_ftol; v->rotation_mode = p.rotation_mode;
  v->filter_local_map = p.filter_local_map; v->lm_groups = p.lm_groups; v->vox_inv = p.vox_inv;
  v->n_streams = p.n_streams; v->max_points = p.max_points; v->ring_cap = p.ring_cap; v->slots_per_ring = p.slots_per_ring;
  v->edge_cap = p.edge_cap; v->map_cap = p.map_cap; v->table_size = p.table_size;
  v->pose_log_cap = p.pose_log_cap; v->debug = p.debug;
  v->ring_id_stride = p.ring_id_stride; v->tile_cap = p.tile_cap; v->split_pad = p.split_pad;
  v->lb_hpad = p.lb_hpad; v->ring_pitch = p.ring_pitch; v->ring_stride = p.ring_stride;
  v->use_imu = p.use_imu; v->mapping = p.mapping; v->recv_cap = p.recv_cap; v->lds_cells_max = p.lds_cells_max;
  v->mask_stride = p.mask_stride; v->knn_partials = p.knn_partials; v->knn_queries = p.knn_queries;
  v->used_cap = p.used_cap; v->sorted_cap = p.sorted_cap; v->ovf_base = p.ovf_base; v->rebuild_delta = p.rebuild_delta;
  v->hb_spill_base = p.hb_spill_base; v->hb_slack_min = p.hb_slack_min; v->hb_new_room = p.hb_new_room; v->hash_incr = p.hash_incr;
  v->early_rebuild = p.early_rebuild; v->knn_grid = p.knn_grid; v->knn_exact_only = p.knn_exact_only; v->knn_blocks = p.knn_blocks;
  v->spec_theta = p.spec_theta; v->spec_backoff = p.spec_backoff; v->speculate = p.speculate;
}

// Safe mode: every dependency that a kernel of this handle would wait for INSIDE a kernel is replaced by one the runtime orders.
// In-kernel waits need the producer to run beside the waiter; a GPU saturated by another process (or a tool that serialises
// kernels) breaks that, the bounded waits give up (LIODOM_STATUS_PIPE_TIMEOUT / LM_SYNC_TIMEOUT) and the scan is lost.  Afterwards:
//   stream dependencies   flags polled by kernels            -> hipEvent pairs
//   second kNN pass       beside the first solve, polling     -> behind it in stream order
//   pose solve            G workgroups exchanging partial sums in the launch -> one workgroup (sums in a different order: poses
//                         agree with the G-workgroup solve to rounding, not to the bit)
//   ring split            one pass whose tiles wait for each other's histograms -> k_classify + k_ring_scatter (bit-identical)
//   hash rebuild          workgroups inside the solve launches waiting for its pose -> k_window_insert / k_hash_alloc /
//                         k_hash_scatter behind the solve (bit-identical: test_early_rebuild_equals_three_kernel_rebuild)
// Entered by liodom_reset() after a timeout — the capacities stay as allocated — or inside plan_handle with LIODOM_SAFE_MODE=1,
// where the steps behind it size the tables for a handle without the streamed rebuild.
inline void plan_enter_safe_mode(HandlePlan* p) {
  p->safe_mode = true;
  p->use_flags = false;
  p->chain_ok = false;
  p->ov_ok = false;          // (these two are read only by scans that overlap or chain, which need use_flags: nothing changes with them,
  p->speculate = 0;          //  but a handle that fell back reports the paths of one created in safe mode)
  p->lm_groups = 1;
  p->early_rebuild = 0;      // (after a timeout: the second table, the padding and the overflow list stay allocated and unused)
  p->ring_split = false;     // k_ring_split's workgroups wait for each other inside the launch: k_classify + k_ring_scatter instead
  p->ring_split_lb = false;  // (k_ring_split_lb's tiles wait for their predecessors' counts; the pitched buffers stay allocated)
}

namespace plan_detail {
inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline long long round_up(long long x, long long m) { return (x + m - 1) / m * m; }
}  // namespace plan_detail

// liodom_create's first refusal, on its own: the create reports it before it looks for a device.
inline int plan_check_params(const liodom_params_t* params, const liodom_config_t* config, const char** error) {
  if (params->scan_lines < 1 || params->scan_lines > 254 || params->scan_regions < 1 ||
      params->edges_per_region < 0 || params->local_map_size < 1 || params->local_map_size > (uint64_t)kMaxFrames ||
      config->n_streams < 1 || config->max_points < 1 || !(params->max_range > params->min_range)) {
    *error = "liodom_create: parameter out of range";
    return LIODOM_ERR_INVALID_ARG;
  }
  return LIODOM_OK;
}

// The plan.  Sizes are computed in 64 bits and must fit the ints of DevView.  Refusals, in this order: parameter range
// (LIODOM_ERR_INVALID_ARG), pick lists over 160 KiB of LDS (LIODOM_ERR_CAPACITY), edge capacity too large for the solve's LDS
// (LIODOM_ERR_INVALID_ARG), capacities beyond 32 bits (LIODOM_ERR_CAPACITY).  The order of the steps carries meaning; each
// dependency is said where it binds.
inline int plan_handle(const liodom_params_t* params, const liodom_config_t* config, const HandleCaps& caps, const HandleEnv& env,
                       HandlePlan* out, const char** error) {
  using plan_detail::cdiv;
  using plan_detail::round_up;
  if (int rc = plan_check_params(params, config, error)) return rc;
  HandlePlan p;
  const int S = config->n_streams, H = params->scan_lines, P = (int)params->local_map_size;

  // 1. what the caller's parameters say as they are
  p.min_range = params->min_range; p.max_range = params->max_range;
  p.lidar_type = params->lidar_type; p.scan_lines = H;
  p.scan_regions = params->scan_regions; p.edges_per_region = params->edges_per_region;
  p.min_points_per_scan = (long long)params->min_points_per_scan;
  p.prev_frames = P;
  p.apply_on_ftol = config->lm_apply_step_on_ftol;
  p.rotation_mode = config->pose_rotation_mode != 0 ? 1 : 0;
  p.filter_local_map = (params->filter_local_map && !params->mapping) ? 1 : 0;   // laser_odometry.cc:286
  p.vox_inv = 1.0f / 0.4f;                                                       // setLeafSize(0.4) :290
  p.n_streams = S;
  p.max_points = config->max_points;
  // (k_ring_extract stages nothing per point in LDS, so there is no per-ring capacity — a ring may hold up to max_points
  // points; config.max_width only picks the kernel instance, launch_extract)
  p.ring_cap = config->max_points;
  p.use_imu = params->use_imu ? 1 : 0;
  p.mapping = params->mapping ? 1 : 0;
  p.pose_log_cap = std::max(1, config->pose_log_capacity);
  p.pose_covariance = config->pose_covariance != 0;
  p.map_rows = env.map_rows;
  p.lds_cells_max = env.lds_cells_max;
  p.rebuild_delta = env.rebuild_delta;
  p.hb_slack_min = env.hb_slack; p.hb_new_room = env.hb_new_room;
  p.knn_save = env.knn_save;
  p.knn_exact_only = env.knn_exact_only ? 1 : 0;
  p.wait_ticks = (unsigned long long)(env.wait_ms * 1.0e5);
  p.lockstep = S >= 16;

  // 2. pick lists and edge capacity; the two refusals that depend on them.  (A product beyond 32 bits is a pick list over
  //    160 KiB as well: scan_lines is at most 254, so nothing below this step overflows through the edge capacity.)
  const long long slots = (long long)params->scan_regions * ((long long)params->edges_per_region + 1);
  if (slots > INT_MAX || ring_extract_lds_bytes((int)slots, params->scan_regions) > 160 * 1024) {
    *error = "pick lists (scan_regions * (edges_per_region + 1)) exceed 160 KiB of LDS";
    return LIODOM_ERR_CAPACITY;
  }
  p.slots_per_ring = (int)slots;
  p.ring_lds_bytes = ring_extract_lds_bytes(p.slots_per_ring, params->scan_regions);
  // There are two edge counts.  `edges` is what the parameters allow, unrounded: the thresholds of the solve's split were
  // measured against it.  edge_cap is the buffers' capacity, rounded up to 64: launches are sized from it, flag_gate included.
  const int edges = H * p.slots_per_ring;
  p.edge_cap = (int)round_up(std::max(1, edges), 64);
  // (the solve's dynamic LDS is its index list, up to ~36 800 edges; 16 KiB are left for its static LDS, 8.7 KiB at most today)
  if (lm_lds_bytes(p.edge_cap) + 16384 > 160 * 1024) {
    *error = "liodom_create: edge capacity too large for the solve's LDS tile";
    return LIODOM_ERR_INVALID_ARG;
  }

  // 3. hash build.  Measured on MI355X (headline shape): one stream rebuilds its hash in 28 us with the three global-atomic
  //    kernels (many workgroups) but needs 86 us as a single LDS workgroup; 64 lock-step streams need 247 us (L2-atomic bound)
  //    against 103 us with one LDS workgroup each.
  p.lds_hash_build = env.hash_build < 0 ? p.lockstep : env.hash_build != 0;

  // 4. Flags instead of events between the extraction and the odometry stream: the first kNN launch of a scan polls the
  //    extraction's flag in every workgroup, so all its workgroups must fit on the GPU with ample room left for the
  //    extraction kernels they may be waiting for (512-thread workgroups): one stream only, and at most 12 of the 24
  //    wave slots per CU the kernel's 74 VGPRs allow — HDL-64 (2 816 waves of 3 072) qualifies, Ouster-128 (5 632) does
  //    not: with 24 it starved the extraction in the non-pipelined replay until the bounded waits gave up.
  //    (Lock-step batches are throughput-bound: 11 us per multi-millisecond step do not matter there.)
  //    Larger launches: a one-wave gate launch polls instead.  liodom_create's probe may still clear use_flags.
  p.use_flags = !p.lockstep && !env.serialised && env.pipe_flags;
  p.flag_gate = !(S == 1 && cdiv(cdiv(p.edge_cap, 8), 2) * 4 <= (long long)caps.cus * 12);

  // 5. solve split over G workgroups (partial sums exchanged inside the launch, ~3 us per evaluation under load): pays once an
  //    evaluation is long enough.  Measured (scans/s, G = 1 / 4 / 8): HDL-64 10.1k / 10.35k / 10.34k, Ouster-128 7.3k / 8.1k / 8.3k,
  //    VLP-16 12.2k / 12.1k / -.  (round 3, A/B on one box, scans/s: HDL-64 G = 2 / 4 / 8: 11.4k / 11.9k / 12.1k; VLP-16
  //    G = 1 / 2 / 4 / 8: 13.2k / 13.5k / 14.0k / 14.0k; 16 workgroups — a build with kLmGroupsMax = 16 — lose: the exchange's
  //    fan-in grows, HDL-64 11.4k, Ouster-128 8.8k vs 9.05k)
  {
    const int auto_g = S > 4 ? 1 : (edges >= 2048 ? kLmGroupsMax : (edges >= 512 ? 4 : 1));
    p.lm_groups = config->lm_workgroups == 0 ? auto_g : std::max(1, std::min(kLmGroupsMax, config->lm_workgroups));
  }

  // 6. streamed rebuild (after lds_hash_build and filter_local_map are known).  (measured, scans/s aggregate, streamed /
  //    three-kernel rebuild: 4 streams 27.6k / 27.3k, 8 streams 40.4k / 41.1k, 12 streams 47.3k / 51.3k — with many streams the
  //    waiting workgroups of one stream hold the CUs the next stream's solve needs)
  p.early_rebuild = (!p.lds_hash_build && !p.filter_local_map && !params->mapping && S <= 4 && env.early_rebuild) ? 1 : 0;

  // 7. LIODOM_SAFE_MODE=1, HERE: in front of every size that early_rebuild shapes (table_size, used_cap, ovf_base, sorted_cap) and
  //    of the ring-split decisions, which test safe_mode.  A handle that enters safe mode at a later liodom_reset keeps the
  //    sizes of the plan without it.
  if (env.safe_mode) plan_enter_safe_mode(&p);

  // 8. window, received map and cell hash
  p.recv_cap = p.mapping ? (config->recv_capacity > 0 ? config->recv_capacity : 262144) : 0;
  const long long map_cap = (long long)p.edge_cap * P + p.recv_cap;
  const long long pad = p.early_rebuild ? 8LL * p.edge_cap : 0;      // (early rebuild: cells that only the padding touches)
  long long ts = 1024;
  while (ts < 2 * (map_cap + pad)) ts <<= 1;
  // k_hash_build publishes its LDS table into slots [0, kLdsSlots) of the stream's table (keys, occupancy bits, cell_cap), however
  // small the window: a lock-step handle with fewer than 2048 window points wrote into the next stream's table and past the last one
  if (p.lds_hash_build && ts < kLdsSlots) ts = kLdsSlots;
  const long long used_cap = map_cap + pad;
  const long long ovf_base = map_cap + pad;
  long long sorted_cap = p.early_rebuild ? ovf_base + p.edge_cap : map_cap;
  // incremental cell hash (k_hash_append): every cell keeps room for the points of the frames that arrive before the next
  // rebuild — twice the window + 64k places per stream (+ the spill list).  Sized HERE, before the kNN instance is known; step
  // 11 decides hash_incr from knn8 AND from this size, so a handle that ends up without k_knn8 keeps the larger array.
  const bool incr_sized = env.hash_incr && p.lockstep && p.lds_hash_build && !params->mapping && !params->filter_local_map && !p.early_rebuild;
  if (incr_sized) sorted_cap = 2 * map_cap + 65536 + (long long)(kHbPeriod - 1) * p.edge_cap;

  // 9. the scan's buffers
  p.debug = config->debug_buffers & 1;
  // in-kernel phase timestamps (tools/gpu_debug.py clocks): they change no result.  Instrumented builds only
  // (-DLIODOM_INSTRUMENT, tools/variant_build.sh): 1: stamps, 65: + histograms (shared-counter atomics: they perturb the timing)
  if (caps.instrumented && env.debug_clocks != 0) {
    const int dc = env.debug_clocks;
    p.debug |= ((dc & (128 | 256)) ? (dc & 32) : 32) | (dc & (64 | 128)) | (dc & ~255);
  }
  const long long ring_id_stride = round_up((long long)config->max_points + 512, 256);
  p.tile_cap = (int)std::max(1LL, cdiv(config->max_points, kTilePts));
  p.split_pad = (int)round_up(p.tile_cap, 8);
  p.lb_hpad = (int)round_up(H, 64);
  // k_ring_split_lb (lock-step batches of Velodyne-type clouds): rings at a fixed pitch of 9/8 of the nominal ring length.
  // (tests safe_mode: behind step 7.)  liodom_create clears it when the kernel cannot have its LDS; the pitched buffers, sized
  // here from the planned value, stay.
  p.ring_split_lb = p.lockstep && params->lidar_type == 0 && !p.safe_mode && env.ring_split_lb;
  const long long ring_pitch = env.ring_pitch ? env.ring_pitch : round_up(cdiv((long long)config->max_points * 9, (long long)H * 8), 8);

  // capacities beyond the ints of DevView (the arithmetic above is 64-bit; in 32 bits it would have overflowed)
  if (ts > (1LL << 30) || map_cap > INT_MAX || used_cap > INT_MAX || sorted_cap > INT_MAX || ring_id_stride > INT_MAX || ring_pitch > INT_MAX) {
    *error = "liodom_create: capacities (window, received map, points per scan) exceed 32-bit sizes";
    return LIODOM_ERR_CAPACITY;
  }
  p.map_cap = (int)map_cap; p.table_size = (int)ts;
  p.used_cap = (int)used_cap; p.ovf_base = (int)ovf_base; p.sorted_cap = (int)sorted_cap;
  p.ring_id_stride = (size_t)ring_id_stride;
  p.ring_pitch = (int)ring_pitch;
  p.ring_stride = p.ring_split_lb ? std::max((size_t)config->max_points, (size_t)H * (size_t)p.ring_pitch) : (size_t)config->max_points;

  // 10. k_ring_split's tiles wait for each other inside the launch, so EVERY workgroup of a launch must be resident at once.  How
  //     many fit is a property of the device (CUs, LDS per CU: a tile holds ~50 KB), not a constant: occupancy x CU count, half
  //     of it left to the odometry chain's kernels that run beside the extraction.  Launches above the budget — and devices or
  //     partitions where a single scan's tiles do not fit (CPX partitions, CU-masked runs) — take k_classify + k_ring_scatter.
  //     (safe mode = no in-kernel waits at all: it overrides the switch, whatever the order of the variables)
  p.ring_split = env.ring_split && !p.safe_mode;
  if (p.ring_split) {
    long long budget = (long long)std::max(0, caps.ring_split_wgs_per_cu) * std::max(0, caps.cus) / 2;
    if (budget > 256) budget = 256;      // (measured: above ~4 HDL-64 streams per launch the waiting tiles lose to the two-kernel split anyway)
    p.ring_split_max_wgs = (int)budget;
    if (p.tile_cap > p.ring_split_max_wgs) p.ring_split = false;      // not even one stream's scan fits: never use it
  }

  // 11. kNN instance, then the incremental cell hash for good: lock-step batches that search with k_knn8 (it skips evicted
  //     points) on the LDS-built table, window only, windows of more frames than a period (the evicted frames are frames the
  //     rebuild knew) — and only where step 8 sized sorted_pts for it.
  p.knn8 = p.lockstep && env.knn8;
  p.knn8_grid = (int)std::max(1LL, cdiv(cdiv(p.edge_cap, kKnn8Queries), kKnnGridDiv));
  p.hash_incr = (env.hash_incr && p.knn8 && p.lds_hash_build && !params->mapping && !params->filter_local_map && P > kHbPeriod &&
                 sorted_cap >= 2 * map_cap + (long long)(kHbPeriod - 1) * p.edge_cap) ? 1 : 0;
  p.hb_spill_base = p.sorted_cap - (kHbPeriod - 1) * p.edge_cap;
  // knn_queries is the number of queries per workgroup of the k_knn instance launch_odometry picks from `lockstep`
  // (k_knn<128> / k_knn<256>; k_knn8 leaves k_line_gate the same layout): both sides read the one flag.
  p.knn_queries = p.lockstep ? 4 : 8;
  p.knn_partials = p.lockstep ? 0 : 1;         // measured: +37 % on the VALU-bound 256-stream kNN pass, -2 us per solve on one stream
  p.knn_blocks = (int)round_up(cdiv(p.edge_cap, p.knn_queries), 4);
  p.knn_grid = (int)std::max(1LL, cdiv(p.knn_blocks, kKnnGridDiv));   // sized for the usual edge count (~1/3 of the capacity): a workgroup takes a second block if there are more
  // (the two passes' validity bytes never share a 128-byte line: the overlapped second pass writes its half while the finalising
  //  solve's launch — which must not read it before ov_wait_knn_done — may hold the first pass's half in its caches)
  p.mask_stride = (int)round_up(p.knn_blocks, 128);

  // 12. Overlapped second kNN pass: its workgroups wait inside the kernel for the first solve, so they must leave most of the GPU
  //     to the launches they wait for (and to the next scan's extraction): one stream, at most a third of the wave slots
  //     (HDL-64: 352 workgroups x 4 waves = 1 408 of 6 144).  (measured with half of the slots allowed: Ouster-128, 704
  //     workgroups = 2 816 waves, loses — 9.0k -> 8.4k scans/s)
  p.ov_ok = env.knn_overlap != 0 && p.early_rebuild && S == 1 && p.knn_partials &&
            (env.knn_overlap == 2 || (long long)p.knn_grid * 4 * 3 <= (long long)caps.cus * 24);
  //     chain mode (kernels_sync.h): one-stream handles with the streamed rebuild whose passes leave at least half of the wave slots
  //     free; the IMU override rewrites the prediction between two scans on the odometry stream (k_imu_override), which the first
  //     pass on stream_k would not be ordered behind
  p.chain_ok = p.early_rebuild && S == 1 && p.knn_partials && !p.use_imu && (long long)p.knn_grid * 4 * 2 <= (long long)caps.cus * 24 &&
               env.knn_overlap != 0 && env.chain;
  //     speculative hand-over of the solves' results (kernels_sync.h), where either of the two exists
  p.speculate = (p.ov_ok || p.chain_ok) ? env.speculate : 0;
  p.spec_backoff = 16;
  p.spec_theta = env.spec_theta;

  *out = p;
  return LIODOM_OK;
}

// The handle's part of the decision to overlap the second kNN pass (ov) and to run a scan in chain mode (chain): the streamed
// rebuild, flags between the streams, and the GPU to this handle alone (`alone`: no second live handle in the process) — its
// waiting workgroups and those of a second handle could end up behind each other in a shared hardware queue.
struct OverlapModes { bool ov, chain; };
inline OverlapModes plan_overlap_modes(const HandlePlan& p, bool alone) {
  const bool base = p.early_rebuild && p.use_flags && alone;
  return {base && p.ov_ok, base && p.chain_ok && !p.flag_gate};
}

// What liodom_get_modes adds to the plan: counters of the scans since the last reset and the state around the handle.
struct ModesRuntime {
  bool alone = true;                 // no second live handle in the process
  bool streams_concurrent = true;    // liodom_create's probe
  int hb_stats[4] = {0, 0, 0, 0}, spec_stats[4] = {0, 0, 0, 0};
  unsigned int chain_count = 0, done0 = 0, done1 = 0;
  double replay_enqueue_us = 0.0, replay_wait_us = 0.0;
  int n_lagged = 0, n_readers = 0, n_hits = 0;
  long long subset_steps = 0;
};

// The text of liodom_get_modes.
inline void plan_format_modes(const HandlePlan& p, const ModesRuntime& r, char* buf, int cap) {
  const OverlapModes om = plan_overlap_modes(p, r.alone);
  snprintf(buf, (size_t)cap,
           "n_streams=%d early_rebuild=%d hash_build=%s pipe_flags=%d flag_gate=%d lm_groups=%d knn_instance=%d knn_queries=%d "
           "knn_grid=%d/%d knn8=%d hash_incr=%d hash_rebuilds=%d hash_appends=%d hash_appends_spilled=%d hash_points_spilled=%d knn_partials=%d knn_saved_bound=%d knn_exact_only=%d line_gate_kernel=%d filter_local_map=%d mapping=%d "
           "rotation_mode=%d table_size=%d sorted_cap=%d hb_spill_base=%d rebuild_delta=%.3f knn_overlap=%d streams_concurrent=%d safe_mode=%d ring_split=%d ring_split_max_wgs=%d ring_split_lb=%d chain=%d speculate=%d spec_early=%d/%d spec_unconfirmed=%d/%d chain_done=%u/%u/%u replay_enqueue_us=%.2f replay_wait_us=%.2f debug=%d",
           p.n_streams, p.early_rebuild, p.early_rebuild ? "streamed" : (p.lds_hash_build ? "lds" : "global"), p.use_flags ? 1 : 0,
           (p.use_flags && p.flag_gate) ? 1 : 0, p.lm_groups, p.lockstep ? 128 : 256, p.knn_queries, p.knn_grid,
           p.knn_blocks, p.knn8 ? 1 : 0, p.hash_incr, r.hb_stats[0], r.hb_stats[1], r.hb_stats[2], r.hb_stats[3], p.knn_partials,
           p.knn_save >= 2 ? 2 : (p.knn_save >= 1 ? 1 : 0), p.knn_exact_only, p.lockstep ? 1 : 0, p.filter_local_map, p.mapping,
           p.rotation_mode, p.table_size, p.sorted_cap, p.hb_spill_base, (double)p.rebuild_delta,
           (om.ov || om.chain) ? 1 : 0, r.streams_concurrent ? 1 : 0, p.safe_mode ? 1 : 0, p.ring_split ? 1 : 0, p.ring_split ? p.ring_split_max_wgs : 0, p.ring_split_lb ? 1 : 0,
           om.chain ? 1 : 0, p.speculate, r.spec_stats[0], r.spec_stats[2], r.spec_stats[1], r.spec_stats[3], r.chain_count, r.done0, r.done1,
           r.replay_enqueue_us, r.replay_wait_us, p.debug);
  auto tail = [&](size_t* room) { const size_t n = std::strlen(buf); *room = (size_t)cap - n; return buf + n; };
  size_t room = 0;
  if (p.pose_covariance) { char* t = tail(&room); snprintf(t, room, " pose_cov=1"); }
  if (r.n_lagged > 0) { char* t = tail(&room); snprintf(t, room, " mapper_lag=%d", r.n_lagged); }      // streams with a lagged mapper (liodom_attach_mapper_ex); their steps run on the odometry stream alone, as every mapping handle's
  if (r.n_readers > 0) { char* t = tail(&room); snprintf(t, room, " map_readers=%d map_rows=%d", r.n_readers, p.map_rows ? 1 : 0); }     // streams that read a map they never write (liodom_attach_map_reader)
  if (r.n_hits > 0) { char* t = tail(&room); snprintf(t, room, " map_hits=%d", r.n_hits); }      // streams with per-scan hit records on (liodom_set_map_hits)
  { char* t = tail(&room); snprintf(t, room, " subset_steps=%lld", r.subset_steps); }      // (steps liodom_process_resident_subset ran over a stream list, i.e. did not hand to the plain step)
}

}  // namespace liodom_dev
