// liodom_sizes.h — the numbers the host's plans (of a handle: handle_plan.h; of a scan's launches: step_plan.h) and the kernels must
// agree on: tile, window and buffer constants, the launch constants (workgroup sizes, workgroups per role) and the dynamic-LDS size of
// every kernel that takes one.  Plain C++ without a HIP include: hipcc takes it through the
// kernel headers, g++ through handle_plan.h.  Each constant sits with the comment of the kernel it belongs to; the kernels
// themselves are in the kernels_*.h file named beside it.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define LS_HD __host__ __device__ __forceinline__
#else
#define LS_HD inline
#endif

namespace liodom_dev {

// ---- liodom_kernels.h ----
// Solving workgroups of 4 waves (round 6; 8 until then): one wave per SIMD with the whole register file to itself — no scratch in
// any instance of k_lm_solve (512 threads: 256 registers per lane and 108-172 B of scratch in the controller's path), half as many
// waves at every barrier.  Interleaved A/B against 512 (same box, bench.py): `value` 14 288 -> 14 577 (K = 200), 13 364 -> 13 503
// (the driver's K = 20), strict-sync +0.9 %, 256 lock-step streams 203.8k -> 207.1k; round 5 had measured +-1 % for the same switch
// (then one instance of the kernel per solve, now one per solve and mode).
#ifndef LIODOM_LM_THREADS
#define LIODOM_LM_THREADS 256
#endif
constexpr int kLmThreads = LIODOM_LM_THREADS;   // k_lm_solve: 4 waves, one per SIMD, all evaluate residual blocks
#ifndef LIODOM_LM_GROUPS_MAX
#define LIODOM_LM_GROUPS_MAX 8
#endif
constexpr int kLmGroupsMax = LIODOM_LM_GROUPS_MAX;
constexpr int kMaxFrames = 256;          // window frames supported by the LDS prefix tables
constexpr int kEdgeBufs = 4;             // dense edge buffers: 0 / 1 / 2 odometry side (pipelined replay), 3 extraction side
constexpr int kEdgePipeBufs = 3;

// ---- kernels_extract.h: k_classify / k_ring_scatter / k_ring_split / k_ring_split_lb ----
constexpr int kTilePts = 2048;
constexpr int kTileChunks = kTilePts / 64;   // 32
constexpr int kTileThreads = 512;            // workgroup of the four ring-split kernels
constexpr int kRowThreads = 512;             // k_row_compact: one workgroup per (row, stream)

LS_HD int ring_scatter_stride(int H) { return H | 1; }
// LDS: phase A = lane masks [32][Hp] u64 + chunk prefixes [32][Hp] u16; phase B reuses the same
// bytes as the staging tile {float4 point, int dst, int src} x 2048; then rbase / lofs / wtot.
LS_HD size_t ring_scatter_stage_bytes(int H) {
  const int Hp = ring_scatter_stride(H);
  const size_t a = (size_t)kTileChunks * Hp * 8 + (size_t)((kTileChunks * Hp * 2 + 15) & ~15);
  const size_t b = (size_t)kTilePts * 24;
  return a > b ? a : b;
}
LS_HD size_t ring_scatter_lds_bytes(int H) {
  return ring_scatter_stage_bytes(H) + (size_t)(2 * H + 2 * 16) * 4;
}
LS_HD size_t ring_split_lb_lds_bytes(int H) {      // + rlim [H]
  return ring_scatter_stage_bytes(H) + (size_t)(3 * H + 16) * 4;
}

// ---- kernels_extract.h: k_ring_extract ----
constexpr int kExLPR = 16;               // lanes per region (one DPP row)
constexpr int kExIPL = 16;               // items per lane -> regions of up to 256 items ...
constexpr int kExIPLBig = 24;            // ... or 384 (the last region takes the remainder of the split: Ouster 2048 / 8 -> 260); the host
                                         // picks the instance from the expected ring width, longer regions take the generic path
constexpr int kGapBitsCap = 16384;       // points per ring covered by the LDS continuity bits (2 KB)
constexpr int kExMaxRegions = 64;

LS_HD int ring_extract_threads(int regions) {
  const int waves = (regions + 3) / 4;
  return 64 * (waves < 1 ? 1 : (waves > 16 ? 16 : waves));
}
LS_HD size_t ring_extract_lds_bytes(int slots, int regions) {
  size_t b = (size_t)(kGapBitsCap / 32 + 4) * 4;          // continuity bits + pad words
  b += (size_t)slots * 4;                                 // pick_idx
  b += (size_t)((slots + 15) / 16 * 16);                  // pick_nfnb
  b += (size_t)regions * 4 + 2 * kExMaxRegions * 4 + 64;  // region_cnt, masks, flags
  return (b + 15) / 16 * 16;
}

// ---- kernels_compact.h ----
constexpr int kCompactBlocks = 8;      // k_compact_edges: grid (kCompactBlocks, streams); every workgroup scans the ring counts itself and copies its interleaved share

// ---- kernels_knn.h / kernels_knn8.h ----
constexpr int kKnnGridDiv = 2;         // k_knn grid = half of the query blocks the edge capacity allows: a workgroup takes block b and, if the scan has that many edges, b + grid
constexpr int kG8 = 8;                    // lanes per query
#ifndef LIODOM_KNN8_THREADS
#define LIODOM_KNN8_THREADS 256
#endif
constexpr int kKnn8Threads = LIODOM_KNN8_THREADS;      // 4 waves = 32 queries per workgroup (512 threads: the sort below balances better, but the workgroups pack worse — 373 us against 334 for a first pass at 256 streams)
constexpr int kKnn8Queries = kKnn8Threads / kG8;
constexpr int kKnn8ExactBlocks = 4;    // k_knn8_exact: workgroups per stream that walk the list of queries the fast path cannot certify (one wave per query)

// ---- kernels_lm.h ----
// dynamic LDS of k_lm_solve: the index list (the reduction's per-wave sums, sh_wsum, are static: 1 KiB)
LS_HD size_t lm_lds_bytes(int edge_cap) {
  return (size_t)((edge_cap + 3) & ~3) * sizeof(int);
}

// ---- kernels_rebuild.h: the streamed rebuild ----
constexpr int kRebuildAuxBlocks = 8;      // workgroups for ALLOC (inside k_knn) and for CLEAR (k_lm_solve)
constexpr int kRebuildAllocBlocks = 32;   // k_rebuild_alloc: the ~8 000 occupied cells of a headline scan in one sweep (it sits between the two solve launches)
#ifndef LIODOM_REBFIN_THREADS
#define LIODOM_REBFIN_THREADS LIODOM_LM_THREADS
#endif
constexpr int kRebFinThreads = LIODOM_REBFIN_THREADS;      // k_rebuild_fin (chain mode: APPEND, CLEAR, SCATTER as a launch of their own)

// ---- kernels_rebuild.h: k_hash_build, k_hash_append ----
constexpr int kBuildThreads = 1024;
constexpr int kLdsSlots = 8192;
constexpr int kLdsCellsMax = 6144;
LS_HD size_t hash_build_lds_bytes() { return (size_t)kLdsSlots * 16 + 64; }
#ifndef LIODOM_HB_PERIOD
#define LIODOM_HB_PERIOD 4
#endif
constexpr int kHbPeriod = LIODOM_HB_PERIOD;       // scans between two rebuilds from the whole window (<= 8: hb_base)
constexpr int kHbNewRoom = 96;     // room of a cell that k_hash_append creates (DevView::hb_new_room; kHbSlackMin = 32: hb_slack_min)
constexpr int kHbSlackMin = 32;

// ---- liodom_map.h: k_map_local_rows ----
constexpr int kMapRowsThreads = 256;

// ---- kernels_graph.h: k_graph_pcg_columns ----
// Bytes of workspace an automatic plan of the covariance calls gives one launch (graph_marginals.h): 30 node_cap doubles per
// column, so 1092 columns of a 1024-node graph, 17 at the full 65 536 nodes — and never fewer than 6.
constexpr size_t kGraphCovWorkspaceBudget = (size_t)256 << 20;

}  // namespace liodom_dev
