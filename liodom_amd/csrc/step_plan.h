// step_plan.h — what one scan launches, decided before anything is enqueued: the state that runs from scan to scan (StepState), what
// an entry point asks for (StepRequest, ExtractRequest) and the ordered list of the step's launches with their grids (StepPlan),
// filled by pure functions.  Plain C++17 without a HIP include, no getenv, no allocation per step: the grid sums that must match
// the workgroup roles a kernel decodes from blockIdx.x, and the switches between the overlapped pass, chain mode and the plain four
// launches, run under g++ and host sanitizers (tests/step_plan_main.cc, tests/test_step_plan.py).  liodom_step_host.h fills a
// request, calls the plan function and issues what the list says.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "handle_plan.h"
#include "liodom_sizes.h"

namespace liodom_dev {

// Per-kernel profiling buckets (liodom_get_kernel_stats).
enum KernelId {
  KID_CLASSIFY = 0, KID_RING_EXTRACT, KID_COMPACT, KID_KNN, KID_LM, KID_HASH_CLEAR,
  KID_WINDOW_INSERT, KID_HASH_ALLOC, KID_HASH_SCATTER, KID_RING_SCATTER, KID_HASH_BUILD, KID_OTHER
};

// One value per kernel instance a step launches; an instance that exists for rows = streams s0 + row and for rows = entries of a
// stream list (stream_of) is one value, StepLaunch::list picks between the two.  The SO_* values are host-side operations.
enum StepKernel : uint8_t {
  // extraction
  SK_ROW_COMPACT, SK_RING_SPLIT_LB, SK_RING_SPLIT_FIX, SK_RING_SPLIT, SK_CLASSIFY, SK_RING_SCATTER,
  SK_RING_EXTRACT_256, SK_RING_EXTRACT_256_BIG, SK_RING_EXTRACT_1024, SK_RING_EXTRACT_1024_BIG, SK_COMPACT_EDGES,
  // odometry
  SK_IMU_OVERRIDE, SK_WINDOW_STASH,
  SK_KNN_CHAIN_FIRST,      // k_knn<256, false, true>: chain mode's first pass
  SK_CHAIN_REDO0, SK_LM0_CHAIN, SK_LM1_CHAIN, SK_OV_GATE,
  SK_KNN_OV,               // k_knn<256, true>: the overlapped second pass
  SK_KNN_REDO, SK_REBUILD_ALLOC, SK_REBUILD_FIN,
  SK_POSE_COV_CHAIN,       // k_pose_cov<> as chain mode names it (on its own: the code object keeps its kernel order, liodom_step_host.h)
  SK_POSE_COV,
  SK_KNN8_0, SK_KNN8_1, SK_KNN8_EXACT, SK_LINE_GATE, SK_KNN128, SK_KNN256, SK_LM0, SK_LM1,
  SK_HASH_APPEND, SK_HASH_BUILD, SK_WINDOW_INSERT, SK_HASH_ALLOC, SK_HASH_SCATTER,
  SK_VOXEL_BBOX, SK_VOXEL_INSERT, SK_VOXEL_ALLOC, SK_VOXEL_SCATTER, SK_VOXEL_CENTROID, SK_FILT_INSERT, SK_FILT_ALLOC, SK_FILT_SCATTER,
  SK_KERNELS,
  SO_EV_OV = SK_KERNELS,   // record ev_ov on the odometry stream, stream_k waits for it
  SO_EV_CH,                // record ev_ch on stream_k, the odometry stream waits for it (behind the chain flush's launch, if any)
  SO_MAP_BLOCK             // the mapper / map-reader block of a mapping handle (liodom_step_host.h)
};

enum StepQueue : uint8_t { SQ_ODO, SQ_K, SQ_X };      // the odometry stream, stream_k, the queue an extraction was given
enum StepScope : uint8_t { SS_NONE, SS_OPEN, SS_SAME };   // per-kernel profiling: no event pair / a new one of `bucket` / the previous launch's

struct StepLaunch {
  StepKernel k;
  StepQueue q;
  StepScope scope;
  uint8_t bucket;          // KID_*
  bool list;
  int gx, gy, block;
  size_t lds;              // dynamic LDS bytes
  // the scalar arguments that are decisions, not data (each kernel takes the ones it has)
  int pass, scan_no, nA, with_pass, with_fix, alloc, tiles;
  unsigned int seq_k, done_target, wait_edges, signal_odo, lb_tag;
};

// The longest plan is a filtering handle's under profiling (IMU override, two passes of three launches and a solve, covariance, the
// three-kernel rebuild, eight filter launches: 22) — chain mode has 9 launches and 3 operations; 8 entries of margin.
constexpr int kStepPlanCap = 32;
struct StepPlan {
  StepLaunch e[kStepPlanCap];
  int n = 0;
  bool overflow = false;   // (never on any handle: tests/test_step_plan.py)
  StepLaunch& add(StepKernel k, StepQueue q, int gx, int gy, int block, size_t lds = 0, StepScope scope = SS_NONE, int bucket = KID_OTHER) {
    if (n == kStepPlanCap) { overflow = true; n--; }
    StepLaunch& l = e[n++];
    l = StepLaunch{};
    l.k = k; l.q = q; l.scope = scope; l.bucket = (uint8_t)bucket; l.gx = gx; l.gy = gy; l.block = block; l.lds = lds;
    return l;
  }
};

// ---- the odometry side's state from scan to scan (under mx_o) ----
constexpr int kOvWarmScans = 2;
struct StepState {
  int ov_warm = 0;                   // scans enqueued so far, up to kOvWarmScans (the first ones run every kernel of the chain for the first time)
  bool ov_prev = false;              // the previous scan was overlapped
  // Not reset: ov_flags[s] and the sequence words of pred_xch keep the number of the last overlapped scan (ov_flags is never cleared, and
  // a waiter compares for "reached seq"): a sequence that started over would find its first numbers already there.  0 means "not overlapped".
  unsigned int ov_seq = 0;
  bool chain_prev = false;           // the previous scan was enqueued in chain mode
  unsigned int chain_count = 0;      // first-pass workgroups launched in chain mode since the last reset (what knn_done0, cleared with it, counts up to)
  bool chain_fix_pending = false;    // the last chain-mode scan's APPEND may need the repair of k_chain_redo0 (speculative hand-over)
  // Not reset: it says that stream_k has carried odometry work of this handle, so the side's results are complete only when stream
  // AND stream_k have drained (sync_odometry); a reset does not take that back, it only leaves the stream idle.
  bool chain_used = false;
  int verdict_scan = -1;             // scans completed when the host last collected stream 0's pose, and whether that scan's speculative
  bool verdict_confirmed = false;    // hand-over was confirmed (HostOut::pad)
  std::vector<int> hb_since;         // hash_incr, per stream: scans since the stream's last k_hash_build (-1: none yet); sized once, by bind

  void bind(int n_streams) { hb_since.assign((size_t)n_streams, -1); }
  // The first scans after a reset (or of an imported one-stream state) are not overlapped, as after liodom_create: the first one
  // runs with st.initialized == 0, where no first solve publishes the pose an overlapped second kNN pass would wait for.
  void restart_overlap() { ov_warm = 0; ov_prev = false; chain_prev = false; chain_count = 0; chain_fix_pending = false; verdict_scan = -1; }
  void reset() { restart_overlap(); std::fill(hb_since.begin(), hb_since.end(), -1); }
};

// The extraction side's (under mx_x).  Not reset: the count words of k_ring_split_lb carry the tag of the launch that wrote them
// and are not cleared, so the tag goes on counting; 0 is never a tag.
struct ExtractState { unsigned int lb_tag = 0; };

struct StepRequest {
  int s0 = 0, count = 1;             // streams s0 .. s0 + count - 1; s0 < 0: the `count` streams of device-side list -s0 - 1 ...
  const int32_t* list = nullptr;     // ... whose entries the host reads here (the caller's array)
  unsigned int wait_edges = 0, signal_odo = 0;      // wait_edges != 0: the edges arrive from the extraction stream by flag
  bool profiling = false, ov_suppress = false, alone = true;
  int scans_enqueued = 0;            // of the first stream
  bool lagged = false;               // a stream of the step has a lagged mapper
  int stream_at(int i) const { return list ? (int)list[i] : s0 + i; }
};

struct ExtractRequest {
  int count = 1;
  bool list = false;
  int n = 0, width = 0;              // points per scan, columns of an organised cloud
  int max_width = 0;                 // liodom_config_t::max_width
};

namespace plan_detail {
inline int icdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
}

// The repair of a chain-mode APPEND that started from a pose the solve did not end with rides behind the NEXT scan's first pass
// (k_chain_redo0).  When no such pass follows — the handle leaves chain mode, or the host is about to read the odometry side's
// results — it is launched on its own (it waits for the scan's verdict; normally it finds nothing to do), unless the scan's pose
// has been collected and its record says "confirmed".  Appends to the plan.
inline void plan_chain_flush(const HandlePlan& p, StepState* st, int scans_enqueued0, StepPlan* out) {
  if (!st->chain_fix_pending) return;
  st->chain_fix_pending = false;
  if (st->verdict_scan == scans_enqueued0 && st->verdict_confirmed) return;
  const int nA = (p.edge_cap + 255) / 256;
  StepLaunch& l = out->add(SK_CHAIN_REDO0, SQ_K, nA, 1, 256);
  l.scan_no = scans_enqueued0; l.nA = nA; l.with_pass = 0; l.with_fix = 1;
}

// Window append and cell hash behind the solves (handles without the streamed rebuild), then the voxel filter.
inline void plan_hash_step(const HandlePlan& p, bool rebuild, bool list, int count, bool scoped, StepPlan* out) {
  const int map_blocks = plan_detail::icdiv(p.map_cap, 256);
  const StepScope open = scoped ? SS_OPEN : SS_NONE;
  if (p.lds_hash_build) {
    if (!rebuild) out->add(SK_HASH_APPEND, SQ_ODO, count, 1, kBuildThreads, 0, open, KID_HASH_BUILD).list = list;
    else out->add(SK_HASH_BUILD, SQ_ODO, count, 1, kBuildThreads, hash_build_lds_bytes(), open, KID_HASH_BUILD).list = list;
  } else {
    out->add(SK_WINDOW_INSERT, SQ_ODO, map_blocks, count, 256, 0, open, KID_WINDOW_INSERT).list = list;
    out->add(SK_HASH_ALLOC, SQ_ODO, map_blocks, count, 256, 0, open, KID_HASH_ALLOC).list = list;
    out->add(SK_HASH_SCATTER, SQ_ODO, map_blocks, count, 256, 0, open, KID_HASH_SCATTER).list = list;
  }
}
inline void plan_filter_step(const HandlePlan& p, bool list, int count, bool scoped, StepPlan* out) {
  if (!p.filter_local_map) return;      // VoxelGrid(0.4) of the full window (every kernel exits unless the window is full)
  const int map_blocks = plan_detail::icdiv(p.map_cap, 256);
  const StepScope open = scoped ? SS_OPEN : SS_NONE, same = scoped ? SS_SAME : SS_NONE;
  out->add(SK_VOXEL_BBOX, SQ_ODO, count, 1, 1024, 0, open, KID_OTHER).list = list;
  out->add(SK_VOXEL_INSERT, SQ_ODO, map_blocks, count, 256, 0, same, KID_OTHER).list = list;
  out->add(SK_VOXEL_ALLOC, SQ_ODO, map_blocks, count, 256, 0, same, KID_OTHER).list = list;
  out->add(SK_VOXEL_SCATTER, SQ_ODO, map_blocks, count, 256, 0, same, KID_OTHER).list = list;
  out->add(SK_VOXEL_CENTROID, SQ_ODO, plan_detail::icdiv(p.map_cap, 8), count, 256, 0, same, KID_OTHER).list = list;
  out->add(SK_FILT_INSERT, SQ_ODO, map_blocks, count, 256, 0, same, KID_OTHER).list = list;
  out->add(SK_FILT_ALLOC, SQ_ODO, map_blocks, count, 256, 0, open, KID_HASH_ALLOC).list = list;
  out->add(SK_FILT_SCATTER, SQ_ODO, map_blocks, count, 256, 0, open, KID_HASH_SCATTER).list = list;
}
// The search structure of one stream rebuilt from its whole window without appending a frame (an imported or seeded state, a new
// received map): the hash step of a scan as a rebuild, then the filter.
inline void plan_full_rebuild(const HandlePlan& p, StepPlan* out) {
  out->n = 0;
  plan_hash_step(p, true, false, 1, false, out);
  plan_filter_step(p, false, 1, false, out);
}

// The odometry of `count` streams on the dense edges already on the device.
inline void plan_odometry_step(const HandlePlan& p, StepState* st, const StepRequest& rq, StepPlan* out) {
  using plan_detail::icdiv;
  out->n = 0;
  const int count = rq.count;
  const bool list = rq.s0 < 0;
  const bool knn_small = p.lockstep;           // 4 queries per workgroup, else 8
  const int P = p.prev_frames;
  if (p.use_imu) out->add(SK_IMU_OVERRIDE, SQ_ODO, icdiv(count, 64), 1, 64, 0, SS_OPEN, KID_OTHER).list = list;
  // Lagged mappers: the frame this scan's append will overwrite is set aside before anything of the step runs (one launch for
  // the step's streams; k_window_stash skips those without a lagged mapper).  A mapping handle runs neither the streamed
  // rebuild nor chain mode nor the overlapped pass (early_rebuild = 0): the previous scan's append, this launch, the solves, the
  // map update and this scan's append are all on the odometry stream, in this order.
  if (rq.lagged) out->add(SK_WINDOW_STASH, SQ_ODO, std::min(16, icdiv(p.edge_cap, 256)), count, 256, 0, SS_OPEN, KID_OTHER).list = list;
  // early rebuild ("streamed rebuild", kernels_rebuild.h): the four launches of a scan carry extra workgroups that build
  // the next scan's cell hash in the second table; nothing follows the finalising solve
  const bool early = p.early_rebuild != 0;
  const int nC = icdiv((long long)p.edge_cap * std::max(1, P - 1), kLmThreads), nP = icdiv(p.edge_cap, kLmThreads);
  // Overlapped second kNN pass (kernels_sync.h): the pass goes to stream_k behind the first solve's launch and waits inside
  // the kernel; it needs kernels of different streams to run side by side (as the flags of the pipelined replay do) and the
  // GPU mostly to itself (plan_overlap_modes), and is not used under per-kernel profiling.
  // (chain mode — only for scans whose edges come from the extraction stream by flag, see below — also overlaps the pass on shapes
  //  where the four-launch chain cannot: Ouster-128's 704 waiting workgroups beside full-CU rebuild workgroups cost 9 %, in chain
  //  mode the overlapped pass gains 19 % there)
  const OverlapModes om = plan_overlap_modes(p, rq.alone);
  const bool chain_cand = om.chain && rq.wait_edges != 0u;
  const bool overlap_ok = (om.ov || chain_cand) && !rq.profiling && !rq.ov_suppress && count == 1;
  // The first scans of a handle are not overlapped: their launches are the first of every kernel of the chain on this queue
  // (scratch set-up, code upload), which can hold the odometry stream back for longer than a waiting kernel is willing to
  // poll.  At a switch to overlapped scans stream_k waits (event) for the odometry stream to have drained, so that its
  // first polling launch cannot start before everything it depends on has run once.
  const bool overlap = overlap_ok && st->ov_warm >= kOvWarmScans;
  if (st->ov_warm < kOvWarmScans) st->ov_warm++;
  unsigned int seq_k = 0u;                           // (0 means "not overlapped" to the kernels)
  if (overlap) {
    if (++st->ov_seq == 0u) st->ov_seq = 1u;
    seq_k = st->ov_seq;
    if (!st->ov_prev) out->add(SO_EV_OV, SQ_ODO, 0, 0, 0);
  }
  // Chain mode: only for scans whose edges come from the extraction stream by flag (the pipelined replay, the ticket API): the
  // first pass then runs on stream_k, where nothing orders it behind an extraction enqueued on the odometry stream itself.
  const bool chain = overlap && chain_cand;
  if (chain != st->chain_prev) {
    if (chain) {
      // (stream_k waits for the odometry stream: planned above unless the previous scan was overlapped without the chain)
      if (st->ov_prev) out->add(SO_EV_OV, SQ_ODO, 0, 0, 0);
    } else {
      plan_chain_flush(p, st, rq.scans_enqueued, out);
      out->add(SO_EV_CH, SQ_K, 0, 0, 0);
    }
  }
  st->chain_prev = chain;
  st->ov_prev = overlap;
  if (chain) {
    st->chain_used = true;
    const int scan_no = rq.scans_enqueued;
    st->chain_count += (unsigned int)p.knn_grid;                        // (wraps with the device counter: the kernels compare differences)
    const unsigned int done_target = st->chain_count;
    const int gx = (p.lm_groups - 1) * 8 + 1;                           // solvers on blocks 0, 8, 16, ... (one XCD); nothing else in the launch
    const size_t lds = lm_lds_bytes(p.edge_cap);
    // stream_k: first pass | gate (first solve's launch has started; + repair of the previous scan's hand-over: k_chain_redo0) | second pass + COUNT + PAD |
    //           ALLOC (+ repeat of unconfirmed second-pass workgroups: k_knn_redo) | APPEND + CLEAR + SCATTER
    // stream:   first solve (resident beside the first pass: waits for its done flags) | finalising solve (waits for the second pass's)
    const int nCP = icdiv((long long)p.edge_cap * std::max(1, P - 1), 256) + icdiv(p.edge_cap, 256);      // COUNT + PAD workgroups of 256 threads
    auto flags = [&](StepLaunch& l) { l.wait_edges = rq.wait_edges; l.signal_odo = rq.signal_odo; };
    auto scan = [&](StepLaunch& l) -> StepLaunch& { l.seq_k = seq_k; l.scan_no = scan_no; l.done_target = done_target; return l; };
    flags(scan(out->add(SK_KNN_CHAIN_FIRST, SQ_K, p.knn_grid, 1, 256)));
    if (p.speculate) {      // (speculative hand-over of the previous scan's result not confirmed: rare)
      const int nA = icdiv(p.edge_cap, 256);
      // (+ 1: the gate in front of the second pass, k_ov_gate's job otherwise)
      StepLaunch& l = scan(out->add(SK_CHAIN_REDO0, SQ_K, nA + p.knn_grid + 1, 1, 256));
      flags(l);
      l.nA = nA; l.with_pass = 1; l.with_fix = st->chain_fix_pending ? 1 : 0;
    }
    st->chain_fix_pending = p.speculate != 0;
    scan(out->add(SK_LM0_CHAIN, SQ_ODO, gx, 1, kLmThreads, lds));
    if (!p.speculate) scan(out->add(SK_OV_GATE, SQ_K, 1, 1, 64));
    scan(out->add(SK_KNN_OV, SQ_K, p.knn_grid + nCP, 1, 256)).pass = 1;
    // (speculative hand-over not confirmed — rare —: the pass's workgroups once more; the launch's first workgroups are ALLOC)
    if (p.speculate) scan(out->add(SK_KNN_REDO, SQ_K, kRebuildAllocBlocks + p.knn_grid, 1, 256)).alloc = kRebuildAllocBlocks;
    scan(out->add(SK_LM1_CHAIN, SQ_ODO, gx, 1, kLmThreads, lds));
    // (pose covariance: behind the finalising solve on its stream; the next scan's first solve follows it there, and the next second
    //  pass — hence the next finalising solve, the next writer of cov_raw — waits for that solve: kernels_cov.h)
    if (p.pose_covariance) out->add(SK_POSE_COV_CHAIN, SQ_ODO, count, 1, 64);
    if (!p.speculate) out->add(SK_REBUILD_ALLOC, SQ_K, kRebuildAllocBlocks, 1, 256);
    const int nCf = icdiv((long long)p.edge_cap * std::max(1, P - 1), kRebFinThreads), nPf = icdiv(p.edge_cap, kRebFinThreads);
    out->add(SK_REBUILD_FIN, SQ_K, nPf + kRebuildAuxBlocks + nCf, 1, kRebFinThreads);
    return;
  }
  for (int it = 0; it < 2; it++) {
    const int kx = p.knn_grid + ((early && it == 1 && !seq_k) ? kRebuildAuxBlocks : 0);     // it 1: + ALLOC (overlapped pass: k_rebuild_alloc below)
    auto knn = [&](StepLaunch& l) { l.list = list; l.pass = it; l.wait_edges = rq.wait_edges; l.signal_odo = rq.signal_odo; };
    const int gate_gx = icdiv((long long)p.knn_blocks * p.knn_queries, 256);
    if (knn_small && p.knn8) {
      // lock-step batches: eight lanes per query (kernels_knn8.h); the workgroups of a stream walk its blocks of 32 queries
      out->add(it == 0 ? SK_KNN8_0 : SK_KNN8_1, SQ_ODO, p.knn8_grid, count, kKnn8Threads, 0, SS_OPEN, KID_KNN).list = list;
      StepLaunch& x = out->add(SK_KNN8_EXACT, SQ_ODO, kKnn8ExactBlocks, count, kKnn8Threads, 0, SS_SAME, KID_KNN);      // (the ~1 % of the queries the fast path cannot certify)
      x.list = list; x.pass = it;
      StepLaunch& g = out->add(SK_LINE_GATE, SQ_ODO, gate_gx, count, 256, 0, SS_SAME, KID_KNN);
      g.list = list; g.pass = it;
    } else if (knn_small) {
      knn(out->add(SK_KNN128, SQ_ODO, kx, count, 128, 0, SS_OPEN, KID_KNN));
      StepLaunch& g = out->add(SK_LINE_GATE, SQ_ODO, gate_gx, count, 256, 0, SS_SAME, KID_KNN);
      g.list = list; g.pass = it;
    } else if (it == 1 && seq_k) {
      out->add(SK_OV_GATE, SQ_K, 1, 1, 64, 0, SS_OPEN, KID_KNN).seq_k = seq_k;
      StepLaunch& l = out->add(SK_KNN_OV, SQ_K, kx, count, 256, 0, SS_SAME, KID_KNN);
      l.pass = it; l.seq_k = seq_k; l.scan_no = -1;
      if (p.speculate) {      // (speculative hand-over not confirmed: rare)
        StepLaunch& r = out->add(SK_KNN_REDO, SQ_K, p.knn_grid, count, 256, 0, SS_SAME, KID_KNN);
        r.seq_k = seq_k; r.scan_no = -1; r.alloc = 0;
      }
      // ALLOC between the two solve launches, beside the pass's tail
      out->add(SK_REBUILD_ALLOC, SQ_ODO, kRebuildAllocBlocks, count, 256, 0, SS_SAME, KID_KNN);
    } else {
      knn(out->add(SK_KNN256, SQ_ODO, kx, count, 256, 0, SS_OPEN, KID_KNN));
    }
    // it 0: + COUNT, PAD; it 1: + APPEND, CLEAR, SCATTER
    const int extra = !early ? 0 : (it == 0 ? nC + nP : nP + kRebuildAuxBlocks + nC);
    const int gx = std::max(p.lm_groups + extra, (p.lm_groups - 1) * 8 + 1);      // solvers on blocks 0, 8, 16, ... (one XCD)
    StepLaunch& lm = out->add(it == 0 ? SK_LM0 : SK_LM1, SQ_ODO, gx, count, kLmThreads, lm_lds_bytes(p.edge_cap), SS_OPEN, KID_LM);
    lm.list = list; lm.seq_k = seq_k;
    // pose covariance of the scan, straight behind its finalising solve (kernels_cov.h)
    if (it == 1 && p.pose_covariance) out->add(SK_POSE_COV, SQ_ODO, count, 1, 64, 0, SS_OPEN, KID_OTHER).list = list;
  }
  if (p.mapping) out->add(SO_MAP_BLOCK, SQ_ODO, 0, 0, 0);
  if (!early) {      // (early: the next cell hash is complete when the finalising solve launch ends)
    // hash_incr: k_hash_build every kHbPeriod-th scan, k_hash_append — the new frame into the cells of the last rebuild — in between.
    // Per stream: a single-stream call or a subset step of a lock-step handle steps some of the streams only.  A launch over several
    // streams rebuilds them all if any one is due — a rebuild is always exact — so that lock-step batches keep every counter in step.
    bool rebuild = true;
    if (p.lds_hash_build) {
      rebuild = !p.hash_incr;
      for (int i = 0; i < count; i++) rebuild = rebuild || st->hb_since[(size_t)rq.stream_at(i)] < 0 || st->hb_since[(size_t)rq.stream_at(i)] >= kHbPeriod - 1;
      for (int i = 0; i < count; i++) { int& hb = st->hb_since[(size_t)rq.stream_at(i)]; hb = rebuild ? 0 : hb + 1; }
    }
    plan_hash_step(p, rebuild, list, count, true, out);
  }
  plan_filter_step(p, list, count, true, out);
}

// Feature extraction of `count` streams: ring split, k_ring_extract, k_compact_edges.
inline void plan_extract_step(const HandlePlan& p, ExtractState* xs, const ExtractRequest& rq, StepPlan* out) {
  using plan_detail::icdiv;
  out->n = 0;
  const int H = p.scan_lines, count = rq.count;
  const int tiles = std::max(1, icdiv(rq.n, kTilePts));
  auto row = [&](StepKernel k, int gx, int gy, int block, size_t lds, int bucket) -> StepLaunch& {
    StepLaunch& l = out->add(k, SQ_X, gx, gy, block, lds, SS_OPEN, bucket);
    l.list = rq.list; l.tiles = tiles;
    return l;
  };
  const bool fits = (long long)tiles * count <= p.ring_split_max_wgs && p.ring_split;      // (every workgroup resident at once: k_ring_split waits inside the launch)
  if (p.lidar_type == 1 && rq.width > 0 && (long long)H * rq.width <= (long long)p.max_points) {
    // organised cloud: ring = row, the split is a per-row compaction (no classify / scatter passes): one pass over the scan
    row(SK_ROW_COMPACT, H, count, kRowThreads, 0, KID_RING_SCATTER);
  } else if (p.ring_split_lb && !fits) {
    // lock-step batches: one pass, rings at a fixed pitch, tiles sum their predecessors' counts (booked as the scatter)
    if (++xs->lb_tag == 0u) xs->lb_tag = 1u;
    row(SK_RING_SPLIT_LB, tiles * count, 1, kTileThreads, ring_split_lb_lds_bytes(H), KID_RING_SCATTER).lb_tag = xs->lb_tag;
    row(SK_RING_SPLIT_FIX, 1, count, kTileThreads, ring_split_lb_lds_bytes(H), KID_RING_SCATTER).scope = SS_SAME;
  } else if (fits) {
    // one pass: classification and scatter in one kernel (booked as the scatter)
    row(SK_RING_SPLIT, tiles, count, kTileThreads, ring_scatter_lds_bytes(H), KID_RING_SCATTER);
  } else {
    row(SK_CLASSIFY, tiles, count, kTileThreads, 0, KID_CLASSIFY);
    row(SK_RING_SCATTER, tiles, count, kTileThreads, ring_scatter_lds_bytes(H), KID_RING_SCATTER);
  }
  const int ext = ring_extract_threads(p.scan_regions);
  // instance by the longest region the expected ring width gives (the last region takes the split's remainder)
  const int w = rq.max_width > 0 ? rq.max_width : std::max(1, p.max_points / std::max(1, H));
  const int total = std::max(0, w - 10), sector = total / std::max(1, p.scan_regions);
  const bool big = total - sector * (p.scan_regions - 1) > kExLPR * kExIPL;
  row(ext <= 256 ? (big ? SK_RING_EXTRACT_256_BIG : SK_RING_EXTRACT_256) : (big ? SK_RING_EXTRACT_1024_BIG : SK_RING_EXTRACT_1024),
      H, count, ext, p.ring_lds_bytes, KID_RING_EXTRACT);
  row(SK_COMPACT_EDGES, kCompactBlocks, count, 256, 0, KID_COMPACT);
}

}  // namespace liodom_dev
