// liodom_hip.hip — host side of libliodom_hip.so: handle, HBM layout, launch sequencing and the
// C-ABI declared in include/liodom_hip.h.  No torch types, no CPU fallback: every entry point
// drives the HIP kernels of liodom_kernels.h or fails with an error code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <atomic>
#include <chrono>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "liodom_kernels.h"
#include "handle_plan.h"
#include "step_plan.h"
#include "edge_pipe.h"
#include "map_attach.h"
#include "odom_edges.h"
#include "kernels_odom_edges.h"

using namespace liodom_dev;

namespace {

thread_local std::string g_last_error;

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      char _buf[512];                                                                         \
      snprintf(_buf, sizeof(_buf), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
               __FILE__, __LINE__);                                                           \
      g_last_error = _buf;                                                                    \
      return LIODOM_ERR_HIP;                                                                  \
    }                                                                                         \
  } while (0)

const char* kKernelNames[LIODOM_NUM_KERNELS] = {
    "k_classify", "k_ring_extract", "k_compact_edges", "k_knn", "k_lm_solve",
    "k_hash_clear", "k_window_insert", "k_hash_alloc", "k_hash_scatter", "k_ring_scatter", "k_hash_build", "other"};

struct EventPair { hipEvent_t a, b; int kid; };

}  // namespace

#include "liodom_map_host.h"

std::atomic<int> g_live_handles{0};      // handles alive in this process (the overlapped second kNN pass is for a GPU one handle has to itself)

struct liodom_handle {
  liodom_params_t params;
  liodom_config_t config;
  HandlePlan plan;                   // what liodom_create decided: code paths, capacities (handle_plan.h); safe mode is the only later change
  DevView v{};                       // its scalar members are the plan's, written by plan_to_view alone
  DevView* d_view = nullptr;         // device copy: kernels take a pointer (8-byte kernarg)
  // Two sides, as in the reference's liodom_node (src/liodom_node.cc:89-91: one FeatureExtractor thread,
  // one LaserOdometer thread).  The EXTRACTION side owns stream_x, the ring-split scratch, stage_in and
  // edge buffer kEdgeBufX; the ODOMETRY side owns `stream`, edge buffers 0 / 1 / 2, the window, the hash and
  // the result records.  mx_x / mx_o serialise callers of each side; an entry point that needs both
  // (process_scan, the resident replay, reset, ...) takes mx_o first, then mx_x.  liodom_extract_edges
  // (mx_x only) and liodom_odometry_step (mx_o only) can therefore run concurrently from two threads.
  std::mutex mx_x, mx_o;
  hipStream_t stream = nullptr;      // odometry side
  StepState step;                    // the odometry side's state from scan to scan (step_plan.h), under mx_o
  ExtractState xstep;                // ... and the extraction side's, under mx_x
  hipStream_t stream_k = nullptr;    // overlapped second kNN pass of a scan (kernels_sync.h "Overlapped second kNN pass"): beside the first solve
  bool counted_live = false;         // this handle is part of g_live_handles
  hipEvent_t ev_ov = nullptr;        // recorded on the odometry stream in front of the first overlapped scan after scans that were not
  bool stream_c_shared = false;      // stream_c is stream_k
  bool ov_suppress = false;          // host-fed replay: the host's enqueue work per scan is the limit there, and the overlapped pass costs two more launches
  // Chain mode (kernels_sync.h "Chain mode"): the scan's kNN passes and the rebuild on stream_k, the two solves — launches of the
  // solving workgroups alone — on `stream`; the first solve's launch is resident beside the first pass.
  double replay_enq_ns = 0.0, replay_wait_ns = 0.0;      // depth-1 resident replay: host time per scan spent enqueueing / waiting for the previous pose
  long long replay_timed = 0;
  hipEvent_t ev_ch = nullptr;        // at a switch out of chain mode: the odometry stream waits for stream_k
  hipStream_t stream_x = nullptr;    // extraction side (liodom_extract_edges, and the next scan's extraction in the pipelined replay)
  hipStream_t stream_c = nullptr;    // host-fed replay: uploads (a copy engine works beside the extraction kernels of the previous scan)
  hipEvent_t ev_up[3] = {nullptr, nullptr, nullptr};      // staging slot uploaded
  hipEvent_t ev_xdone[3] = {nullptr, nullptr, nullptr};   // extraction that read the staging slot has been issued (recorded on the extraction stream)
  hipEvent_t ev_edges[kEdgePipeBufs] = {nullptr, nullptr, nullptr};   // edge buffer b written
  hipEvent_t ev_free[kEdgePipeBufs] = {nullptr, nullptr, nullptr};    // odometry finished reading edge buffer b
  // Who may use the three pipeline edge buffers, and what a launch into one has to wait for (edge_pipe.h): the pipelined replay
  // (flags in device memory, pipe_flags in DevView; events for handles with >= 16 streams and as the fallback) and the device-resident
  // hand-off of the two-thread binding (liodom_extract_edges_device on the extraction side fills a buffer and returns a ticket,
  // liodom_odometry_step_device on the odometry side consumes it: the element of the reference's feature queue,
  // shared_data.cc:64-89, without the cloud leaving HBM).
  EdgePipe pipe;
  float4* host_edges = nullptr;      // host-mapped mirror of the dense edges of pipeline buffers 0..2 (one-stream handles; DevView::host_edges)
  int4* host_edges_meta = nullptr;
  unsigned int* host_edges_hdr = nullptr;
  StagingRing pin;                   // page-locked scan staging ring [kEdgePipeBufs][max_points] (hipHostMalloc: pin.base): liodom_scan_buffer hands slots out, pageable scans are copied through it
  std::vector<double> replay_stamps;  // (debug) host time, us since the call began, at which every pose of the last liodom_replay_resident call was collected
  hipEvent_t ev_pin[kEdgePipeBufs] = {nullptr, nullptr, nullptr};     // the upload out of staging slot r has completed
  // Polar scans (liodom_set_polar_geometry; nothing below exists on a handle that never sets one): the geometry's tables on the
  // device, three compact staging slots the blobs are uploaded into (taken in turn), and the page-locked blob ring of the ticket
  // path (liodom_scan_buffer_polar) with the events that tell when an upload has left a ring slot.
  bool polar = false;
  PolarView pol{};                   // (beam / enc point into pol_tables)
  void* pol_tables = nullptr;        // device: float4 beam[H], float2 enc[T]
  unsigned char* pol_stage = nullptr;     // device: [kEdgePipeBufs][blob_bytes]
  int pol_stage_next = 0;
  StagingRing pol_pin;                    // host, page-locked: [kEdgePipeBufs][blob_bytes]
  hipEvent_t ev_polpin[kEdgePipeBufs] = {nullptr, nullptr, nullptr};
  bool streams_concurrent = true;    // liodom_create's probe: kernels of two streams of this handle ran side by side
  std::atomic<bool> fallback_pending{false};   // a kernel of this handle gave up an in-kernel wait (LIODOM_STATUS_PIPE_TIMEOUT): liodom_reset() switches to events
  long long subset_steps = 0;        // steps that ran over a stream list (liodom_get_modes)
  std::vector<int> last_eb;          // per stream: edge buffer of the stream's most recent scan that entered odometry (inspection)
  hipEvent_t pose_event = nullptr;
  int S = 1, H = 0, P = 0;
  // staging
  float4* stage_in = nullptr;        // [S][max_points]  (host-provided scans / edges)
  float4* resident = nullptr;        // [S][n_slots][max_points]
  int n_slots = 0;
  HostOut* host_out = nullptr;       // host-mapped pinned result records, one per stream
  HostCov* cov_host = nullptr;       // pose_covariance = 1: host-mapped covariance records, two per stream (DevView::cov_host)
  std::vector<int> scans_enqueued;   // per stream: scans launched so far (expected HostOut.seq)
  std::vector<int> log_first;        // per stream: scans_enqueued as the last reset, seed or import left it — the first scan this life of the stream logs (liodom_get_odometry_edges)
  void* odom_ws = nullptr;           // liodom_get_odometry_edges: intervals and records of one call on the device; null until the first call
  size_t odom_ws_bytes = 0;
  unsigned char* state_stage = nullptr;       // stream-state blob staging (liodom_export_stream_state / liodom_import_stream_state): device side,
  unsigned char* state_stage_host = nullptr;  // page-locked host side; both allocated by the first export or import
  std::vector<void*> allocs;
  // profiling
  std::atomic<bool> profiling{false};   // read without a lock by SideLocks / extract_queue, written under both mutexes
  // which map each stream writes (mapping replay) or reads (localising in a map it never writes; a step enqueues one
  // k_map_local_rows launch per distinct map over the step's rows), and with hits on or off: map_attach.h.  Below, the device
  // words that mirror it, each null until first used.
  StreamMaps<liodom_map, liodom_mapper_options_t> maps;
  // lagged mappers (lag = 1; from the first such attach on): per stream, the frame the step's append overwrites
  float4* lag_stash = nullptr;        // [S][edge_cap]
  int* lag_stash_n = nullptr;         // [S] its points (0 while the window is not full)
  int* lag_on = nullptr;              // [S] the stream has a lagged mapper (read by k_window_stash)
  int4* reader_sel = nullptr;         // [S] from the first reader on: {tag of the map the stream reads (0: none), cells_xy, cells_z, 0}
  // per-scan map-hit records (liodom_set_map_hits; from the first enabling call on)
  liodom_map_hit_t* hit_log = nullptr;   // [S][pose_log_cap] device, indexed like pose_log
  int* hit_radius = nullptr;          // [S] device: -1 off, else the radius the stream's scans are counted with
  std::vector<EventPair> ev_pool;
  size_t ev_used = 0;
  double k_ms[LIODOM_NUM_KERNELS] = {0};
  long long k_count[LIODOM_NUM_KERNELS] = {0};
};

namespace {

template <typename T>
int dev_alloc(liodom_handle* h, T** p, size_t count, int memset_value = 0) {
  void* raw = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIP_TRY(hipMalloc(&raw, bytes));
  h->allocs.push_back(raw);
  HIP_TRY(hipMemsetAsync(raw, memset_value, bytes, h->stream));
  *p = static_cast<T*>(raw);
  return LIODOM_OK;
}

// A map whose last attachment has gone gets a stream of its own again (a failure leaves it with none, and "attached" to callers).
hipError_t map_own_stream(liodom_map* m) {
  m->stream = nullptr; m->own_stream = false;
  const hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e == hipSuccess) m->own_stream = true;
  return e;
}

int drain_events(liodom_handle* h) {
  if (h->ev_used == 0) return LIODOM_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->stream_x) HIP_TRY(hipStreamSynchronize(h->stream_x));
  for (size_t i = 0; i < h->ev_used; i++) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_pool[i].a, h->ev_pool[i].b));
    h->k_ms[h->ev_pool[i].kid] += ms;
    h->k_count[h->ev_pool[i].kid] += 1;
  }
  h->ev_used = 0;
  return LIODOM_OK;
}

struct ProfScope {
  liodom_handle* h;
  EventPair* ep = nullptr;
  hipStream_t st;
  ProfScope(liodom_handle* hh, int kid, hipStream_t stream = nullptr) : h(hh), st(stream ? stream : hh->stream) {
    if (!h->profiling) return;
    if (h->ev_used == h->ev_pool.size()) {
      if (h->ev_pool.size() < 4096) {
        EventPair e; e.kid = kid;
        if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
        h->ev_pool.push_back(e);
      } else {
        drain_events(h);
      }
    }
    ep = &h->ev_pool[h->ev_used++];
    ep->kid = kid;
    hipEventRecord(ep->a, st);
  }
  ~ProfScope() { if (ep) hipEventRecord(ep->b, st); }
};

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

#include "liodom_step_host.h"

// Every entry point starts here: the calling thread's current device becomes the handle's (other
// handles / maps of the process may live on other GPUs, and HIP's current device is per thread).
int enter(liodom_handle* h) {
  if (!h) return LIODOM_ERR_INVALID_ARG;
  HIP_TRY(hipSetDevice(h->config.device));
  return LIODOM_OK;
}
int check_stream(liodom_handle* h, int stream) {
  int rc = enter(h);
  if (rc) return rc;
  if (stream < 0 || stream >= h->S) { g_last_error = "stream index out of range"; return LIODOM_ERR_INVALID_ARG; }
  return LIODOM_OK;
}
// entry points that enqueue scans: not after an in-kernel wait of this handle gave up (see wait_pose)
int check_usable(liodom_handle* h) {
  if (h->fallback_pending.load()) {
    g_last_error = "the handle had a LIODOM_STATUS_PIPE_TIMEOUT: call liodom_reset() before processing further scans";
    return LIODOM_ERR_HIP;
  }
  return LIODOM_OK;
}
// Lock guards of the two sides.  While per-kernel profiling is on, extraction runs on the odometry
// stream (so that HIP-event durations are not inflated by the other side's kernels) and shares the
// event pool: then every entry point takes both locks and the two sides are serialised.
struct SideLocks {
  std::unique_lock<std::mutex> lo, lx;
  SideLocks(liodom_handle* h, bool odo, bool ext) {
    if (odo || h->profiling) lo = std::unique_lock<std::mutex>(h->mx_o);
    if (ext || h->profiling) lx = std::unique_lock<std::mutex>(h->mx_x);
    // profiling was switched on between the test above and the locks (set_profiling holds both): take the rest
    if (h->profiling && !(lo.owns_lock() && lx.owns_lock())) {
      if (lx.owns_lock()) lx.unlock();
      if (!lo.owns_lock()) lo = std::unique_lock<std::mutex>(h->mx_o);
      lx = std::unique_lock<std::mutex>(h->mx_x);
    }
  }
};
hipStream_t extract_queue(liodom_handle* h) { return h->profiling ? h->stream : h->stream_x; }

// The plain (non-pipelined) entry points run everything on h->stream with edge buffer 0; make
// sure no extraction issued ahead by the pipelined replay is still in flight.
int tickets_idle(liodom_handle* h) {      // the plain entry points use pipeline edge buffer 0 themselves
  if (h->pipe.tickets_idle()) return LIODOM_OK;
  g_last_error = "edge tickets of liodom_extract_edges_device are outstanding: consume them with liodom_odometry_step_device first";
  return LIODOM_ERR_BUSY;
}
int drain_pipeline(liodom_handle* h) {
  if (h->pipe.needs_drain()) {
    HIP_TRY(hipStreamSynchronize(h->stream_x));
    HIP_TRY(sync_odometry(h));
    h->pipe.drained();
  }
  return LIODOM_OK;
}

// The odometry of the scan in pipeline edge buffer eb behind whatever produces that buffer (extraction number wait_seq with
// flags, ev_edges[eb] with events), as the pipelined replay and the device-resident hand-off enqueue it.  Odometry side.
// (s0, count, list): the step's streams as launch_odometry takes them; every stream by default.
int enqueue_pipeline_odometry(liodom_handle* h, int eb, unsigned int wait_seq, int s0 = 0, int count = -1, const int32_t* list = nullptr) {
  int rc;
  if (count < 0) count = h->S;
  if (h->plan.use_flags) {
    // no cross-stream events (they cost ~11 us of idle odometry stream per scan, with the host far ahead as well): the
    // first kNN launch waits for the extraction's flag and signals that the previous odometry has completed
    const unsigned int m = h->pipe.odometry_numbered();
    if (h->plan.flag_gate) {
      if (s0 < 0) hipLaunchKernelGGL(k_pipe_gate<true>, dim3(1), dim3(64), 0, h->stream, h->v, s0, eb, wait_seq, m - 1u);
      else hipLaunchKernelGGL(k_pipe_gate<>, dim3(1), dim3(64), 0, h->stream, h->v, s0, eb, wait_seq, m - 1u);
      rc = launch_odometry(h, eb, s0, count, 0u, 0u, list);
    } else {
      rc = launch_odometry(h, eb, s0, count, wait_seq, m - 1u, list);
    }
    if (rc) return rc;
    h->pipe.odometry_reads(eb, m);
  } else {
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_edges[eb], 0));
    rc = launch_odometry(h, eb, s0, count, 0u, 0u, list);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_free[eb], h->stream));
    h->pipe.odometry_recorded(eb);
  }
  return LIODOM_OK;
}

// Extraction of resident slot `slot` into edge buffer `eb` on the extraction stream.
// (s0, count): the streams as launch_extract takes them; every stream by default.  A list launch reads the slot by stream, so `in` is the slot's base either way.
int issue_extract(liodom_handle* h, int slot, int eb, int n, int height, int width, int s0 = 0, int count = -1) {
  if (count < 0) count = h->S;
  // while per-kernel profiling is on, everything runs on one stream so that the HIP-event
  // durations are not inflated by kernels of the other stream sharing the GPU
  hipStream_t q = extract_queue(h);
  const float4* in = h->resident + (size_t)slot * h->S * (size_t)h->v.max_points;
  if (h->plan.use_flags) {
    // dependencies through flags in device memory (pipe_wait): the buffer's last reader must have
    // completed before k_compact_edges rewrites it; the last workgroup of k_compact_edges sets the flag of this extraction
    const unsigned int seq = h->pipe.extract_numbered(eb);
    return launch_extract(h, q, eb, s0, count, in, (size_t)h->v.max_points, n, height, width, h->pipe.eb_reader[eb], 0,
                          h->v.pipe_flags + eb, nullptr, seq);
  }
  if (h->pipe.ev_free_valid[eb]) HIP_TRY(hipStreamWaitEvent(q, h->ev_free[eb], 0));
  int rc = launch_extract(h, q, eb, s0, count, in, (size_t)h->v.max_points, n, height, width);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(h->ev_edges[eb], q));
  return LIODOM_OK;
}

// Safe mode (plan_enter_safe_mode, handle_plan.h) after an in-kernel wait gave up: the plan changes, the view follows; every
// buffer stays as allocated.
void enter_safe_mode(liodom_handle* h) {
  plan_enter_safe_mode(&h->plan);
  plan_to_view(h->plan, &h->v);
}

int reset_state(liodom_handle* h) {
  // nothing of an earlier scan may still be in flight: its finalize would publish into the records
  // zeroed below, and an extraction issued ahead would write into scratch that is being reset
  if (h->stream_x) HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->stream_k) HIP_TRY(hipStreamSynchronize(h->stream_k));
  if (h->fallback_pending.exchange(false)) enter_safe_mode(h);      // an in-kernel wait gave up (wait_pose)
  std::vector<StreamState> init((size_t)h->S);
  for (auto& st : init) {
    std::memset(&st, 0, sizeof(st));
    iso_identity(st.odom); iso_identity(st.prev_odom); iso_identity(st.final_odom); iso_identity(st.pred_odom[0]); iso_identity(st.pred_odom[1]);
    st.param_q[3] = 1.0;
    st.table_mask = (uint32_t)h->v.table_size - 1u;
  }
  HIP_TRY(hipMemcpyAsync(h->v.state, init.data(), sizeof(StreamState) * init.size(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->v.pub_counter, 0, sizeof(unsigned int) * (size_t)kEdgeBufs, h->stream));
  if (h->v.lb_ticket) { HIP_TRY(hipMemsetAsync(h->v.lb_ticket, 0, sizeof(unsigned int), h->stream)); HIP_TRY(hipMemsetAsync(h->v.lb_ovf, 0, sizeof(unsigned int) * (size_t)h->S, h->stream)); }
  {
    std::vector<double> qid((size_t)h->S * 4, 0.0);          // IMU orientation: identity until imuClb delivers one
    for (int s = 0; s < h->S; s++) qid[(size_t)s * 4 + 3] = 1.0;
    HIP_TRY(hipMemcpy(h->v.imu_q, qid.data(), sizeof(double) * qid.size(), hipMemcpyHostToDevice));
  }
  {
    const size_t total = (size_t)h->S * h->v.table_size * (h->v.early_rebuild ? 2 : 1);
    hipLaunchKernelGGL(k_init_cells, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->v);
    HIP_TRY(hipGetLastError());
  }
  h->last_eb.assign((size_t)h->S, 0);
  h->step.reset();
  if (h->stream_c && !h->stream_c_shared) HIP_TRY(hipStreamSynchronize(h->stream_c));
  h->pipe.reset();      // outstanding edge tickets are void
  h->pin.uploads_left(); h->pol_pin.uploads_left();
  if (h->host_edges_hdr) std::memset(h->host_edges_hdr, 0, sizeof(unsigned int) * 2 * kEdgePipeBufs);
  HIP_TRY(hipMemsetAsync(h->v.pipe_flags, 0, sizeof(unsigned int) * (kEdgePipeBufs + 1), h->stream));
  HIP_TRY(hipMemsetAsync(h->v.lm_xch, 0, sizeof(unsigned long long) * (size_t)h->S * 2 * kLmGroupsMax * 64, h->stream));
  HIP_TRY(hipMemsetAsync(h->v.pose_xch, 0, sizeof(unsigned long long) * (size_t)h->S * 64, h->stream));
  HIP_TRY(hipMemsetAsync(h->v.redo_sync, 0, sizeof(unsigned int) * 64, h->stream));
  if (h->v.pred_xch) HIP_TRY(hipMemsetAsync(h->v.pred_xch, 0, sizeof(unsigned long long) * (size_t)h->S * kOvReplicas * 512, h->stream));
  HIP_TRY(hipMemsetAsync(h->v.knn_done0, 0, sizeof(unsigned int) * ((size_t)h->S + 64), h->stream));
  h->replay_enq_ns = 0.0; h->replay_wait_ns = 0.0; h->replay_timed = 0;
  std::memset(h->host_out, 0, sizeof(HostOut) * 2 * (size_t)h->S);
  if (h->cov_host) {
    std::memset(h->cov_host, 0, sizeof(HostCov) * 2 * (size_t)h->S);
    HIP_TRY(hipMemsetAsync(h->v.cov_raw, 0, sizeof(PoseCovRaw) * (size_t)h->S, h->stream));
  }
  std::fill(h->scans_enqueued.begin(), h->scans_enqueued.end(), 0);
  std::fill(h->log_first.begin(), h->log_first.end(), 0);
  HIP_TRY(hipMemsetAsync(h->v.win_n, 0, sizeof(int) * (size_t)h->S * h->P, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return LIODOM_OK;
}

// A kernel's dynamic LDS above the 48 KiB every kernel may have needs the function attribute (liodom_create).
struct LdsNeed {
  const void* fn;
  size_t bytes;
  bool always;          // set the attribute below 48 KiB as well
  bool list;            // a list instance (subset steps, stream_of): handles with more than one stream only
  const bool* when;     // null, or the path the kernel belongs to: skipped while it is off
  bool* clears;         // null: a failure fails the create; else the path a failure switches off
};

}  // namespace

extern "C" {

const char* liodom_last_error(void) { return g_last_error.c_str(); }

void liodom_params_default(liodom_params_t* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_range = 3.0;            // params.cc:40
  p->max_range = 75.0;           // params.cc:44
  p->lidar_type = 0;             // params.cc:48
  p->scan_lines = 64;            // params.cc:52
  p->scan_regions = 8;           // params.cc:56
  p->edges_per_region = 10;      // params.cc:60
  p->min_points_per_scan = 8 * 10 + 10;  // params.cc:63
  p->local_map_size = 5;         // params.cc:90-93
  p->save_results = 0;           // params.cc:66
  std::strcpy(p->results_dir, "~/");        // params.cc:70
  std::strcpy(p->fixed_frame, "odom");      // params.cc:74
  std::strcpy(p->base_frame, "base_link");  // params.cc:78
  p->laser_frame[0] = 0;                    // params.cc:82
  p->use_imu = 0; p->filter_local_map = 0; p->mapping = 0;   // params.cc:96,100,104
  p->publish_tf = 1;                                         // params.cc:108
}

void liodom_config_default(liodom_config_t* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->device = 0; c->n_streams = 1; c->max_points = 64 * 1800; c->max_width = 1800;
  c->reserved1 = 0; c->lm_apply_step_on_ftol = 0; c->pose_log_capacity = 1024; c->debug_buffers = 0;
  c->lm_workgroups = 0;
  c->pose_rotation_mode = 1;    // Eigen 3.3.x Transform::rotation()
}

int liodom_create(const liodom_params_t* params, const liodom_config_t* config, liodom_handle_t** out) {
  if (!params || !config || !out) return LIODOM_ERR_INVALID_ARG;
  *out = nullptr;
  const char* why = nullptr;
  if (int rc = plan_check_params(params, config, &why)) { g_last_error = why; return rc; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    g_last_error = "no HIP device available (libliodom_hip has no CPU fallback)";
    return LIODOM_ERR_NO_DEVICE;
  }
  if (config->device < 0 || config->device >= ndev) { g_last_error = "bad device ordinal"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(hipSetDevice(config->device));
  const int H = params->scan_lines;
  // what the device contributes to the plan
  HandleCaps caps;
  caps.instrumented = kInstrument;
  (void)hipDeviceGetAttribute(&caps.cus, hipDeviceAttributeMultiprocessorCount, config->device);
  {
    const size_t lds = ring_scatter_lds_bytes(H);
    const void* fn = reinterpret_cast<const void*>(&k_ring_split<>);
    if ((lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&caps.ring_split_wgs_per_cu, fn, kTileThreads, lds) != hipSuccess) {
      (void)hipGetLastError(); caps.ring_split_wgs_per_cu = 0;
    }
  }
  HandlePlan plan;
  if (int rc = plan_handle(params, config, caps, read_handle_env(), &plan, &why)) { g_last_error = why; return rc; }

  liodom_handle* h = new liodom_handle();
  h->params = *params;
  h->config = *config;
  h->S = config->n_streams; h->H = H; h->P = (int)params->local_map_size;
  h->plan = plan;
  HandlePlan& p = h->plan;
  DevView& v = h->v;
  plan_to_view(p, &v);
  iso_identity(v.laser_to_base);
  int rc = LIODOM_OK;
  auto fail = [&](int code) { liodom_destroy(h); return code; };
  // The odometry chain is the critical path; the extraction of the next scan only has to finish
  // before that chain ends.  Stream priorities let the chain's kernels win the CUs when both want them.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const bool use_prio = prio_least != prio_greatest;
  // (a CU split — hipExtStreamCreateWithCUMask: the extraction stream on 32 / 64 / 96 CUs, the chain's streams on the rest —
  //  was measured: -0.1 / -1.5 / -2.7 %; the wave priority of the chain's kernels, LIODOM_CHAIN_PRIO, is what helps)
  auto make_stream = [&](hipStream_t* st, int prio) {
    return use_prio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio) : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  };
  auto make_event = [&](hipEvent_t* ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming); };
  // (extraction: one level below the odometry stream, not the lowest: kernels of the odometry stream may wait in-kernel for it)
  const int prio_x = (prio_least - prio_greatest >= 2) ? prio_greatest + 1 : prio_least;
  // (stream_k exists only on handles that use it: HIP multiplexes its streams onto a few hardware queues, and one more
  //  stream made the host-fed replay's copy stream share a queue — 11.3k -> 7.5k scans/s on every workload)
  if (make_stream(&h->stream, prio_greatest) != hipSuccess || make_stream(&h->stream_x, prio_x) != hipSuccess ||
      ((p.ov_ok || p.chain_ok) && make_stream(&h->stream_k, prio_greatest) != hipSuccess)) { g_last_error = "hipStreamCreate failed"; return fail(LIODOM_ERR_HIP); }
  bool events = make_event(&h->ev_ov) == hipSuccess && make_event(&h->pose_event) == hipSuccess && (!p.chain_ok || make_event(&h->ev_ch) == hipSuccess);
  for (int b = 0; b < kEdgePipeBufs; b++) events = events && make_event(&h->ev_edges[b]) == hipSuccess && make_event(&h->ev_free[b]) == hipSuccess;
  if (!events) { g_last_error = "hipEventCreate failed"; return fail(LIODOM_ERR_HIP); }

  const size_t S = (size_t)h->S;
#define ALLOC(ptr, count, fill) do { rc = dev_alloc(h, &(ptr), (count), (fill)); if (rc != LIODOM_OK) return fail(rc); } while (0)
  ALLOC(v.state, S, 0);
  ALLOC(v.ring_id, S * p.ring_id_stride, 0xFF);
  ALLOC(v.tile_hist, S * (size_t)p.tile_cap * H, 0);
  if (p.ring_split_lb) { ALLOC(v.lb_desc, S * (size_t)p.tile_cap * p.lb_hpad, 0); ALLOC(v.lb_ticket, 1, 0); ALLOC(v.lb_ovf, S, 0); }
  // + padding: region_keys_load reads unconditionally up to 16 * IPL + 10 points past the start of a ring's last region,
  // i.e. up to kExLPR * kExIPLBig + 10 points past the end of the last ring of the last stream (values never used)
  ALLOC(v.ring_pts, S * p.ring_stride + kExLPR * kExIPLBig + 64, 0);
  ALLOC(v.ring_src, S * p.ring_stride, 0);
  ALLOC(v.ring_start, S * (size_t)(H + 1), 0);
  ALLOC(v.ring_len, S * (size_t)H, 0);
  ALLOC(v.edges_pad, S * H * p.slots_per_ring, 0);
  ALLOC(v.edges_pad_meta, S * H * p.slots_per_ring, 0);
  ALLOC(v.ring_nedges, S * H, 0);
  if (p.ring_split) { ALLOC(v.split_ctr, 2 * S, 0); ALLOC(v.split_hist, S * (size_t)H * p.split_pad + 64, 0); }      // (+ one batch of 64 tiles: k_ring_split reads whole batches)
  ALLOC(v.ring_npoints, S * H, 0);
  ALLOC(v.ring_c, S * p.ring_stride, 0);
  ALLOC(v.ring_picked, S * p.ring_stride, 0);
  ALLOC(v.edges, kEdgeBufs * S * p.edge_cap, 0);
  ALLOC(v.edges_meta, kEdgeBufs * S * p.edge_cap, 0);
  ALLOC(v.corr_a, S * 2 * p.edge_cap, 0);
  ALLOC(v.corr_b, S * 2 * p.edge_cap, 0);
  ALLOC(v.corr_idx, S * 2 * p.edge_cap, 0xFF);
  if (p.debug & 1) ALLOC(v.knn_q, S * 2 * p.edge_cap, 0);
  ALLOC(v.win_pts, S * p.prev_frames * p.edge_cap, 0);
  ALLOC(v.win_n, S * p.prev_frames, 0);
  ALLOC(v.win_base, S * (p.prev_frames + 1), 0);
  ALLOC(v.win_slot, S * p.prev_frames, 0);
  const size_t ntab = p.early_rebuild ? 2 : 1;     // early_rebuild: two cell hashes per stream (index s + parity * S)
  ALLOC(v.cells, ntab * S * p.table_size, 0);
  ALLOC(v.pt_rank, S * p.map_cap, 0);
  ALLOC(v.cell_bits, ntab * S * (size_t)(p.table_size / 32), 0);
  ALLOC(v.used_cells, ntab * S * (size_t)p.used_cap, 0);
  ALLOC(v.pt_cell, S * p.map_cap, 0xFF);
  if (p.recv_cap) ALLOC(v.recv_pts, S * p.recv_cap, 0);
  ALLOC(v.imu_q, S * 4, 0);
  ALLOC(v.sorted_pts, ntab * S * (size_t)p.sorted_cap, 0);
  if (p.early_rebuild) ALLOC(v.cell_pad, 2 * S * (size_t)p.table_size, 0);
  if (p.filter_local_map) {
    ALLOC(v.vox_cells, S * p.table_size, 0);
    ALLOC(v.vox_fill, S * p.table_size, 0);
    ALLOC(v.vox_used_list, S * p.map_cap, 0);
    ALLOC(v.pt_vox, S * p.map_cap, 0xFF);
    ALLOC(v.vox_pts, S * p.map_cap, 0);
    ALLOC(v.filt_pts, S * p.map_cap, 0);
    ALLOC(v.filt_int, S * p.map_cap, 0);
  }
  ALLOC(v.pose_log, S * p.pose_log_cap * 7, 0);
  ALLOC(v.info_log, S * p.pose_log_cap, 0);
  ALLOC(h->stage_in, S * (size_t)p.max_points, 0);
  ALLOC(v.dbg_clk, 16 * 32, 0);
  if (p.debug & 32) ALLOC(v.dbg_q, 2 * (size_t)p.edge_cap * 12, 0);
  ALLOC(v.lm_xch, S * 2 * kLmGroupsMax * 64, 0);
  ALLOC(v.pose_xch, S * 64, 0);
  ALLOC(v.redo_sync, 64, 0);
  ALLOC(v.pipe_flags, (size_t)kStreamListBase + (size_t)kStreamLists * S, 0);      // (+ the stream lists of subset steps, stream_of)
  if (S == 1) {
    // device-resident hand-off (liodom_extract_edges_device): host-mapped mirror of the dense edges of the three pipeline buffers
    const size_t ne = (size_t)kEdgePipeBufs * p.edge_cap;
    void *he = nullptr, *hm = nullptr, *hh = nullptr;
    if (hipHostMalloc(&he, sizeof(float4) * ne, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc(&hm, sizeof(int4) * ne, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc(&hh, sizeof(unsigned int) * 2 * kEdgePipeBufs, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      if (he) hipHostFree(he);
      if (hm) hipHostFree(hm);
      g_last_error = "hipHostMalloc (edge mirror) failed"; return fail(LIODOM_ERR_HIP);
    }
    h->host_edges = static_cast<float4*>(he); h->host_edges_meta = static_cast<int4*>(hm); h->host_edges_hdr = static_cast<unsigned int*>(hh);
    std::memset(hh, 0, sizeof(unsigned int) * 2 * kEdgePipeBufs);
    void *de = nullptr, *dm = nullptr, *dh = nullptr;
    if (hipHostGetDevicePointer(&de, he, 0) != hipSuccess || hipHostGetDevicePointer(&dm, hm, 0) != hipSuccess ||
        hipHostGetDevicePointer(&dh, hh, 0) != hipSuccess) { g_last_error = "hipHostGetDevicePointer failed"; return fail(LIODOM_ERR_HIP); }
    v.host_edges = static_cast<float4*>(de); v.host_edges_meta = static_cast<int4*>(dm); v.host_edges_hdr = static_cast<unsigned int*>(dh);
  }
  if (p.lockstep) ALLOC(v.knn_nn, S * (size_t)p.edge_cap * 5, 0);      // lock-step batches: line gates in their own launch (k_line_gate)
  if (p.hash_incr) ALLOC(v.cell_cap, S * (size_t)p.table_size, 0);
  if (p.knn8) { ALLOC(v.knn8_cnt, S, 0); ALLOC(v.knn8_list, S * (size_t)p.edge_cap, 0); }
  if (p.knn_save >= 1) ALLOC(v.knn_save_q, S * (size_t)p.edge_cap, 0);
  if (p.knn_save >= 2) { ALLOC(v.knn_save_pos, S * (size_t)p.edge_cap * kKnnGroup, 0xFF); ALLOC(v.knn_save_g, S * (size_t)p.edge_cap, 0); }
  ALLOC(v.knn_part, S * 2 * (size_t)p.knn_blocks * 32, 0);
  ALLOC(v.ov_flags, S, 0);
  ALLOC(v.pose_xch0, S * (size_t)kOvReplicas * 512, 0);
  ALLOC(v.knn_done, S * (size_t)p.knn_grid, 0);
  ALLOC(v.knn_done0, S + 64, 0);
  if (p.early_rebuild) ALLOC(v.pred_xch, S * (size_t)kOvReplicas * 512, 0);
  ALLOC(v.edge_cnt, (size_t)kEdgeBufs * 32, 0);
  ALLOC(v.pub_counter, (size_t)kEdgeBufs, 0);
  if (p.early_rebuild) ALLOC(v.edges_keep, S * (size_t)p.edge_cap, 0);
  ALLOC(v.corr_mask, S * 2 * (size_t)p.mask_stride, 0);
  {
    void* hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(HostOut) * 2 * S, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { g_last_error = "hipHostMalloc failed"; return fail(LIODOM_ERR_HIP); }
    h->host_out = static_cast<HostOut*>(hp);
    std::memset(hp, 0, sizeof(HostOut) * 2 * S);
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) { g_last_error = "hipHostGetDevicePointer failed"; return fail(LIODOM_ERR_HIP); }
    v.host_out = static_cast<HostOut*>(dp);
    h->scans_enqueued.assign(S, 0);
    h->log_first.assign(S, 0);
    h->step.bind(S);
    h->last_eb.assign(S, 0);
    h->maps.bind(h, S);
  }
  if (p.pose_covariance) {
    // per-scan pose covariance (kernels_cov.h): nothing of it exists on handles created without it
    ALLOC(v.cov_raw, S, 0);
    ALLOC(v.cov_log, S * (size_t)p.pose_log_cap, 0);
    void* hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(HostCov) * 2 * S, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { g_last_error = "hipHostMalloc failed"; return fail(LIODOM_ERR_HIP); }
    h->cov_host = static_cast<HostCov*>(hp);
    std::memset(hp, 0, sizeof(HostCov) * 2 * S);
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) { g_last_error = "hipHostGetDevicePointer failed"; return fail(LIODOM_ERR_HIP); }
    v.cov_host = static_cast<HostCov*>(dp);
  }
  {
    // dynamic LDS: one entry per kernel instance a handle may launch (k_ring_split<> has its attribute from the caps above).
    // k_ring_split_lb comes first: it is the one path a failure only switches off — its pitched buffers, sized from the
    // planned value, stay allocated — and its list instances further down are then skipped.
    const size_t scatter = ring_scatter_lds_bytes(H), split_lb = ring_split_lb_lds_bytes(H), build = hash_build_lds_bytes();
    const size_t solve = lm_lds_bytes(p.edge_cap), extract = p.ring_lds_bytes;
#define FN(...) reinterpret_cast<const void*>(&__VA_ARGS__)
    const LdsNeed needs[] = {
        {FN(k_ring_split_lb<>), split_lb, false, false, &p.ring_split_lb, &p.ring_split_lb},
        {FN(k_ring_split_fix<>), split_lb, false, false, &p.ring_split_lb, &p.ring_split_lb},
        {FN(k_ring_scatter<>), scatter, false, false, nullptr, nullptr},
        {FN(k_hash_build<>), build, true, false, nullptr, nullptr},
        {FN(k_lm_solve<0, false>), solve, true, false, nullptr, nullptr},
        {FN(k_lm_solve<1, false>), solve, true, false, nullptr, nullptr},
        {FN(k_lm_solve<0, true>), solve, true, false, nullptr, nullptr},
        {FN(k_lm_solve<1, true>), solve, true, false, nullptr, nullptr},
        {FN(k_ring_extract<256, kExIPL>), extract, false, false, nullptr, nullptr},
        {FN(k_ring_extract<256, kExIPLBig>), extract, false, false, nullptr, nullptr},
        {FN(k_ring_extract<1024, kExIPL>), extract, false, false, nullptr, nullptr},
        {FN(k_ring_extract<1024, kExIPLBig>), extract, false, false, nullptr, nullptr},
        // the list instances of the kernels above (subset steps, stream_of) take the same dynamic LDS
        {FN(k_ring_split_lb<true>), split_lb, false, true, &p.ring_split_lb, nullptr},
        {FN(k_ring_split_fix<true>), split_lb, false, true, &p.ring_split_lb, nullptr},
        {FN(k_ring_split<true>), scatter, false, true, &p.ring_split, nullptr},
        {FN(k_ring_scatter<true>), scatter, false, true, nullptr, nullptr},
        {FN(k_hash_build<true>), build, true, true, nullptr, nullptr},
        {FN(k_lm_solve<0, false, true>), solve, true, true, nullptr, nullptr},
        {FN(k_lm_solve<1, false, true>), solve, true, true, nullptr, nullptr},
        {FN(k_ring_extract<256, kExIPL, true>), extract, false, true, nullptr, nullptr},
        {FN(k_ring_extract<256, kExIPLBig, true>), extract, false, true, nullptr, nullptr},
        {FN(k_ring_extract<1024, kExIPL, true>), extract, false, true, nullptr, nullptr},
        {FN(k_ring_extract<1024, kExIPLBig, true>), extract, false, true, nullptr, nullptr},
    };
#undef FN
    for (const LdsNeed& n : needs) {
      if ((n.list && S == 1) || (n.when && !*n.when) || !(n.always || n.bytes > 48 * 1024)) continue;
      if (hipFuncSetAttribute(n.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)n.bytes) == hipSuccess) continue;
      if (!n.clears) { g_last_error = "hipFuncSetAttribute(max dynamic LDS) failed"; return fail(LIODOM_ERR_HIP); }
      (void)hipGetLastError(); *n.clears = false;
    }
  }
  if (p.use_flags) {
    // Flags need kernels of the handle's streams to run side by side.  Known serialisers are caught by name (HandleEnv); this probe
    // catches the rest (a profiler collecting counters, a debugger): one wave on the odometry stream waits up to ~2 ms (k_probe_wait) for a flag
    // that a launch on the extraction stream sets.  If it gives up, the handle uses events from the start.
    unsigned int* probe = nullptr;
    ALLOC(probe, 4, 0);
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, h->stream, probe + 2, 1u);        // (first launches on both streams: code upload)
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, h->stream_x, probe + 3, 1u);
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipStreamSynchronize(h->stream_x) != hipSuccess) { g_last_error = "stream probe failed"; return fail(LIODOM_ERR_HIP); }
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(64), 0, h->stream, probe, probe + 1);
    hipLaunchKernelGGL(k_set_flag, dim3(1), dim3(1), 0, h->stream_x, probe, 1u);
    unsigned int res = 0;
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipStreamSynchronize(h->stream_x) != hipSuccess ||
        hipMemcpy(&res, probe + 1, sizeof(res), hipMemcpyDeviceToHost) != hipSuccess) { g_last_error = "stream probe failed"; return fail(LIODOM_ERR_HIP); }
    h->streams_concurrent = res == 1u;
    if (!h->streams_concurrent) p.use_flags = false;
  }
  // wall-clock bound of every in-kernel wait (g_wait_ticks, 100 MHz ticks)
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_wait_ticks), &p.wait_ticks, sizeof(p.wait_ticks)) != hipSuccess) { g_last_error = "hipMemcpyToSymbol(g_wait_ticks) failed"; return fail(LIODOM_ERR_HIP); }
  ALLOC(h->d_view, 1, 0);
  if (hipMemcpy(h->d_view, &h->v, sizeof(DevView), hipMemcpyHostToDevice) != hipSuccess) { g_last_error = "DevView upload failed"; return fail(LIODOM_ERR_HIP); }
  rc = reset_state(h);
  if (rc != LIODOM_OK) return fail(rc);
  g_live_handles.fetch_add(1);
  h->counted_live = true;
  *out = h;
  return LIODOM_OK;
#undef ALLOC
}

void liodom_destroy(liodom_handle_t* h) {
  if (!h) return;
  if (h->counted_live) g_live_handles.fetch_sub(1);
  if (h->stream_x) hipStreamSynchronize(h->stream_x);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream_k) { hipStreamSynchronize(h->stream_k); hipStreamDestroy(h->stream_k); }
  if (h->ev_ov) hipEventDestroy(h->ev_ov);
  if (h->ev_ch) hipEventDestroy(h->ev_ch);
  while (liodom_map* mp = h->maps.release_next()) (void)map_own_stream(mp);      // attached maps outlive the handle
  for (void* p : h->allocs) hipFree(p);
  if (h->resident) hipFree(h->resident);
  if (h->host_out) hipHostFree(h->host_out);
  if (h->cov_host) hipHostFree(h->cov_host);
  if (h->host_edges) hipHostFree(h->host_edges);
  if (h->host_edges_meta) hipHostFree(h->host_edges_meta);
  if (h->host_edges_hdr) hipHostFree(h->host_edges_hdr);
  if (h->pin.base) hipHostFree(h->pin.base);
  if (h->odom_ws) hipFree(h->odom_ws);
  if (h->pol_tables) hipFree(h->pol_tables);
  if (h->pol_stage) hipFree(h->pol_stage);
  if (h->pol_pin.base) hipHostFree(h->pol_pin.base);
  for (int b = 0; b < kEdgePipeBufs; b++) { if (h->ev_polpin[b]) hipEventDestroy(h->ev_polpin[b]); }
  if (h->state_stage_host) hipHostFree(h->state_stage_host);
  for (int b = 0; b < kEdgePipeBufs; b++) { if (h->ev_pin[b]) hipEventDestroy(h->ev_pin[b]); }
  for (auto& e : h->ev_pool) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
  if (h->pose_event) hipEventDestroy(h->pose_event);
  for (int b = 0; b < kEdgePipeBufs; b++) { if (h->ev_edges[b]) hipEventDestroy(h->ev_edges[b]); if (h->ev_free[b]) hipEventDestroy(h->ev_free[b]); }
  if (h->stream_c && !h->stream_c_shared) { hipStreamSynchronize(h->stream_c); hipStreamDestroy(h->stream_c); }
  for (int b = 0; b < 3; b++) { if (h->ev_up[b]) hipEventDestroy(h->ev_up[b]); if (h->ev_xdone[b]) hipEventDestroy(h->ev_xdone[b]); }
  if (h->stream_x) hipStreamDestroy(h->stream_x);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int liodom_reset(liodom_handle_t* h) {
  int rc = enter(h);
  if (rc) return rc;
  SideLocks lk(h, true, true);
  return reset_state(h);
}

// ---- streams with a life of their own: per-stream reset, export and import of the odometry state (kernels_state.h, stream_state_format.h) ----
// None of these calls is on the per-scan path; each takes both sides, refuses while edge tickets are outstanding, and waits for
// every HIP stream of the handle (a pending chain-mode repair included) before it touches anything.
static size_t state_max_bytes(const liodom_handle* h) {
  return state_blob_bytes(h->P, (long long)h->P * h->v.edge_cap, h->v.recv_cap);
}
static int state_quiesce(liodom_handle* h) {
  int rc = tickets_idle(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  if (h->stream_k) HIP_TRY(hipStreamSynchronize(h->stream_k));
  if (h->stream_c && !h->stream_c_shared) HIP_TRY(hipStreamSynchronize(h->stream_c));
  return LIODOM_OK;
}
static int ensure_state_stage(liodom_handle* h) {
  if (h->state_stage) return LIODOM_OK;
  void* hp = nullptr;
  HIP_TRY(hipHostMalloc(&hp, state_max_bytes(h), hipHostMallocDefault));
  h->state_stage_host = static_cast<unsigned char*>(hp);
  void* dp = nullptr;
  HIP_TRY(hipMalloc(&dp, state_max_bytes(h)));
  h->allocs.push_back(dp);
  h->state_stage = static_cast<unsigned char*>(dp);
  return LIODOM_OK;
}
static StateBlobHeader state_fingerprint(const liodom_handle* h) {
  StateBlobHeader hd = {};
  hd.local_map_size = (uint32_t)h->P; hd.mapping = h->params.mapping ? 1u : 0u; hd.filter_local_map = h->params.filter_local_map ? 1u : 0u;
  hd.use_imu = h->params.use_imu ? 1u : 0u; hd.pose_rotation_mode = (uint32_t)h->v.rotation_mode; hd.lm_apply_step_on_ftol = h->v.apply_on_ftol ? 1u : 0u;
  return hd;
}
// Everything of stream `stream` but its edge buffers becomes what `blob` (device staging; null: a stream that never ran) says, and
// the structure its next scan searches is rebuilt from the window for the variant this handle runs.  Streams are idle (state_quiesce).
// Left alone: the handle-wide pipeline state (EdgePipe, edge_pipe.h; the edge buffers and pipe_flags on the device): an extraction
// issued ahead stays valid for every stream.
static int install_stream_state(liodom_handle* h, int stream, const unsigned char* blob, int n_frames, int scan_counter, int n_recv = 0) {
  const DevView& v = h->v;
  const size_t S = (size_t)h->S, s = (size_t)stream;
  hipLaunchKernelGGL(k_stream_clear, dim3(64), dim3(kStateThreads), 0, h->stream, v, stream);
  hipLaunchKernelGGL(k_state_unpack, dim3(std::max(1, cdiv(v.map_cap, kStateThreads))), dim3(kStateThreads), 0, h->stream, v, stream, blob);
  // the stream's exchange granules carry tags derived from its frame and scan counts, which start over or jump here
  HIP_TRY(hipMemsetAsync(v.lm_xch + s * 2 * kLmGroupsMax * 64, 0, sizeof(unsigned long long) * 2 * kLmGroupsMax * 64, h->stream));
  HIP_TRY(hipMemsetAsync(v.pose_xch + s * 64, 0, sizeof(unsigned long long) * 64, h->stream));
  if (v.pred_xch) HIP_TRY(hipMemsetAsync(v.pred_xch + s * kOvReplicas * 512, 0, sizeof(unsigned long long) * kOvReplicas * 512, h->stream));
  if (v.cov_raw) HIP_TRY(hipMemsetAsync(v.cov_raw + s, 0, sizeof(PoseCovRaw), h->stream));
  if (S == 1) {
    // one-stream handles: the overlapped pass and chain mode start as after liodom_create — the first scans run every launch on the
    // odometry stream (an uninitialised stream publishes no pose an overlapped pass could wait for; the prediction granules of an
    // imported stream are written by its first scan here); their counters start over with the device's
    HIP_TRY(hipMemsetAsync(v.knn_done0, 0, sizeof(unsigned int) * (S + 64), h->stream));
    h->step.restart_overlap();
  }
  if (n_frames > 0 || n_recv > 0) {      // (a received map without a frame — a seeded stream before its first scan — is searched too)
    // (the hash step of a scan, always a rebuild, over the installed window: eb -1.  early_rebuild: the three kernels fill the table of
    //  parity frame_count & 1, the one the next scan searches; the other one and both overflow lists are empty)
    StepPlan plan;
    plan_full_rebuild(h->plan, &plan);
    StepData d;
    d.s0 = stream; d.count = 1; d.eb = -1;
    if (const int rc = issue_plan(h, plan, d)) return rc;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::memset(h->host_out + 2 * s, 0, sizeof(HostOut) * 2);
  if (h->cov_host) std::memset(h->cov_host + 2 * s, 0, sizeof(HostCov) * 2);
  h->scans_enqueued[s] = scan_counter;
  h->log_first[s] = scan_counter;
  h->step.hb_since[s] = -1;      // (hash_incr: the stream's next step rebuilds from the whole window)
  return LIODOM_OK;
}

int liodom_reset_stream(liodom_handle_t* h, int stream) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  SideLocks lk(h, true, true);
  if ((rc = state_quiesce(h))) return rc;
  return install_stream_state(h, stream, nullptr, 0, 0);
}

int liodom_stream_state_size(liodom_handle_t* h, int64_t* max_bytes) {
  int rc = enter(h);
  if (rc) return rc;
  if (!max_bytes) return LIODOM_ERR_INVALID_ARG;
  *max_bytes = (int64_t)state_max_bytes(h);
  return LIODOM_OK;
}

int liodom_export_stream_state(liodom_handle_t* h, int stream, void* blob, int64_t cap, int64_t* bytes) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!bytes || cap < 0 || (cap > 0 && !blob)) return LIODOM_ERR_INVALID_ARG;
  SideLocks lk(h, true, true);
  if ((rc = state_quiesce(h))) return rc;
  if ((rc = ensure_state_stage(h))) return rc;
  const DevView& v = h->v;
  // one kernel gathers record, frame counts, frames (oldest first) and the received map into the staging buffer; the record and the
  // counts come over first (they say how large the blob is), then the points in ONE copy of the blob's real size — not of the
  // buffer's upper bound, and not one copy per frame
  hipLaunchKernelGGL(k_state_pack, dim3(std::max(1, cdiv(v.map_cap, kStateThreads))), dim3(kStateThreads), 0, h->stream, v, stream, h->state_stage);
  HIP_TRY(hipGetLastError());
  const size_t prefix = state_points_offset(h->P);
  HIP_TRY(hipMemcpyAsync(h->state_stage_host, h->state_stage, prefix, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  StateBlobRecord rec;
  if (!state_packed_record(h->state_stage_host, h->P, v.edge_cap, v.recv_cap, &rec)) {
    g_last_error = "liodom_export_stream_state: inconsistent stream state"; return LIODOM_ERR_HIP;
  }
  const size_t need = state_blob_bytes(h->P, rec.n_points, rec.n_recv);
  *bytes = (int64_t)need;
  if ((int64_t)need > cap) { g_last_error = "liodom_export_stream_state: blob buffer too small"; return LIODOM_ERR_CAPACITY; }
  if (need > prefix) {
    HIP_TRY(hipMemcpyAsync(h->state_stage_host + prefix, h->state_stage + prefix, need - prefix, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  const StateBlobHeader hd = state_header(state_fingerprint(h), (uint64_t)need);
  std::memcpy(blob, &hd, sizeof(hd));
  std::memcpy(static_cast<unsigned char*>(blob) + kStateHeaderBytes, h->state_stage_host + kStateHeaderBytes, need - (size_t)kStateHeaderBytes);
  return LIODOM_OK;
}

int liodom_import_stream_state(liodom_handle_t* h, int stream, const void* blob, int64_t bytes) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (!blob) return LIODOM_ERR_INVALID_ARG;
  SideLocks lk(h, true, true);
  if ((rc = state_quiesce(h))) return rc;
  // every rejection comes before the handle is touched
  const char* why;
  StateBlobRecord rec;
  if ((rc = stream_state_validate(blob, bytes, state_fingerprint(h), h->v.mapping, h->v.edge_cap, h->v.recv_cap, &why, &rec))) {
    g_last_error = std::string("liodom_import_stream_state: ") + why; return rc;
  }
  if ((rc = ensure_state_stage(h))) return rc;
  std::memcpy(h->state_stage_host, blob, (size_t)bytes);
  HIP_TRY(hipMemcpyAsync(h->state_stage, h->state_stage_host, (size_t)bytes, hipMemcpyHostToDevice, h->stream));
  return install_stream_state(h, stream, h->state_stage, rec.n_frames, rec.scan_counter, rec.n_recv);
}

// The attachment of a stream, whichever kind: its writing mapper's map and extents, or its reader's.
static liodom_map* stream_map(const liodom_handle* h, int stream, int* cells_xy, int* cells_z) {
  liodom_map* mp = h->maps.map_of(stream);
  if (mp) { *cells_xy = h->maps.opts(stream).cells_xy; *cells_z = h->maps.opts(stream).cells_z; }
  return mp;
}

int liodom_seed_stream(liodom_handle_t* h, int stream, const double* pose) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (!h->v.mapping) { g_last_error = "liodom_seed_stream: the handle was created with mapping = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (!pose) { g_last_error = "liodom_seed_stream: null pose"; return LIODOM_ERR_INVALID_ARG; }
  if (const Pose7Verdict bad = pose7_check(pose)) {
    g_last_error = bad == kPose7NonFinite ? "liodom_seed_stream: non-finite pose" : "liodom_seed_stream: the quaternion is not normalised (" POSE7_RULE ")";
    return LIODOM_ERR_INVALID_ARG;
  }
  SideLocks lk(h, true, true);
  if ((rc = state_quiesce(h))) return rc;
  if ((rc = ensure_state_stage(h))) return rc;
  const StateBlobRecord rec = state_seed_record(pose);
  const size_t prefix = state_points_offset(h->P);
  // the received map: getLocalMap(T(pose)) of the stream's attachment, planned and gathered straight into the staging blob's
  // received-map section (the window is empty: it follows the counts); its size is read before anything of the stream is touched
  int cxy = 0, cz = 0, n_recv = 0;
  if (liodom_map* mp = stream_map(h, stream, &cxy, &cz)) {
    HIP_TRY(hipMemcpyAsync(mp->d_T, rec.odom, sizeof(double) * 12, hipMemcpyHostToDevice, h->stream));
    if ((rc = map_enqueue_local(mp, mp->d_T, cxy, cz, reinterpret_cast<float4*>(h->state_stage + prefix), h->v.recv_cap, mp->d_out_n, h->stream, 0))) return rc;
    MapState ms;
    HIP_TRY(hipMemcpyAsync(&ms, mp->m.st, sizeof(ms), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (ms.n_result > h->v.recv_cap) { g_last_error = "liodom_seed_stream: the local map at the seed is larger than recv_capacity"; return LIODOM_ERR_CAPACITY; }
    n_recv = ms.n_result < 0 ? 0 : ms.n_result;
  }
  state_seed_prefix(rec, n_recv, h->P, h->state_stage_host);
  HIP_TRY(hipMemcpyAsync(h->state_stage, h->state_stage_host, prefix, hipMemcpyHostToDevice, h->stream));
  return install_stream_state(h, stream, h->state_stage, 0, 0, n_recv);
}

static int copy_edges_out(liodom_handle_t* h, int stream, int eb, hipStream_t q, float* edges_xyzi, int32_t* edge_ring,
                          int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges) {
  int E = 0;
  HIP_TRY(hipMemcpyAsync(&E, &h->v.state[stream].n_edges_buf[eb], sizeof(int), hipMemcpyDeviceToHost, q));
  HIP_TRY(hipStreamSynchronize(q));
  if (n_edges) *n_edges = E;
  if (E > cap) { g_last_error = "edge buffer too small"; return LIODOM_ERR_CAPACITY; }
  if (E == 0) return LIODOM_OK;
  if (edges_xyzi)
    HIP_TRY(hipMemcpyAsync(edges_xyzi, h->v.edges + ((size_t)eb * h->S + stream) * h->v.edge_cap, sizeof(float4) * (size_t)E, hipMemcpyDeviceToHost, q));
  std::vector<int4> meta;
  if (edge_ring || edge_idx || edge_src) {
    meta.resize((size_t)E);
    HIP_TRY(hipMemcpyAsync(meta.data(), h->v.edges_meta + ((size_t)eb * h->S + stream) * h->v.edge_cap, sizeof(int4) * (size_t)E, hipMemcpyDeviceToHost, q));
  }
  HIP_TRY(hipStreamSynchronize(q));
  for (int i = 0; i < E && !meta.empty(); i++) {
    if (edge_ring) edge_ring[i] = meta[i].x;
    if (edge_idx) edge_idx[i] = meta[i].y;
    if (edge_src) edge_src[i] = meta[i].z;
  }
  return LIODOM_OK;
}

int liodom_extract_edges(liodom_handle_t* h, int stream, const float* xyzi, int64_t n, int height,
                         int width, float* edges_xyzi, int32_t* edge_ring, int32_t* edge_idx,
                         int32_t* edge_src, int cap, int* n_edges) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (n < 0 || n > h->v.max_points || (n > 0 && !xyzi)) { g_last_error = "bad point count"; return LIODOM_ERR_CAPACITY; }
  // Extraction side only (mx_x, stream_x, edge buffer kEdgeBufX): safe beside a concurrent
  // liodom_odometry_step of another thread.  An extraction the pipelined replay issued ahead is on the
  // same HIP stream, so the shared ring-split scratch is used in stream order.
  SideLocks lk(h, false, true);
  hipStream_t q = extract_queue(h);
  float4* in = h->stage_in + (size_t)stream * h->v.max_points;
  if (n) HIP_TRY(hipMemcpyAsync(in, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, q));
  rc = launch_extract(h, q, kEdgeBufX, stream, 1, in, 0, (int)n, height, width);
  if (rc) return rc;
  return copy_edges_out(h, stream, kEdgeBufX, q, edges_xyzi, edge_ring, edge_idx, edge_src, cap, n_edges);
}

int liodom_get_edges(liodom_handle_t* h, int stream, float* edges_xyzi, int32_t* edge_ring,
                     int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  SideLocks lk(h, true, false);
  return copy_edges_out(h, stream, h->last_eb[stream], h->stream, edges_xyzi, edge_ring, edge_idx, edge_src, cap, n_edges);
}

static int wait_pose(liodom_handle_t* h, int s0, int count, double* pose_out, liodom_step_info_t* info, int lag = 0, const int32_t* list = nullptr) {
  // zero-copy: k_lm_solve's finalize writes pose + diagnostics into host-mapped memory and
  // releases HostOut.seq; spin on it (an event / memcpy round trip costs ~15 us on this stack)
  bool timed_out = false;
  for (int i = 0; i < count; i++) {
    const int s = list ? (int)list[i] : s0 + i;      // (list: the streams of a subset step, results in list order)
    const int expect = h->scans_enqueued[s] - lag;      // lag 1: the scan before the one enqueued last
    volatile HostOut* ho = h->host_out + (size_t)s * 2 + ((expect - 1) & 1);     // (scan k = expect - 1 publishes into record k & 1)
    unsigned long long spins = 0;
    while (__atomic_load_n(&ho->seq, __ATOMIC_ACQUIRE) != expect) {
      if ((++spins & 0xFFFFull) == 0) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q != hipErrorNotReady && q != hipSuccess) { g_last_error = std::string("stream error while waiting: ") + hipGetErrorString(q); return LIODOM_ERR_HIP; }
        if (q == hipSuccess && __atomic_load_n(&ho->seq, __ATOMIC_ACQUIRE) != expect) { g_last_error = "stream drained without publishing the scan result"; return LIODOM_ERR_HIP; }
      }
    }
    const HostOut* r = h->host_out + (size_t)s * 2 + ((expect - 1) & 1);
    if (pose_out) std::memcpy(pose_out + 7 * i, r->pose, sizeof(double) * 7);
    if (info) info[i] = r->info;
    if (r->info.status & (LIODOM_STATUS_PIPE_TIMEOUT | LIODOM_STATUS_LM_SYNC_TIMEOUT)) timed_out = true;
    // (speculative hand-over: the record carries the scan's verdict — a confirmed scan needs no repair, chain_flush)
    if (s == 0) { h->step.verdict_scan = expect; h->step.verdict_confirmed = r->pad == 1; }
  }
  if (timed_out) {
    // A kernel gave up waiting for another HIP stream of the handle (pipe_wait / ov_wait_*): its workgroups skipped the scan, the
    // published pose is the prediction.  Fail loudly; the switch to event-based dependencies needs both sides of the handle
    // (this caller may hold the odometry side only while another thread extracts): it is applied by liodom_reset(), and every
    // entry point that enqueues work refuses until then (check_usable).
    h->fallback_pending.store(true);
    g_last_error = "a kernel timed out waiting for another kernel of the handle (LIODOM_STATUS_PIPE_TIMEOUT / LM_SYNC_TIMEOUT): kernels are "
                   "serialised across streams (profiler with --pmc, AMD_SERIALIZE_KERNEL, debugger) or the GPU is saturated by another "
                   "process; the scan's result is invalid; call liodom_reset(): the handle then continues in safe mode (no in-kernel waits)";
    return LIODOM_ERR_HIP;
  }
  return LIODOM_OK;
}

int liodom_odometry_step(liodom_handle_t* h, int stream, const float* edges_xyzi, int n_edges,
                         double stamp, double* pose_out, liodom_step_info_t* info) {
  (void)stamp;
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (n_edges < 0 || n_edges > h->v.edge_cap || (n_edges > 0 && !edges_xyzi)) { g_last_error = "edge count exceeds capacity"; return LIODOM_ERR_CAPACITY; }
  // Odometry side only (mx_o, h->stream, edge buffer 0): safe beside a concurrent liodom_extract_edges.
  SideLocks lk(h, true, false);
  if ((rc = tickets_idle(h))) return rc;
  rc = drain_pipeline(h);
  if (rc) return rc;
  if (n_edges)
    HIP_TRY(hipMemcpyAsync(h->v.edges + (size_t)stream * h->v.edge_cap, edges_xyzi, sizeof(float4) * (size_t)n_edges, hipMemcpyHostToDevice, h->stream));
  {
    ProfScope ps(h, KID_OTHER);
    hipLaunchKernelGGL(k_set_edges, dim3(1), dim3(64), 0, h->stream, h->v, stream, n_edges, 0);
  }
  rc = launch_odometry(h, 0, stream, 1);
  if (rc) return rc;
  return wait_pose(h, stream, 1, pose_out, info);
}

// ---- device-resident hand-off between the two sides (the reference's feature queue without the cloud leaving HBM) ----
// The HIP half of a page-locked staging ring (StagingRing, edge_pipe.h; ev: its three events), for XYZI scans (h->pin) and for polar
// blobs (h->pol_pin) alike.  Extraction side (mx_x held).
// The upload that last read slot r (three scans ago) must have left it.
static int ring_slot_wait(StagingRing& ring, hipEvent_t* ev, int r) {
  if (ring.valid[r]) { HIP_TRY(hipEventSynchronize(ev[r])); ring.valid[r] = false; }
  return LIODOM_OK;
}
// liodom_scan_buffer*: the slot the caller assembles the next scan in.
static int ring_hand_out(StagingRing& ring, hipEvent_t* ev, void** out) {
  if (int rc = ring_slot_wait(ring, ev, ring.next)) return rc;
  *out = ring.slot(ring.next);
  return LIODOM_OK;
}
// Where the upload of `bytes` at *src starts from.  An upload is asynchronous when it starts from page-locked memory: a slot of the
// ring itself (liodom_scan_buffer*), or a buffer the caller registered (liodom_pin_host_buffer) — which must stay untouched until
// liodom_wait_edges / liodom_odometry_step_device of the ticket has returned.  A pageable source is copied through the ring (*src
// then points into it).  *used: the ring slot the upload reads, -1 for a registered buffer; ring_uploaded takes it.
static int ring_source(StagingRing& ring, hipEvent_t* ev, const void** src, size_t bytes, int* used) {
  const int own = ring.owns(*src);
  bool pinned = own >= 0;
  if (!pinned) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, *src) == hipSuccess) pinned = attr.type == hipMemoryTypeHost;
    else (void)hipGetLastError();                    // (unregistered pageable memory: not an error)
  }
  *used = ring.source_slot(own, pinned);
  if (!pinned) {
    if (int rc = ring_slot_wait(ring, ev, *used)) return rc;
    std::memcpy(ring.slot(*used), *src, bytes);
    *src = ring.slot(*used);
  }
  return LIODOM_OK;
}
// The upload has been enqueued on q: the ring slot it reads may be refilled once it has left it.
static int ring_uploaded(StagingRing& ring, hipEvent_t* ev, int used, hipStream_t q) {
  if (used < 0) return LIODOM_OK;
  HIP_TRY(hipEventRecord(ev[used], q));
  ring.upload_recorded(used);
  return LIODOM_OK;
}

static int ensure_pin_ring(liodom_handle* h) {
  if (h->pin.base) return LIODOM_OK;
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, sizeof(float4) * (size_t)kEdgePipeBufs * (size_t)h->v.max_points, hipHostMallocDefault));
  h->pin.bind(p, sizeof(float4) * (size_t)h->v.max_points);
  for (int b = 0; b < kEdgePipeBufs; b++) HIP_TRY(hipEventCreateWithFlags(&h->ev_pin[b], hipEventDisableTiming));
  return LIODOM_OK;
}

int liodom_scan_buffer(liodom_handle_t* h, int stream, float** xyzi, int64_t* capacity_points) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!xyzi) return LIODOM_ERR_INVALID_ARG;
  if (h->S != 1) { g_last_error = "liodom_scan_buffer: one-stream handles only"; return LIODOM_ERR_UNSUPPORTED; }
  SideLocks lk(h, false, true);
  if ((rc = ensure_pin_ring(h))) return rc;
  if ((rc = ring_hand_out(h->pin, h->ev_pin, reinterpret_cast<void**>(xyzi)))) return rc;
  if (capacity_points) *capacity_points = h->v.max_points;
  return LIODOM_OK;
}

// The two ends of liodom_extract_edges_device that its polar form shares.  Extraction side (mx_x held).
// Is the hand-off slot of the next extraction free?  (EdgePipe::ticket_slot says why each refusal is what it is.)
static int ticket_slot_free(liodom_handle* h) {
  switch (h->pipe.ticket_slot()) {
    case kSlotFree: return LIODOM_OK;
    case kSlotExtractionAhead:
      g_last_error = "edge extraction by ticket: a pipelined replay of this handle has an extraction issued ahead: call liodom_sync() first";
      return LIODOM_ERR_NEEDS_SYNC;
    case kSlotReplayLive:      // (not BUSY: a caller that keeps the cloud and retries would spin forever)
      g_last_error = "edge extraction by ticket: scans of a pipelined replay (liodom_process_resident / liodom_replay_*) are still in the edge buffers: call liodom_sync() first";
      return LIODOM_ERR_NEEDS_SYNC;
    case kSlotsFull: break;
  }
  g_last_error = "edge extraction by ticket: all hand-off slots hold edge clouds no liodom_odometry_step_device has taken yet";
  return LIODOM_ERR_BUSY;
}
// The extraction of the cloud at `in` (device, its upload or projection enqueued on q) into the free hand-off slot, and its ticket.
static int ticket_extract(liodom_handle* h, hipStream_t q, int stream, const float4* in, int n, int height, int width, liodom_edge_ticket_t* ticket) {
  const EdgeTicketDraft t = h->pipe.ticket_draft();
  const int eb = t.slot;
  unsigned int* host_seq = h->v.host_edges_hdr ? h->v.host_edges_hdr + eb : nullptr;
  // (the slot is free: the odometry that last read buffer eb has been collected, i.e. has completed — no wait on the device,
  //  which would depend on when the other thread submits its next scan)
  unsigned int* const dev_flag = h->plan.use_flags ? h->v.pipe_flags + eb : (unsigned int*)nullptr;
  int rc = launch_extract(h, q, eb, stream, 1, in, 0, n, height, width, 0u, 1, dev_flag, host_seq, t.seq);
  if (rc) return rc;
  if (!h->plan.use_flags) HIP_TRY(hipEventRecord(h->ev_edges[eb], q));
  h->pipe.ticket_issued(t);
  ticket->seq = t.seq; ticket->slot = eb; ticket->stream = stream; ticket->reserved = 0;
  return LIODOM_OK;
}

int liodom_extract_edges_device(liodom_handle_t* h, int stream, const float* xyzi, int64_t n, int height, int width,
                                liodom_edge_ticket_t* ticket) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (!ticket) return LIODOM_ERR_INVALID_ARG;
  if (h->S != 1) { g_last_error = "liodom_extract_edges_device: one-stream handles only (lock-step handles advance all streams together: liodom_process_resident)"; return LIODOM_ERR_UNSUPPORTED; }
  if (n < 0 || n > h->v.max_points || (n > 0 && !xyzi)) { g_last_error = "bad point count"; return LIODOM_ERR_CAPACITY; }
  SideLocks lk(h, false, true);                      // extraction side only: safe beside a concurrent liodom_odometry_step_device
  if ((rc = ticket_slot_free(h))) return rc;
  hipStream_t q = extract_queue(h);
  float4* in = h->stage_in + (size_t)stream * h->v.max_points;
  if (n) {
    if ((rc = ensure_pin_ring(h))) return rc;
    const void* src = xyzi;
    int used = -1;
    if ((rc = ring_source(h->pin, h->ev_pin, &src, sizeof(float4) * (size_t)n, &used))) return rc;
    HIP_TRY(hipMemcpyAsync(in, src, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, q));
    if ((rc = ring_uploaded(h->pin, h->ev_pin, used, q))) return rc;
  }
  return ticket_extract(h, q, stream, in, (int)n, height, width, ticket);
}

int liodom_wait_edges(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, float* edges_xyzi, int32_t* edge_ring,
                      int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges) {
  if (!h || !ticket) return LIODOM_ERR_INVALID_ARG;
  int rc = check_stream(h, ticket->stream);
  if (rc) return rc;
  const int eb = ticket->slot;
  if (eb < 0 || eb >= kEdgePipeBufs || !h->host_edges_hdr) { g_last_error = "liodom_wait_edges: bad ticket"; return LIODOM_ERR_INVALID_ARG; }
  // No lock: the slot's mirror is rewritten only by an extraction issued after the ticket has been consumed
  // (liodom_odometry_step_device), which the caller orders behind this call.
  volatile unsigned int* hs = h->host_edges_hdr + eb;
  unsigned long long spins = 0;
  while ((int)(__atomic_load_n(hs, __ATOMIC_ACQUIRE) - ticket->seq) < 0) {
    if ((++spins & 0xFFFFull) == 0) {
      const hipError_t q = hipStreamQuery(extract_queue(h));
      if (q != hipErrorNotReady && q != hipSuccess) { g_last_error = std::string("stream error while waiting for edges: ") + hipGetErrorString(q); return LIODOM_ERR_HIP; }
      if (q == hipSuccess && (int)(__atomic_load_n(hs, __ATOMIC_ACQUIRE) - ticket->seq) < 0) { g_last_error = "extraction stream drained without publishing the ticket's edges"; return LIODOM_ERR_HIP; }
    }
  }
  if (__atomic_load_n(hs, __ATOMIC_ACQUIRE) != ticket->seq) { g_last_error = "liodom_wait_edges: the ticket's slot has been reused (stale ticket)"; return LIODOM_ERR_INVALID_ARG; }
  const int E = (int)h->host_edges_hdr[kEdgePipeBufs + eb];
  if (n_edges) *n_edges = E;
  if (E > cap && (edges_xyzi || edge_ring || edge_idx || edge_src)) { g_last_error = "edge buffer too small"; return LIODOM_ERR_CAPACITY; }
  const float4* he = h->host_edges + (size_t)eb * h->v.edge_cap;
  const int4* hm = h->host_edges_meta + (size_t)eb * h->v.edge_cap;
  if (edges_xyzi && E) std::memcpy(edges_xyzi, he, sizeof(float4) * (size_t)E);
  if (edge_ring || edge_idx || edge_src) {
    for (int i = 0; i < E; i++) {
      if (edge_ring) edge_ring[i] = hm[i].x;
      if (edge_idx) edge_idx[i] = hm[i].y;
      if (edge_src) edge_src[i] = hm[i].z;
    }
  }
  return LIODOM_OK;
}

int liodom_odometry_submit_device(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, double stamp) {
  (void)stamp;
  if (!h || !ticket) return LIODOM_ERR_INVALID_ARG;
  int rc = check_stream(h, ticket->stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  const int eb = ticket->slot;
  if (h->S != 1 || eb < 0 || eb >= kEdgePipeBufs) { g_last_error = "liodom_odometry_submit_device: bad ticket"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);                      // odometry side only: safe beside a concurrent liodom_extract_edges_device
  switch (h->pipe.submit_check(ticket->seq, eb)) {
    case kSubmitOk: break;
    case kSubmitStale:
      g_last_error = "liodom_odometry_submit_device: stale or unknown ticket (already consumed, or voided by liodom_reset)";
      return LIODOM_ERR_INVALID_ARG;
    case kSubmitAlready: g_last_error = "liodom_odometry_submit_device: ticket already submitted"; return LIODOM_ERR_INVALID_ARG;
    case kSubmitTwoInFlight:
      g_last_error = "liodom_odometry_submit_device: two scans are in flight: collect a pose first (liodom_odometry_collect)";
      return LIODOM_ERR_BUSY;
  }
  rc = enqueue_pipeline_odometry(h, eb, ticket->seq);
  if (rc) return rc;
  h->pipe.submitted(eb);
  return LIODOM_OK;
}

int liodom_odometry_collect(liodom_handle_t* h, int stream, double* pose_out, liodom_step_info_t* info) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  SideLocks lk(h, true, false);
  const int lag = h->pipe.collect_lag();
  if (lag < 0) { g_last_error = "liodom_odometry_collect: no scan has been submitted"; return LIODOM_ERR_INVALID_ARG; }
  rc = wait_pose(h, stream, 1, pose_out, info, lag);      // the oldest of the (at most two) scans in flight
  h->pipe.collected();
  return rc;
}

int liodom_odometry_step_device(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, double stamp, double* pose_out,
                                liodom_step_info_t* info) {
  if (!h || !ticket) return LIODOM_ERR_INVALID_ARG;
  if (h->pipe.odo_pending != 0) { g_last_error = "liodom_odometry_step_device: a submitted scan has not been collected (liodom_odometry_collect)"; return LIODOM_ERR_BUSY; }
  const int rc = liodom_odometry_submit_device(h, ticket, stamp);
  if (rc) return rc;
  return liodom_odometry_collect(h, ticket->stream, pose_out, info);
}

// liodom_process_scan and its polar form.  Both take the two sides — they use the extraction scratch on the odometry stream — and
// start with scan_alone; once the cloud is on its way into the stream's staging block on the odometry stream, scan_tail does the rest.
static int scan_alone(liodom_handle* h) {
  if (int rc = tickets_idle(h)) return rc;
  return drain_pipeline(h);           // nothing issued ahead on the extraction stream may still use that scratch
}
static int scan_tail(liodom_handle* h, int stream, int n, int height, int width, double* pose_out, liodom_step_info_t* info) {
  int rc = launch_extract(h, h->stream, 0, stream, 1, h->stage_in + (size_t)stream * h->v.max_points, 0, n, height, width);
  if (rc) return rc;
  rc = launch_odometry(h, 0, stream, 1);
  if (rc) return rc;
  return wait_pose(h, stream, 1, pose_out, info);
}

int liodom_process_scan(liodom_handle_t* h, int stream, const float* xyzi, int64_t n, int height,
                        int width, double stamp, double* pose_out, liodom_step_info_t* info) {
  (void)stamp;
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (n < 0 || n > h->v.max_points || (n > 0 && !xyzi)) { g_last_error = "bad point count"; return LIODOM_ERR_CAPACITY; }
  SideLocks lk(h, true, true);
  if ((rc = scan_alone(h))) return rc;
  if (n) HIP_TRY(hipMemcpyAsync(h->stage_in + (size_t)stream * h->v.max_points, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  return scan_tail(h, stream, (int)n, height, width, pose_out, info);
}

// ---- polar scans: the sensor's counts go up, the projection to XYZI runs on the device (kernels_polar.h) ----
static int polar_sizes_valid(const liodom_polar_geometry_t* g) {
  if (!g) return LIODOM_ERR_INVALID_ARG;
  if ((g->range_bits != 16 && g->range_bits != 32) || (g->intensity_bits != 0 && g->intensity_bits != 8 && g->intensity_bits != 16) ||
      g->height < 1 || g->height > kPolarMaxHeight || g->width < 1) {
    g_last_error = "polar geometry: range_bits must be 16 or 32, intensity_bits 0, 8 or 16, 1 <= height <= 2048, width >= 1";
    return LIODOM_ERR_INVALID_ARG;
  }
  return LIODOM_OK;
}

int liodom_polar_layout(const liodom_polar_geometry_t* geom, liodom_polar_layout_t* out) {
  if (!out) return LIODOM_ERR_INVALID_ARG;
  if (int rc = polar_sizes_valid(geom)) return rc;
  long long r, i, t;
  polar_sections(geom->height, geom->width, geom->range_bits, geom->intensity_bits, &r, &i, &t);
  out->tick_offset = 0; out->range_offset = r; out->intensity_offset = i; out->total_bytes = t;
  return LIODOM_OK;
}

int liodom_set_polar_geometry(liodom_handle_t* h, const liodom_polar_geometry_t* g) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = polar_sizes_valid(g))) return rc;
  if (g->ticks < 1 || !g->cos_alt || !g->sin_alt || !g->cos_baz || !g->sin_baz || !g->cos_enc || !g->sin_enc) {
    g_last_error = "polar geometry: a table is null or ticks < 1";
    return LIODOM_ERR_INVALID_ARG;
  }
  if ((long long)g->height * g->width > (long long)h->v.max_points) { g_last_error = "polar geometry: height * width exceeds max_points"; return LIODOM_ERR_CAPACITY; }
  SideLocks lk(h, true, true);
  if ((rc = tickets_idle(h))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream_x));       // a projection in flight reads the tables and the staging slots replaced below
  HIP_TRY(sync_odometry(h));
  PolarView pv{};
  pv.H = g->height; pv.W = g->width; pv.T = g->ticks; pv.n = g->height * g->width;
  pv.range_bytes = g->range_bits / 8; pv.inten_bytes = g->intensity_bits / 8;
  pv.order = h->v.lidar_type == 1 ? 1 : 0;
  pv.range_unit = g->range_unit; pv.beam_origin = g->beam_origin;
  polar_sections(pv.H, pv.W, g->range_bits, g->intensity_bits, &pv.range_off, &pv.inten_off, &pv.blob_bytes);
  // the tables as the kernel reads them: one float4 per row, one float2 per tick
  const size_t beam_bytes = sizeof(float4) * (size_t)pv.H, enc_bytes = sizeof(float2) * (size_t)pv.T;
  std::vector<float> tab((beam_bytes + enc_bytes) / sizeof(float));
  for (int r = 0; r < pv.H; r++) { tab[4 * r] = g->cos_alt[r]; tab[4 * r + 1] = g->sin_alt[r]; tab[4 * r + 2] = g->cos_baz[r]; tab[4 * r + 3] = g->sin_baz[r]; }
  for (int t = 0; t < pv.T; t++) { tab[4 * (size_t)pv.H + 2 * (size_t)t] = g->cos_enc[t]; tab[4 * (size_t)pv.H + 2 * (size_t)t + 1] = g->sin_enc[t]; }
  // everything new first: a failure leaves the handle as it was
  void *tables = nullptr, *stage = nullptr, *pin = nullptr;
  hipError_t e = hipMalloc(&tables, beam_bytes + enc_bytes);
  if (e == hipSuccess) e = hipMalloc(&stage, (size_t)kEdgePipeBufs * (size_t)pv.blob_bytes);
  if (e == hipSuccess) e = hipHostMalloc(&pin, (size_t)kEdgePipeBufs * (size_t)pv.blob_bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMemcpy(tables, tab.data(), beam_bytes + enc_bytes, hipMemcpyHostToDevice);
  for (int b = 0; b < kEdgePipeBufs && e == hipSuccess; b++) if (!h->ev_polpin[b]) e = hipEventCreateWithFlags(&h->ev_polpin[b], hipEventDisableTiming);
  if (e != hipSuccess) {
    if (tables) (void)hipFree(tables);
    if (stage) (void)hipFree(stage);
    if (pin) (void)hipHostFree(pin);
    g_last_error = std::string("liodom_set_polar_geometry: ") + hipGetErrorString(e);
    return LIODOM_ERR_HIP;
  }
  if (h->pol_tables) (void)hipFree(h->pol_tables);
  if (h->pol_stage) (void)hipFree(h->pol_stage);
  if (h->pol_pin.base) (void)hipHostFree(h->pol_pin.base);
  h->pol_tables = tables; h->pol_stage = static_cast<unsigned char*>(stage);
  h->pol_pin.bind(pin, (size_t)pv.blob_bytes);      // (a new ring: it starts at slot 0 with no upload to wait for)
  pv.beam = static_cast<const float4*>(tables);
  pv.enc = reinterpret_cast<const float2*>(static_cast<const unsigned char*>(tables) + beam_bytes);
  h->pol = pv;
  h->pol_stage_next = 0;
  h->polar = true;
  return LIODOM_OK;
}

static int polar_ready(liodom_handle* h, const void* blob) {
  if (!h->polar) { g_last_error = "no polar geometry has been set (liodom_set_polar_geometry)"; return LIODOM_ERR_UNSUPPORTED; }
  if (!blob) return LIODOM_ERR_INVALID_ARG;
  return LIODOM_OK;
}
// Upload of a blob into the next compact staging slot and its projection into dst (device, n points), both on q.  Extraction side.
static int polar_upload_project(liodom_handle* h, hipStream_t q, const void* blob, float4* dst) {
  const PolarView& pv = h->pol;
  unsigned char* st = h->pol_stage + (size_t)h->pol_stage_next * (size_t)pv.blob_bytes;
  h->pol_stage_next = (h->pol_stage_next + 1) % kEdgePipeBufs;
  HIP_TRY(hipMemcpyAsync(st, blob, (size_t)pv.blob_bytes, hipMemcpyHostToDevice, q));
  {
    ProfScope ps(h, KID_OTHER, q);
    hipLaunchKernelGGL(k_polar_project, dim3(cdiv(pv.n, kPolarTile)), dim3(kPolarThreads), polar_lds_bytes(pv.H), q, pv, st, dst);
  }
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}

int liodom_project_polar(liodom_handle_t* h, const void* blob, float* xyzi_out) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = polar_ready(h, blob))) return rc;
  if (!xyzi_out) return LIODOM_ERR_INVALID_ARG;
  SideLocks lk(h, false, true);
  hipStream_t q = extract_queue(h);
  if ((rc = polar_upload_project(h, q, blob, h->stage_in))) return rc;
  HIP_TRY(hipMemcpyAsync(xyzi_out, h->stage_in, sizeof(float4) * (size_t)h->pol.n, hipMemcpyDeviceToHost, q));
  HIP_TRY(hipStreamSynchronize(q));
  return LIODOM_OK;
}

int liodom_upload_scan_polar(liodom_handle_t* h, int stream, int slot, const void* blob) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = polar_ready(h, blob))) return rc;
  if (!h->resident || slot < 0 || slot >= h->n_slots) { g_last_error = "bad resident slot"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, false, true);
  hipStream_t q = extract_queue(h);
  if ((rc = polar_upload_project(h, q, blob, h->resident + ((size_t)slot * h->S + stream) * (size_t)h->v.max_points))) return rc;
  HIP_TRY(hipStreamSynchronize(q));                  // like liodom_upload_scan: the blob is the caller's again on return
  return LIODOM_OK;
}

int liodom_process_scan_polar(liodom_handle_t* h, int stream, const void* blob, double stamp, double* pose_out, liodom_step_info_t* info) {
  (void)stamp;
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if ((rc = polar_ready(h, blob))) return rc;
  SideLocks lk(h, true, true);
  if ((rc = scan_alone(h))) return rc;
  if ((rc = polar_upload_project(h, h->stream, blob, h->stage_in + (size_t)stream * h->v.max_points))) return rc;
  return scan_tail(h, stream, h->pol.n, h->pol.H, h->pol.W, pose_out, info);
}

int liodom_scan_buffer_polar(liodom_handle_t* h, int stream, void** blob, int64_t* bytes) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!blob) return LIODOM_ERR_INVALID_ARG;
  if (!h->polar) { g_last_error = "no polar geometry has been set (liodom_set_polar_geometry)"; return LIODOM_ERR_UNSUPPORTED; }
  if (h->S != 1) { g_last_error = "liodom_scan_buffer_polar: one-stream handles only"; return LIODOM_ERR_UNSUPPORTED; }
  SideLocks lk(h, false, true);
  if ((rc = ring_hand_out(h->pol_pin, h->ev_polpin, blob))) return rc;
  if (bytes) *bytes = h->pol.blob_bytes;
  return LIODOM_OK;
}

int liodom_extract_edges_device_polar(liodom_handle_t* h, int stream, const void* blob, liodom_edge_ticket_t* ticket) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if ((rc = polar_ready(h, blob))) return rc;
  if (!ticket) return LIODOM_ERR_INVALID_ARG;
  if (h->S != 1) { g_last_error = "liodom_extract_edges_device_polar: one-stream handles only"; return LIODOM_ERR_UNSUPPORTED; }
  SideLocks lk(h, false, true);
  if ((rc = ticket_slot_free(h))) return rc;
  hipStream_t q = extract_queue(h);
  int used = -1;      // (the source rules of liodom_extract_edges_device, over the blob ring)
  if ((rc = ring_source(h->pol_pin, h->ev_polpin, &blob, (size_t)h->pol.blob_bytes, &used))) return rc;
  float4* in = h->stage_in + (size_t)stream * h->v.max_points;
  if ((rc = polar_upload_project(h, q, blob, in))) return rc;
  if ((rc = ring_uploaded(h->pol_pin, h->ev_polpin, used, q))) return rc;
  return ticket_extract(h, q, stream, in, h->pol.n, h->pol.H, h->pol.W, ticket);
}

// Rebuilds the kNN structure of one stream from window ++ received map without appending a frame.
static int rebuild_search_structure(liodom_handle* h, int stream) {
  const DevView& v = h->v;
  hipLaunchKernelGGL(k_hash_reset, dim3(64), dim3(256), 0, h->stream, v, stream);
  hipLaunchKernelGGL(k_hash_reset_done, dim3(1), dim3(1), 0, h->stream, v, stream);
  // (a mapping handle: no voxel filter follows the hash step)
  StepPlan plan;
  plan_full_rebuild(h->plan, &plan);
  StepData d;
  d.s0 = stream; d.count = 1; d.eb = -1;
  return issue_plan(h, plan, d);
}

int liodom_set_received_map(liodom_handle_t* h, int stream, const float* xyzi, int64_t n) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.mapping) { g_last_error = "liodom_set_received_map: the handle was created with mapping = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (n < 0 || (n > 0 && !xyzi)) return LIODOM_ERR_INVALID_ARG;
  if (n > h->v.recv_cap) { g_last_error = "liodom_set_received_map: cloud larger than recv_capacity"; return LIODOM_ERR_CAPACITY; }
  SideLocks lk(h, true, false);
  const int ni = (int)n;
  if (n) HIP_TRY(hipMemcpyAsync(h->v.recv_pts + (size_t)stream * h->v.recv_cap, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(&h->v.state[stream].n_recv, &ni, sizeof(int), hipMemcpyHostToDevice, h->stream));
  rc = rebuild_search_structure(h, stream);
  if (rc) return rc;
  HIP_TRY(sync_odometry(h));        // xyzi / ni are the caller's and this frame's memory
  return LIODOM_OK;
}

int liodom_set_imu_orientation(liodom_handle_t* h, int stream, const double* q_xyzw) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!q_xyzw) return LIODOM_ERR_INVALID_ARG;
  // what would poison the stream is refused before anything is touched (liodom_seed_stream's rule for its pose): tf's setRotation
  // divides by |q|^2, so a zero or non-finite quaternion makes the prediction — and every pose after it — NaN, with no status bit.
  // A non-unit quaternion is fine: tf divides the norm out.
  double nn = 0.0;
  for (int i = 0; i < 4; i++) {
    if (!std::isfinite(q_xyzw[i])) { g_last_error = "liodom_set_imu_orientation: non-finite quaternion"; return LIODOM_ERR_INVALID_ARG; }
    nn += q_xyzw[i] * q_xyzw[i];
  }
  // (|q|^2 as tf forms it: a norm so small or so large that it underflows to 0 or overflows counts as zero / non-finite)
  if (!(nn > 0.0) || !std::isfinite(nn) || !std::isfinite(2.0 / nn)) { g_last_error = "liodom_set_imu_orientation: quaternion of zero norm"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);
  // pageable-memory async copies are staged by the runtime before the call returns
  HIP_TRY(hipMemcpyAsync(h->v.imu_q + (size_t)stream * 4, q_xyzw, sizeof(double) * 4, hipMemcpyHostToDevice, h->stream));
  return LIODOM_OK;
}

int liodom_set_laser_to_base(liodom_handle_t* h, const double* T) {
  if (!h || !T) return LIODOM_ERR_INVALID_ARG;
  if (int rc = enter(h)) return rc;
  SideLocks lk(h, true, true);
  for (int k = 0; k < 12; k++) h->v.laser_to_base[k] = T[k];      // kernels take the view by value
  return LIODOM_OK;
}

int liodom_get_received_map(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.mapping) { if (n_points) *n_points = 0; return LIODOM_OK; }
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  int n = 0;
  HIP_TRY(hipMemcpy(&n, &h->v.state[stream].n_recv, sizeof(int), hipMemcpyDeviceToHost));
  if (n_points) *n_points = n;
  if (n > cap) { g_last_error = "received-map buffer too small"; return LIODOM_ERR_CAPACITY; }
  if (n && xyzi) HIP_TRY(hipMemcpy(xyzi, h->v.recv_pts + (size_t)stream * h->v.recv_cap, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

void liodom_mapper_options_default(liodom_mapper_options_t* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->cells_xy = 2; o->cells_z = 1;      // liodom_mapping_node.cc:130-134
}

// The HIP half of a transition of h->maps (map_attach.h), in the order the record names.  The odometry stream has drained (the
// callers synchronise).
static int carry_out(liodom_handle* h, int stream, const AttachEffects<liodom_map>& e) {
  if (liodom_map* m = e.move_in) {
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (m->own_stream) { (void)hipStreamDestroy(m->stream); m->own_stream = false; }
    m->stream = h->stream;
  }
  const int4 none = make_int4(0, 0, 0, 0), sel = make_int4(e.sel[0], e.sel[1], e.sel[2], e.sel[3]);
  if (e.sel_cleared) HIP_TRY(hipMemcpy(h->reader_sel + stream, &none, sizeof(none), hipMemcpyHostToDevice));
  if (e.own_again) HIP_TRY(map_own_stream(e.own_again));
  if (e.sel_written) HIP_TRY(hipMemcpy(h->reader_sel + stream, &sel, sizeof(sel), hipMemcpyHostToDevice));
  if (e.lag_on >= 0 && h->lag_on) HIP_TRY(hipMemcpy(h->lag_on + stream, &e.lag_on, sizeof(int), hipMemcpyHostToDevice));
  return LIODOM_OK;
}

int liodom_attach_map_reader(liodom_handle_t* h, int stream, liodom_map_t* m, int cells_xy, int cells_z) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.mapping) { g_last_error = "liodom_attach_map_reader: the handle was created with mapping = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (!m) return liodom_attach_mapper_ex(h, stream, nullptr, nullptr);
  // every rejection comes before the attachment is touched
  if (m->device != h->config.device) { g_last_error = "liodom_attach_map_reader: map and handle live on different devices"; return LIODOM_ERR_INVALID_ARG; }
  if (cells_xy < 0 || cells_z < 0) { g_last_error = "liodom_attach_map_reader: negative extent"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);
  switch (h->maps.reader_check(stream, m)) {
    case kAttachMapIsWritten: g_last_error = "liodom_attach_map_reader: the map is attached writing (liodom_attach_mapper): a map is read or written, not both"; return LIODOM_ERR_INVALID_ARG;
    case kAttachOtherHandle: g_last_error = "liodom_attach_map_reader: the map is attached to another handle"; return LIODOM_ERR_INVALID_ARG;
    default: break;
  }
  HIP_TRY(sync_odometry(h));
  if (!h->reader_sel) {      // one int4 per stream, from the first reader on
    if ((rc = dev_alloc(h, &h->reader_sel, (size_t)h->S))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (h->maps.hits_on(stream) && (rc = map_keep_occ(m))) return rc;      // (hit records: the kept occupancy, sized once)
  liodom_mapper_options_t o{};
  o.cells_xy = cells_xy; o.cells_z = cells_z;
  return carry_out(h, stream, h->maps.attach(stream, m, true, o));
}

static_assert(sizeof(liodom_map_hit_t) == liodom_dev::kMapHitRecordBytes, "k_map_hit_rows writes the record as eight 16-byte stores");
int liodom_set_map_hits(liodom_handle_t* h, int stream, int radius) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.mapping) { g_last_error = "liodom_set_map_hits: the handle was created with mapping = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (radius < -1 || radius > 1) { g_last_error = "liodom_set_map_hits: radius is -1 (off), 0 or 1"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, true);
  if ((rc = state_quiesce(h))) return rc;
  if (!h->hit_log) {
    if (radius < 0) return LIODOM_OK;      // never on: nothing to switch off
    // the log and the per-stream radius, from the first enabling call on
    if ((rc = dev_alloc(h, &h->hit_log, (size_t)h->S * (size_t)h->v.pose_log_cap))) return rc;
    if ((rc = dev_alloc(h, &h->hit_radius, (size_t)h->S, 0xff))) return rc;      // (all -1)
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  liodom_map* rd = h->maps.reader(stream);
  if (radius >= 0 && rd && (rc = map_keep_occ(rd))) return rc;
  h->maps.set_hits(stream, radius);
  HIP_TRY(hipMemcpy(h->hit_radius + stream, &radius, sizeof(int), hipMemcpyHostToDevice));
  return LIODOM_OK;
}

int liodom_get_map_hit_log(liodom_handle_t* h, int stream, int first, int count, liodom_map_hit_t* out) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->hit_log) { g_last_error = "liodom_get_map_hit_log: liodom_set_map_hits has never been switched on for this handle"; return LIODOM_ERR_UNSUPPORTED; }
  if (first < 0 || count < 0 || first + count > h->v.pose_log_cap) { g_last_error = "pose log range"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  if (out && count)
    HIP_TRY(hipMemcpy(out, h->hit_log + (size_t)stream * h->v.pose_log_cap + first, sizeof(liodom_map_hit_t) * (size_t)count, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

int liodom_attach_mapper_ex(liodom_handle_t* h, int stream, liodom_map_t* m, const liodom_mapper_options_t* options) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.mapping) { g_last_error = "liodom_attach_mapper: the handle was created with mapping = 0"; return LIODOM_ERR_UNSUPPORTED; }
  liodom_mapper_options_t o;
  liodom_mapper_options_default(&o);
  if (options) o = *options;
  if (m) {      // every rejection comes before the attachment is touched
    if (m->device != h->config.device) { g_last_error = "liodom_attach_mapper: map and handle live on different devices"; return LIODOM_ERR_INVALID_ARG; }
    if (o.cells_xy < 0 || o.cells_z < 0 || o.lag < 0 || o.lag > 1 || o.prune_period < 0 || o.keep_cells_xy < 0 || o.keep_cells_z < 0) {
      g_last_error = "liodom_attach_mapper_ex: negative extent or period, or lag not 0 / 1"; return LIODOM_ERR_INVALID_ARG;
    }
    // auto-prune must not change getLocalMap(pose_k): the keep box has to hold every key that visit reaches — its square, and
    // its z column, whose extent the reference takes from the xy size (map.cc:175-178)
    if (o.prune_period > 0 && !(o.keep_cells_xy >= o.cells_xy && (double)o.keep_cells_z * m->cfg.voxel_zsize >= (double)o.cells_z * m->cfg.voxel_xysize)) {
      g_last_error = "liodom_attach_mapper_ex: prune_period needs keep_cells_xy >= cells_xy and keep_cells_z * voxel_zsize >= cells_z * voxel_xysize";
      return LIODOM_ERR_INVALID_ARG;
    }
  }
  SideLocks lk(h, true, false);
  if (m && h->maps.writer_check(stream, m) == kAttachMapIsRead) {
    g_last_error = "liodom_attach_mapper: the map is attached reading (liodom_attach_map_reader): a map is read or written, not both"; return LIODOM_ERR_INVALID_ARG;
  }
  HIP_TRY(sync_odometry(h));
  if (m && o.lag == 1 && !h->lag_stash) {      // one edge_cap frame per stream, from the first lagged attach on
    if ((rc = dev_alloc(h, &h->lag_stash, (size_t)h->S * (size_t)h->v.edge_cap))) return rc;
    if ((rc = dev_alloc(h, &h->lag_stash_n, (size_t)h->S))) return rc;
    if ((rc = dev_alloc(h, &h->lag_on, (size_t)h->S))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (m && o.prune_period > 0 && (rc = map_ensure_prune(m))) return rc;
  return carry_out(h, stream, m ? h->maps.attach(stream, m, false, o) : h->maps.detach(stream));
}

int liodom_attach_mapper(liodom_handle_t* h, int stream, liodom_map_t* m, int cells_xy, int cells_z) {
  liodom_mapper_options_t o;
  liodom_mapper_options_default(&o);
  o.cells_xy = cells_xy; o.cells_z = cells_z;
  return liodom_attach_mapper_ex(h, stream, m, &o);
}

int liodom_alloc_resident(liodom_handle_t* h, int n_slots) {
  if (!h || n_slots < 1) return LIODOM_ERR_INVALID_ARG;
  int rc0 = enter(h);
  if (rc0) return rc0;
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));       // an extraction issued ahead may still read the old buffer
  HIP_TRY(sync_odometry(h));
  h->pipe.ahead_clear();
  if (h->resident) { hipFree(h->resident); h->resident = nullptr; h->n_slots = 0; }
  const size_t bytes = sizeof(float4) * (size_t)h->S * (size_t)n_slots * (size_t)h->v.max_points;
  void* raw = nullptr;
  HIP_TRY(hipMalloc(&raw, bytes));
  h->resident = static_cast<float4*>(raw);
  h->n_slots = n_slots;
  return LIODOM_OK;
}

int liodom_upload_scan(liodom_handle_t* h, int stream, int slot, const float* xyzi, int64_t n) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->resident || slot < 0 || slot >= h->n_slots || n < 0 || n > h->v.max_points) { g_last_error = "bad resident slot"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, false, true);
  float4* dst = h->resident + ((size_t)slot * h->S + stream) * (size_t)h->v.max_points;
  if (n) HIP_TRY(hipMemcpy(dst, xyzi, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
  return LIODOM_OK;
}

int liodom_process_resident(liodom_handle_t* h, int slot, int64_t n, int height, int width,
                            double* poses_out, liodom_step_info_t* infos_out) {
  return liodom_process_resident_pipelined(h, slot, -1, n, height, width, poses_out, infos_out);
}

// ---- subset steps: a lock-step step over a list of streams (liodom_process_resident_subset) ----
// A strictly ascending list of stream numbers in [0, n_streams).
static bool stream_list_valid(const liodom_handle* h, const int32_t* streams, int n) {
  if (n < 0 || n > h->S || (n > 0 && !streams)) return false;
  for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= h->S || (i > 0 && streams[i] <= streams[i - 1])) return false;
  return true;
}
// Stream list `list_id` (stream_of in liodom_kernels.h) on HIP stream q, in front of the launches that read it.  The entries
// travel in the kernel arguments of k_put_list: the caller's array is free when this returns, however far the host runs ahead.
// (Not booked by per-kernel profiling, like the copies of the other entry points: it is the step's argument, not a stage of it.)
static int put_stream_list(liodom_handle* h, hipStream_t q, int list_id, const int32_t* streams, int n) {
  for (int first = 0; first < n; first += kStreamListChunk) {
    StreamListChunk c;
    const int cnt = std::min(kStreamListChunk, n - first);
    std::memcpy(c.s, streams + first, sizeof(int32_t) * (size_t)cnt);
    hipLaunchKernelGGL(k_put_list, dim3(1), dim3(kStreamListChunk), 0, q, h->v, list_id, first, cnt, c);
  }
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}
// Extraction of the listed streams of resident slot `slot` into pipeline edge buffer eb (list eb, uploaded on the extraction stream:
// the previous extraction into eb, the list's last reader there, precedes it in stream order).  The full list is the plain extraction.
static int issue_extract_list(liodom_handle* h, int slot, int eb, int n, int height, int width, const int32_t* streams, int count) {
  if (count == h->S) return issue_extract(h, slot, eb, n, height, width);
  const int rc = put_stream_list(h, extract_queue(h), eb, streams, count);
  if (rc) return rc;
  return issue_extract(h, slot, eb, n, height, width, -eb - 1, count);
}

// Host-fed replay: the scan of every stream for resident slot `slot` is copied from host memory on the extraction stream
// (ordered behind the extraction that last read the slot).
static int upload_slot_async(liodom_handle_t* h, int slot, const float* host, int64_t stride, int64_t n) {
  // copies on their own stream (copy engine) so that they run beside the extraction kernels of the previous scan; the
  // slot is free once the extraction that last read it has completed, and its extraction waits for the upload
  const int r = slot % 3;
  if (!h->stream_c) {
    // HIP multiplexes its streams onto a few hardware queues: a handle that owns stream_k (overlapped second kNN pass) has
    // no queue left for a copy stream of its own — with one, the uploads of the host-fed replay ended up behind other
    // streams' launches (11.3k -> 7.5k scans/s).  That replay does not overlap the pass (ov_suppress), so stream_k is
    // idle in it and carries the uploads.
    if (h->stream_k) { h->stream_c = h->stream_k; h->stream_c_shared = true; }
    else HIP_TRY(hipStreamCreateWithFlags(&h->stream_c, hipStreamNonBlocking));
  }
  if (!h->ev_up[0]) {
    for (int b = 0; b < 3; b++) {
      HIP_TRY(hipEventCreateWithFlags(&h->ev_up[b], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_xdone[b], hipEventDisableTiming));
    }
  }
  hipStream_t q = extract_queue(h);
  if (h->pipe.xdone_valid[r]) HIP_TRY(hipStreamWaitEvent(h->stream_c, h->ev_xdone[r], 0));
  for (int s = 0; s < h->S && n > 0; s++) {
    float4* dst = h->resident + ((size_t)slot * h->S + s) * (size_t)h->v.max_points;
    HIP_TRY(hipMemcpyAsync(dst, host + (size_t)s * (size_t)stride, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream_c));
  }
  HIP_TRY(hipEventRecord(h->ev_up[r], h->stream_c));
  HIP_TRY(hipStreamWaitEvent(q, h->ev_up[r], 0));
  return LIODOM_OK;
}
static int upload_slot_consumed(liodom_handle_t* h, int slot) {      // call right after the slot's extraction has been issued
  const int r = slot % 3;
  HIP_TRY(hipEventRecord(h->ev_xdone[r], extract_queue(h)));
  h->pipe.xdone_valid[r] = true;
  return LIODOM_OK;
}

// One step of the pipelined replay over resident slots (both sides locked by the caller): the odometry of the `n_active` streams
// of `streams` on slot `slot`, and, next_slot >= 0, the extraction of the `n_next` streams of `next_streams` issued ahead on the
// extraction stream (next_host: uploaded first, the host-fed replay).  A list of all h->S streams is the plain lock-step step,
// launch for launch — the range instances, no list upload — and its pointer is not read.  wait: read the poses back before returning.
static int step_resident(liodom_handle_t* h, int slot, const int32_t* streams, int n_active, int next_slot, const int32_t* next_streams, int n_next,
                         int64_t n, int height, int width, bool wait, double* poses_out, liodom_step_info_t* infos_out,
                         const float* next_host = nullptr, int64_t host_stride = 0) {
  if (!h->resident || slot < 0 || slot >= h->n_slots || next_slot >= h->n_slots || n < 0 || n > h->v.max_points) {
    g_last_error = "bad resident slot"; return LIODOM_ERR_INVALID_ARG;
  }
  // resident layout: [slot][stream][max_points]: one lock-step launch reads a contiguous block
  EdgePipe& pipe = h->pipe;
  const int eb = pipe.replay_buffer();
  const bool full = n_active == h->S, next_full = n_next == h->S;
  int rc;
  if (n_active > 0) {
    // issued ahead for exactly these streams?  Anything else — another slot, another list, nothing — is extracted now
    if (!pipe.ahead_matches(slot, streams, n_active, h->S)) { rc = issue_extract_list(h, slot, eb, (int)n, height, width, streams, n_active); if (rc) return rc; }
    pipe.ahead_clear();
    if (full) {
      rc = enqueue_pipeline_odometry(h, eb, pipe.eb_seq[eb]);
    } else {
      // (list kEdgePipeBufs + eb, uploaded on the odometry stream behind the previous odometry of buffer eb)
      rc = put_stream_list(h, h->stream, kEdgePipeBufs + eb, streams, n_active);
      if (rc) return rc;
      rc = enqueue_pipeline_odometry(h, eb, pipe.eb_seq[eb], -(kEdgePipeBufs + eb) - 1, n_active, streams);
    }
    if (rc) return rc;
    pipe.replay_advance();
  }
  if (!(full && (next_slot < 0 || next_full))) h->subset_steps++;      // (liodom_get_modes: steps that were not the plain step)
  if (next_slot >= 0) {                           // overlap the next scan's (upload and) extraction with this odometry
    if (next_host) { rc = upload_slot_async(h, next_slot, next_host, host_stride, n); if (rc) return rc; }
    // (a gate in front of the next scan's extraction — start it when this scan's first solve starts, so that it runs beside the
    //  solves instead of beside the first kNN pass — was measured: -1.6 %; removed)
    // (an extraction issued ahead earlier and not consumed — n_active == 0 — is replaced: same buffer, same HIP stream)
    if (n_next > 0) { rc = issue_extract_list(h, next_slot, pipe.parity, (int)n, height, width, next_streams, n_next); if (rc) return rc; }
    if (next_host) { rc = upload_slot_consumed(h, next_slot); if (rc) return rc; }
    pipe.ahead_set(next_slot, next_streams, n_next, h->S);
  }
  if (wait && n_active > 0) return wait_pose(h, full ? 0 : -1, n_active, poses_out, infos_out, 0, full ? nullptr : streams);
  return LIODOM_OK;
}

// The consumer loop of liodom_replay_resident and liodom_replay_host over `count` scans, scan i stepped by step(i, wait, poses, infos):
// depth 0 waits inside the step; depth 1 enqueues scan i, then collects the pose of scan i - 1 (its sequence number is one behind
// the enqueue count).  timed: the resident replay's counters (where the host's time goes in this loop: liodom_get_modes reports the
// two averages — the host has one scan's duration to enqueue the next scan's launches; if the first number approaches the scan period
// the GPU starves) and the stamp of every collected pose.
extern "C++" {      // (a template, inside the C entry points)
template <class Step>
static int replay_loop(liodom_handle_t* h, int count, int depth, double* poses_out, liodom_step_info_t* infos_out, bool timed, Step step) {
  using clock = std::chrono::steady_clock;
  auto out_p = [&](int i) { return poses_out ? poses_out + (size_t)i * h->S * 7 : nullptr; };
  auto out_i = [&](int i) { return infos_out ? infos_out + (size_t)i * h->S : nullptr; };
  const clock::time_point t_call = timed ? clock::now() : clock::time_point();
  auto stamp = [&]() { if (timed) h->replay_stamps.push_back(std::chrono::duration<double, std::micro>(clock::now() - t_call).count()); };
  for (int i = 0; i < count; i++) {
    if (depth == 0) {
      const int rc = step(i, true, out_p(i), out_i(i));
      if (rc) return rc;
      continue;
    }
    const clock::time_point t_a = timed ? clock::now() : clock::time_point();
    int rc = step(i, false, nullptr, nullptr);
    if (rc) return rc;
    const clock::time_point t_b = timed ? clock::now() : clock::time_point();
    if (i > 0) { rc = wait_pose(h, 0, h->S, out_p(i - 1), out_i(i - 1), 1); if (rc) return rc; stamp(); }
    if (timed) {
      h->replay_enq_ns += std::chrono::duration<double, std::nano>(t_b - t_a).count();
      h->replay_wait_ns += std::chrono::duration<double, std::nano>(clock::now() - t_b).count();
      h->replay_timed++;
    }
  }
  if (depth == 1 && count > 0) { const int rc = wait_pose(h, 0, h->S, out_p(count - 1), out_i(count - 1), 0); if (rc) return rc; stamp(); }
  return LIODOM_OK;
}
}

int liodom_process_resident_pipelined(liodom_handle_t* h, int slot, int next_slot, int64_t n, int height,
                                      int width, double* poses_out, liodom_step_info_t* infos_out) {
  int rc0 = enter(h);
  if (rc0) return rc0;
  if ((rc0 = check_usable(h))) return rc0;
  SideLocks lk(h, true, true);
  if ((rc0 = tickets_idle(h))) return rc0;        // (the replay fills the same pipeline edge buffers)
  return step_resident(h, slot, nullptr, h->S, next_slot, nullptr, h->S, n, height, width, poses_out != nullptr || infos_out != nullptr, poses_out, infos_out);
}

int liodom_process_resident_subset(liodom_handle_t* h, int slot, const int32_t* streams, int n_active,
                                   int next_slot, const int32_t* next_streams, int n_next,
                                   int64_t n, int height, int width, double* poses_out, liodom_step_info_t* infos_out) {
  int rc = enter(h);
  if (rc) return rc;
  if ((rc = check_usable(h))) return rc;
  if (!stream_list_valid(h, streams, n_active)) { g_last_error = "liodom_process_resident_subset: streams must be strictly ascending stream indices"; return LIODOM_ERR_INVALID_ARG; }
  if (next_slot >= 0 && !next_streams) { next_streams = streams; n_next = n_active; }      // (the same streams step again)
  if (next_slot >= 0 && !stream_list_valid(h, next_streams, n_next)) { g_last_error = "liodom_process_resident_subset: next_streams must be strictly ascending stream indices"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, true);
  if ((rc = tickets_idle(h))) return rc;        // (the pipeline edge buffers, as the replay)
  const bool wait = poses_out != nullptr || infos_out != nullptr;
  return step_resident(h, slot, streams, n_active, next_slot, next_streams, n_next, n, height, width, wait, poses_out, infos_out);
}

int liodom_replay_resident(liodom_handle_t* h, int first_slot, int count, int ahead, int depth, int64_t n, int height, int width,
                           double* poses_out, liodom_step_info_t* infos_out) {
  int rc0 = enter(h);
  if (rc0) return rc0;
  if ((rc0 = check_usable(h))) return rc0;
  if (count < 0 || first_slot < 0 || depth < 0 || depth > 1) { g_last_error = "bad resident range / depth"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, true);
  if ((rc0 = tickets_idle(h))) return rc0;
  h->replay_stamps.clear();
  h->replay_stamps.reserve((size_t)count);
  return replay_loop(h, count, depth, poses_out, infos_out, true, [&](int i, bool wait, double* poses, liodom_step_info_t* infos) {
    const int slot = first_slot + i;
    const int next = (i + 1 < count || ahead) ? slot + 1 : -1;
    return step_resident(h, slot, nullptr, h->S, next, nullptr, h->S, n, height, width, wait, poses, infos);
  });
}

int liodom_replay_host(liodom_handle_t* h, const float* xyzi_base, int64_t scan_stride_floats, int count, int depth,
                       int64_t n, int height, int width, double* poses_out, liodom_step_info_t* infos_out) {
  int rc0 = enter(h);
  if (rc0) return rc0;
  if ((rc0 = check_usable(h))) return rc0;
  if (count < 0 || depth < 0 || depth > 1 || n < 0 || n > h->v.max_points || (count > 0 && n > 0 && !xyzi_base) || scan_stride_floats < 4 * n) {
    g_last_error = "liodom_replay_host: bad arguments"; return LIODOM_ERR_INVALID_ARG;
  }
  constexpr int kRing = 3;
  if (h->n_slots < kRing) { const int rc = liodom_alloc_resident(h, kRing); if (rc) return rc; }
  SideLocks lk(h, true, true);
  int rc = tickets_idle(h);
  if (rc) return rc;
  rc = drain_pipeline(h);
  if (rc) return rc;
  // Measured (MI355X, HDL-64 shape): with uploads the loop is bound by the host's enqueue work (an upload, three event
  // operations, six extraction and five odometry launches per scan: 88 us); the overlapped second kNN pass adds a gate and an
  // ALLOC launch on a third stream and made it 133 us.  So not here.
  struct Suppress { liodom_handle* h; ~Suppress() { h->ov_suppress = false; } } suppress{h};
  h->ov_suppress = true;
  auto src = [&](int i) { return xyzi_base + (size_t)i * (size_t)h->S * (size_t)scan_stride_floats; };
  rc = replay_loop(h, count, depth, poses_out, infos_out, false, [&](int i, bool wait, double* poses, liodom_step_info_t* infos) {
    const int slot = i % kRing, next = (i + 1 < count) ? (i + 1) % kRing : -1;
    if (i == 0) {                                 // first scan: upload + extraction now
      int rc1 = upload_slot_async(h, slot, src(0), scan_stride_floats, n);
      if (rc1) return rc1;
      rc1 = issue_extract(h, slot, h->pipe.parity, (int)n, height, width);
      if (rc1) return rc1;
      h->pipe.ahead_set(slot, nullptr, h->S, h->S);
      rc1 = upload_slot_consumed(h, slot);
      if (rc1) return rc1;
    }
    return step_resident(h, slot, nullptr, h->S, next, nullptr, h->S, n, height, width, wait, poses, infos, next >= 0 ? src(i + 1) : nullptr, scan_stride_floats);
  });
  if (rc) return rc;
  if (h->stream_c) HIP_TRY(hipStreamSynchronize(h->stream_c));
  for (int b = 0; b < 3; b++) h->pipe.xdone_valid[b] = false;
  return drain_pipeline(h);                       // the caller's buffer may be reused / unpinned after the return
}

int liodom_pin_host_buffer(void* p, int64_t bytes) {
  if (!p || bytes <= 0) return LIODOM_ERR_INVALID_ARG;
  HIP_TRY(hipHostRegister(p, (size_t)bytes, hipHostRegisterDefault));
  return LIODOM_OK;
}
int liodom_unpin_host_buffer(void* p) {
  if (!p) return LIODOM_ERR_INVALID_ARG;
  HIP_TRY(hipHostUnregister(p));
  return LIODOM_OK;
}

int liodom_sync(liodom_handle_t* h) {
  int rc0 = enter(h);
  if (rc0) return rc0;
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  if (h->stream_k) HIP_TRY(hipStreamSynchronize(h->stream_k));
  // everything has completed: unless an extraction has been issued ahead for the replay's next scan, the pipeline edge buffers
  // are free again (for the ticket API, or for a replay that starts over at buffer 0)
  if (h->pipe.pf_slot < 0) return drain_pipeline(h);
  return LIODOM_OK;
}

int liodom_get_pose_log(liodom_handle_t* h, int stream, int first, int count, double* poses_out,
                        liodom_step_info_t* infos_out) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (first < 0 || count < 0 || first + count > h->v.pose_log_cap) { g_last_error = "pose log range"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  if (poses_out && count)
    HIP_TRY(hipMemcpy(poses_out, h->v.pose_log + ((size_t)stream * h->v.pose_log_cap + first) * 7, sizeof(double) * 7 * (size_t)count, hipMemcpyDeviceToHost));
  if (infos_out && count)
    HIP_TRY(hipMemcpy(infos_out, h->v.info_log + (size_t)stream * h->v.pose_log_cap + first, sizeof(liodom_step_info_t) * (size_t)count, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

int liodom_get_pose_covariance_log(liodom_handle_t* h, int stream, int first, int count, liodom_pose_cov_t* out) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.cov_log) { g_last_error = "liodom_get_pose_covariance_log: the handle was created with pose_covariance = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (first < 0 || count < 0 || first + count > h->v.pose_log_cap) { g_last_error = "pose log range"; return LIODOM_ERR_INVALID_ARG; }
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  if (out && count)
    HIP_TRY(hipMemcpy(out, h->v.cov_log + (size_t)stream * h->v.pose_log_cap + first, sizeof(liodom_pose_cov_t) * (size_t)count, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

// ---- odometry edges from the scans' covariances (odom_edges.h decides, kernels_odom_edges.h computes) ----
// One launch of k_odom_edges on q over device-resident poses and records; ws: odom_ws_bytes(n) of device memory (the records
// first: they are stored as 8-byte words).  Returns after the records have arrived in `out`.
static size_t odom_ws_bytes(int n) { return (size_t)n * (sizeof(liodom_odom_edge_t) + 2 * sizeof(int32_t)); }
static int odom_edges_launch(const double* d_poses, const liodom_pose_cov_t* d_recs, const int32_t* from, const int32_t* to, int n,
                             const liodom_odom_edge_options_t& o, unsigned char* ws, hipStream_t q, liodom_odom_edge_t* out) {
  liodom_odom_edge_t* d_out = reinterpret_cast<liodom_odom_edge_t*>(ws);
  int32_t* d_from = reinterpret_cast<int32_t*>(ws + (size_t)n * sizeof(liodom_odom_edge_t));
  int32_t* d_to = d_from + n;
  HIP_TRY(hipMemcpyAsync(d_from, from, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, q));
  HIP_TRY(hipMemcpyAsync(d_to, to, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, q));
  hipLaunchKernelGGL(k_odom_edges, dim3((unsigned int)n), dim3(64), 0, q, d_poses, d_recs, d_from, d_to, n, o.inflation,
                     o.floor_rotation * o.floor_rotation, o.floor_translation * o.floor_translation, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out, sizeof(liodom_odom_edge_t) * (size_t)n, hipMemcpyDeviceToHost, q));
  HIP_TRY(hipStreamSynchronize(q));
  return LIODOM_OK;
}
// the options of a call (null: the defaults) into *o, or why not
static int odom_edge_options_in(const liodom_odom_edge_options_t* opt, liodom_odom_edge_options_t* o, const char* who) {
  if (opt) *o = *opt; else odom_edge_options_default(o);
  if (const char* why = odom_edge_options_refusal(o)) { g_last_error = std::string(who) + ": " + why; return LIODOM_ERR_INVALID_ARG; }
  return LIODOM_OK;
}

void liodom_odom_edge_options_default(liodom_odom_edge_options_t* opt) {
  if (opt) odom_edge_options_default(opt);
}

int liodom_chain_odometry_edges(const double* poses, const liodom_pose_cov_t* records, int m, const int32_t* from, const int32_t* to,
                                int n, const liodom_odom_edge_options_t* opt, liodom_odom_edge_t* out) {
  static const char* who = "liodom_chain_odometry_edges";
  liodom_odom_edge_options_t o;
  if (const int rc = odom_edge_options_in(opt, &o, who)) return rc;
  if (m < 0 || (m > 0 && (!poses || !records))) { g_last_error = std::string(who) + ": m < 0, or null poses or records"; return LIODOM_ERR_INVALID_ARG; }
  if (const char* why = odom_edge_ranges_refusal(from, to, n, 0, m, nullptr)) { g_last_error = std::string(who) + ": " + why; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  if (!out) { g_last_error = std::string(who) + ": null out"; return LIODOM_ERR_INVALID_ARG; }
  // one block of device memory for the call: records (8-byte aligned sizes first), poses, then the launch's workspace
  const size_t rec_bytes = sizeof(liodom_pose_cov_t) * (size_t)m, pose_bytes = sizeof(double) * 7 * (size_t)m;
  struct Block { void* p = nullptr; ~Block() { if (p) hipFree(p); } } blk;
  HIP_TRY(hipMalloc(&blk.p, rec_bytes + pose_bytes + odom_ws_bytes(n)));
  unsigned char* base = static_cast<unsigned char*>(blk.p);
  HIP_TRY(hipMemcpyAsync(base, records, rec_bytes, hipMemcpyHostToDevice, nullptr));
  HIP_TRY(hipMemcpyAsync(base + rec_bytes, poses, pose_bytes, hipMemcpyHostToDevice, nullptr));
  return odom_edges_launch(reinterpret_cast<const double*>(base + rec_bytes), reinterpret_cast<const liodom_pose_cov_t*>(base), from, to, n, o,
                           base + rec_bytes + pose_bytes, nullptr, out);
}

int liodom_get_odometry_edges(liodom_handle_t* h, int stream, const int32_t* from, const int32_t* to, int n,
                              const liodom_odom_edge_options_t* opt, liodom_odom_edge_t* out) {
  static const char* who = "liodom_get_odometry_edges";
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->v.cov_log) { g_last_error = std::string(who) + ": the handle was created with pose_covariance = 0"; return LIODOM_ERR_UNSUPPORTED; }
  liodom_odom_edge_options_t o;
  if ((rc = odom_edge_options_in(opt, &o, who))) return rc;
  SideLocks lk(h, true, false);      // (no scan can be enqueued meanwhile: the limit below holds until the records are out)
  const int limit = odom_edge_log_limit(h->scans_enqueued[stream], h->v.pose_log_cap);
  if (const char* why = odom_edge_ranges_refusal(from, to, n, h->log_first[stream], limit, nullptr)) { g_last_error = std::string(who) + ": " + why; return LIODOM_ERR_INVALID_ARG; }
  if (n == 0) return LIODOM_OK;
  if (!out) { g_last_error = std::string(who) + ": null out"; return LIODOM_ERR_INVALID_ARG; }
  HIP_TRY(sync_odometry(h));
  if (h->odom_ws_bytes < odom_ws_bytes(n)) {      // the call's workspace: made by the first call, grown when one needs more
    if (h->odom_ws) { HIP_TRY(hipFree(h->odom_ws)); h->odom_ws = nullptr; h->odom_ws_bytes = 0; }
    HIP_TRY(hipMalloc(&h->odom_ws, odom_ws_bytes(n)));
    h->odom_ws_bytes = odom_ws_bytes(n);
  }
  return odom_edges_launch(h->v.pose_log + (size_t)stream * h->v.pose_log_cap * 7, h->v.cov_log + (size_t)stream * h->v.pose_log_cap, from, to, n,
                           o, static_cast<unsigned char*>(h->odom_ws), h->stream, out);
}

int liodom_wait_pose_covariance(liodom_handle_t* h, int stream, int scan_index, liodom_pose_cov_t* out) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!h->cov_host) { g_last_error = "liodom_wait_pose_covariance: the handle was created with pose_covariance = 0"; return LIODOM_ERR_UNSUPPORTED; }
  if (!out) return LIODOM_ERR_INVALID_ARG;
  SideLocks lk(h, true, false);      // (no scan can be enqueued meanwhile: record scan_index & 1 is not rewritten while this waits)
  const int enq = h->scans_enqueued[stream];
  if (scan_index < 0 || scan_index >= enq || scan_index < enq - 2) {
    g_last_error = "liodom_wait_pose_covariance: the scan is not among the two latest enqueued scans of the stream";
    return LIODOM_ERR_INVALID_ARG;
  }
  volatile HostCov* hc = h->cov_host + (size_t)stream * 2 + (scan_index & 1);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned long long spins = 0;
  while (__atomic_load_n(&hc->seq, __ATOMIC_ACQUIRE) != scan_index + 1) {
    if ((++spins & 0xFFFFull) == 0) {
      const hipError_t q = hipStreamQuery(h->stream);
      if (q != hipErrorNotReady && q != hipSuccess) { g_last_error = std::string("stream error while waiting: ") + hipGetErrorString(q); return LIODOM_ERR_HIP; }
      if (q == hipSuccess && __atomic_load_n(&hc->seq, __ATOMIC_ACQUIRE) != scan_index + 1) { g_last_error = "stream drained without publishing the scan's covariance record"; return LIODOM_ERR_HIP; }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) { g_last_error = "liodom_wait_pose_covariance: timed out"; return LIODOM_ERR_HIP; }
    }
  }
  std::memcpy(out, const_cast<const liodom_pose_cov_t*>(&h->cov_host[(size_t)stream * 2 + (scan_index & 1)].rec), sizeof(liodom_pose_cov_t));
  return LIODOM_OK;
}

static int get_window_impl(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points, int* n_frames) {
  HIP_TRY(sync_odometry(h));
  StreamState st;
  HIP_TRY(hipMemcpy(&st, h->v.state + stream, sizeof(st), hipMemcpyDeviceToHost));
  const int P = h->P;
  std::vector<int> base((size_t)P + 1), slot((size_t)P);
  HIP_TRY(hipMemcpy(base.data(), h->v.win_base + (size_t)stream * (P + 1), sizeof(int) * (P + 1), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slot.data(), h->v.win_slot + (size_t)stream * P, sizeof(int) * P, hipMemcpyDeviceToHost));
  if (n_points) *n_points = st.n_map;
  if (n_frames) *n_frames = st.n_frames;
  if (st.n_map > cap) { g_last_error = "window buffer too small"; return LIODOM_ERR_CAPACITY; }
  for (int j = 0; j < st.n_frames && xyzi; j++) {
    const int cnt = base[j + 1] - base[j];
    if (cnt > 0)
      HIP_TRY(hipMemcpy(xyzi + 4 * (size_t)base[j], h->v.win_pts + ((size_t)stream * P + slot[j]) * h->v.edge_cap,
                        sizeof(float4) * (size_t)cnt, hipMemcpyDeviceToHost));
  }
  return LIODOM_OK;
}

int liodom_get_window(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points, int* n_frames) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  SideLocks lk(h, true, false);
  return get_window_impl(h, stream, xyzi, cap, n_points, n_frames);
}

int liodom_get_local_map(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points, int* filtered) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  StreamState st;
  HIP_TRY(hipMemcpy(&st, h->v.state + stream, sizeof(st), hipMemcpyDeviceToHost));
  if (filtered) *filtered = st.n_filt > 0 ? 1 : 0;
  if (st.n_filt == 0) {
    int nf = 0;
    int64_t nw = 0;
    rc = get_window_impl(h, stream, xyzi, cap, &nw, &nf);
    const int nr = h->v.mapping ? st.n_recv : 0;
    if (n_points) *n_points = nw + nr;
    if (rc) return rc;
    if (nw + nr > cap) { g_last_error = "local-map buffer too small"; return LIODOM_ERR_CAPACITY; }
    if (nr && xyzi) HIP_TRY(hipMemcpy(xyzi + 4 * (size_t)nw, h->v.recv_pts + (size_t)stream * h->v.recv_cap, sizeof(float4) * (size_t)nr, hipMemcpyDeviceToHost));
    return LIODOM_OK;
  }
  const int n = st.n_filt;
  if (n_points) *n_points = n;
  if (n > cap) { g_last_error = "local-map buffer too small"; return LIODOM_ERR_CAPACITY; }
  std::vector<float4> pts((size_t)n);
  std::vector<float> inten((size_t)n);
  HIP_TRY(hipMemcpy(pts.data(), h->v.filt_pts + (size_t)stream * h->v.map_cap, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(inten.data(), h->v.filt_int + (size_t)stream * h->v.map_cap, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; i++) order[i] = i;
  auto leaf = [&](int i) { unsigned int u; std::memcpy(&u, &pts[i].w, 4); return u; };
  std::sort(order.begin(), order.end(), [&](int a, int b) { return leaf(a) < leaf(b); });   // PCL output order
  for (int i = 0; i < n && xyzi; i++) {
    const float4& p = pts[order[i]];
    xyzi[4 * i] = p.x; xyzi[4 * i + 1] = p.y; xyzi[4 * i + 2] = p.z; xyzi[4 * i + 3] = inten[order[i]];
  }
  return LIODOM_OK;
}

int liodom_get_correspondences(liodom_handle_t* h, int stream, int it, int32_t* valid, int32_t* idx_a,
                               int32_t* idx_b, int cap, int* n) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (it < 0 || it > 1) return LIODOM_ERR_INVALID_ARG;
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  StreamState st;
  HIP_TRY(hipMemcpy(&st, h->v.state + stream, sizeof(st), hipMemcpyDeviceToHost));
  const int E = st.n_edges_buf[h->last_eb[stream]];
  if (n) *n = E;
  if (E > cap) { g_last_error = "correspondence buffer too small"; return LIODOM_ERR_CAPACITY; }
  std::vector<int2> ci((size_t)std::max(E, 1));
  if (E) HIP_TRY(hipMemcpy(ci.data(), h->v.corr_idx + ((size_t)stream * 2 + it) * h->v.edge_cap, sizeof(int2) * (size_t)E, hipMemcpyDeviceToHost));
  for (int i = 0; i < E; i++) {
    if (valid) valid[i] = ci[i].x >= 0 ? 1 : 0;
    if (idx_a) idx_a[i] = ci[i].x;
    if (idx_b) idx_b[i] = ci[i].y;
  }
  return LIODOM_OK;
}

int liodom_get_knn_queries(liodom_handle_t* h, int stream, int it, float* xyz0, int cap, int* n) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (it < 0 || it > 1) return LIODOM_ERR_INVALID_ARG;
  if (!h->v.knn_q) { g_last_error = "create the handle with debug_buffers = 1"; return LIODOM_ERR_UNSUPPORTED; }
  SideLocks lk(h, true, false);
  HIP_TRY(sync_odometry(h));
  int E = 0;
  HIP_TRY(hipMemcpy(&E, &h->v.state[stream].n_edges_buf[h->last_eb[stream]], sizeof(int), hipMemcpyDeviceToHost));
  if (n) *n = E;
  if (E > cap) { g_last_error = "query buffer too small"; return LIODOM_ERR_CAPACITY; }
  if (E && xyz0) HIP_TRY(hipMemcpy(xyz0, h->v.knn_q + ((size_t)stream * 2 + it) * h->v.edge_cap, sizeof(float4) * (size_t)E, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

int liodom_get_curvature(liodom_handle_t* h, int stream, double* curv, int64_t cap, int32_t* ring_offsets) {
  int rc = check_stream(h, stream);
  if (rc) return rc;
  if (!(h->v.debug & 1)) { g_last_error = "create the handle with debug_buffers = 1"; return LIODOM_ERR_UNSUPPORTED; }
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  std::vector<int> rs((size_t)h->H + 1), rl((size_t)h->H);
  HIP_TRY(hipMemcpy(rs.data(), h->v.ring_start + (size_t)stream * (h->H + 1), sizeof(int) * (h->H + 1), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rl.data(), h->v.ring_len + (size_t)stream * h->H, sizeof(int) * h->H, hipMemcpyDeviceToHost));
  // output: the compacted rings back to back (on the device the rings of an organised cloud sit at ring * width)
  int64_t off = 0;
  for (int r = 0; r < h->H; r++) { if (ring_offsets) ring_offsets[r] = (int32_t)off; off += rl[r]; }
  if (ring_offsets) ring_offsets[h->H] = (int32_t)off;
  if (off > cap) { g_last_error = "curvature buffer too small"; return LIODOM_ERR_CAPACITY; }
  int64_t o = 0;
  for (int r = 0; r < h->H && curv; r++) {
    if (rl[r]) HIP_TRY(hipMemcpy(curv + o, h->v.ring_c + (size_t)stream * h->v.ring_stride + rs[r], sizeof(double) * (size_t)rl[r], hipMemcpyDeviceToHost));
    o += rl[r];
  }
  return LIODOM_OK;
}

int liodom_set_profiling(liodom_handle_t* h, int enable) {
  int rc = enter(h);
  if (rc) return rc;
  std::unique_lock<std::mutex> lo(h->mx_o), lx(h->mx_x);
  rc = drain_events(h);
  h->profiling = enable != 0;
  return rc;
}

int liodom_get_kernel_stats(liodom_handle_t* h, liodom_kernel_stat_t* stats) {
  if (!h || !stats) return LIODOM_ERR_INVALID_ARG;
  int rc = enter(h);
  if (rc) return rc;
  SideLocks lk(h, true, true);
  rc = drain_events(h);
  if (rc) return rc;
  for (int i = 0; i < LIODOM_NUM_KERNELS; i++) {
    std::memset(&stats[i], 0, sizeof(stats[i]));
    std::strncpy(stats[i].name, kKernelNames[i], sizeof(stats[i].name) - 1);
    stats[i].launches = h->k_count[i];
    stats[i].total_ms = h->k_ms[i];
  }
  return LIODOM_OK;
}

int liodom_reset_kernel_stats(liodom_handle_t* h) {
  int rc = enter(h);
  if (rc) return rc;
  SideLocks lk(h, true, true);
  rc = drain_events(h);
  for (int i = 0; i < LIODOM_NUM_KERNELS; i++) { h->k_ms[i] = 0; h->k_count[i] = 0; }
  return rc;
}

/* debug (schedule perturbation, tools/inject_delay.py): seed of the pseudo-random delays in front of every publication and behind
 * every successful in-kernel wait; 0 switches them off.  Only in a library built with -DLIODOM_INJECT_DELAY. */
int liodom_debug_set_inject_seed(liodom_handle_t* h, unsigned int seed) {
#if defined(LIODOM_INJECT_DELAY)
  if (!h) return LIODOM_ERR_INVALID_ARG;
  if (int rc = enter(h)) return rc;
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_inject_seed), &seed, sizeof(seed)));
  return LIODOM_OK;
#else
  (void)h; (void)seed;
  g_last_error = "liodom_debug_set_inject_seed: the product library carries no delay injection; build a variant with -DLIODOM_INJECT_DELAY (tools/variant_build.sh)";
  return LIODOM_ERR_UNSUPPORTED;
#endif
}

/* debug: raw phase timestamps (100 MHz) written by the kernels when LIODOM_DEBUG_CLOCKS is set */
// (debug) when the host collected every pose of the last liodom_replay_resident call (depth 1): microseconds since the call began
int liodom_debug_replay_stamps(liodom_handle_t* h, double* out_us, int cap) {
  if (!h || !out_us || cap < 0) return LIODOM_ERR_INVALID_ARG;
  const int n = (int)std::min<size_t>(h->replay_stamps.size(), (size_t)cap);
  for (int i = 0; i < n; i++) out_us[i] = h->replay_stamps[(size_t)i];
  return n;
}
int liodom_debug_clocks(liodom_handle_t* h, unsigned long long* out512) {
  if (!h || !out512) return LIODOM_ERR_INVALID_ARG;
  if (!kInstrument) { g_last_error = "liodom_debug_clocks: the product library carries no instrumentation; build a variant with -DLIODOM_INSTRUMENT (tools/variant_build.sh)"; return LIODOM_ERR_UNSUPPORTED; }
  if (int rc = enter(h)) return rc;
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  HIP_TRY(hipMemcpy(out512, h->v.dbg_clk, sizeof(unsigned long long) * 512, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

/* debug: per-query phase times of k_knn (stream 0, latest scan): out[2][edge_cap][8]; returns edge_cap through *cap */
int liodom_debug_knn_times(liodom_handle_t* h, unsigned int* out, int* cap) {
  if (!h || !cap) return LIODOM_ERR_INVALID_ARG;
  *cap = h->v.edge_cap;
  if (!out) return LIODOM_OK;
  if (!h->v.dbg_q) return LIODOM_ERR_UNSUPPORTED;
  if (int rc = enter(h)) return rc;
  SideLocks lk(h, true, true);
  HIP_TRY(hipStreamSynchronize(h->stream_x));
  HIP_TRY(sync_odometry(h));
  HIP_TRY(hipMemcpy(out, h->v.dbg_q, sizeof(unsigned int) * 2 * (size_t)h->v.edge_cap * 12, hipMemcpyDeviceToHost));
  return LIODOM_OK;
}

int liodom_get_modes(liodom_handle_t* h, char* buf, int cap) {
  if (!h || !buf || cap < 2) return LIODOM_ERR_INVALID_ARG;
  if (int rc = enter(h)) return rc;
  SideLocks lk(h, true, true);
  const DevView& v = h->v;
  ModesRuntime r;
  r.alone = g_live_handles.load() <= 1;
  r.streams_concurrent = h->streams_concurrent;
  // (speculative hand-overs of stream 0 since the last reset: the launches enqueued so far have to have run for the figures to mean
  //  anything — a caller that wants them synchronises first; this call does not)
  unsigned int done_cnt[64] = {0};      // (chain mode: the passes' done counters of stream 0 — first pass [0], second pass [32] — against the host's target)
  if (v.knn_done0) (void)hipMemcpy(done_cnt, v.knn_done0, sizeof(done_cnt), hipMemcpyDeviceToHost);
  (void)hipMemcpy(r.spec_stats, reinterpret_cast<const char*>(v.state) + offsetof(StreamState, spec_stats), sizeof(r.spec_stats), hipMemcpyDeviceToHost);
  (void)hipMemcpy(r.hb_stats, reinterpret_cast<const char*>(v.state) + offsetof(StreamState, hb_stats), sizeof(r.hb_stats), hipMemcpyDeviceToHost);
  r.chain_count = h->step.chain_count; r.done0 = done_cnt[0]; r.done1 = done_cnt[32];
  if (h->replay_timed) { r.replay_enqueue_us = h->replay_enq_ns / (1e3 * (double)h->replay_timed); r.replay_wait_us = h->replay_wait_ns / (1e3 * (double)h->replay_timed); }
  r.n_lagged = h->maps.n_lagged; r.n_readers = h->maps.n_readers; r.subset_steps = h->subset_steps; r.n_hits = h->maps.n_hits;
  plan_format_modes(h->plan, r, buf, cap);
  return LIODOM_OK;
}

int liodom_device_count(int* count) {
  if (!count) return LIODOM_ERR_INVALID_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return LIODOM_OK;
}

int liodom_device_pci_bus_id(int device, char* bus_id, int cap) {
  if (!bus_id || cap < 16) return LIODOM_ERR_INVALID_ARG;
  HIP_TRY(hipDeviceGetPCIBusId(bus_id, cap, device));
  return LIODOM_OK;
}

int liodom_device_info(liodom_handle_t* h, char* name, int name_cap, int* compute_units) {
  if (!h) return LIODOM_ERR_INVALID_ARG;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, h->config.device));
  if (name && name_cap > 0) {
    const char* nm = prop.name[0] ? prop.name : prop.gcnArchName;   // some driver stacks leave name empty
    std::strncpy(name, nm, (size_t)name_cap - 1); name[name_cap - 1] = 0;
  }
  if (compute_units) *compute_units = prop.multiProcessorCount;
  return LIODOM_OK;
}

}  // extern "C"

#include "liodom_places_host.h"
#include "liodom_graph_host.h"
