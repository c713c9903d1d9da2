/* liodom_hip.h — C-ABI of the MI355X-native LiODOM hot path (libliodom_hip.so).
 *
 * The reference (/root/reference, emiliofidalgo/liodom) has no plugin / FFI surface: its hot
 * path lives in private member functions of two worker classes fed by ROS callbacks.  This
 * header is the boundary a maintainer binds instead of those members; each entry point names
 * the reference interface it replaces (paths relative to /root/reference).  INTEGRATION.md
 * shows the reference-side glue.
 *
 * Conventions: plain C, caller-owned buffers with explicit capacities, int status return
 * (0 = LIODOM_OK, negative = error), no exceptions cross the boundary.  Points are packed
 * float[4] XYZI (pcl::PointXYZI without padding).  Poses are world<-laser, 7 doubles
 * [qx qy qz qw tx ty tz] — the storage order of param_q / param_t
 * (include/liodom/laser_odometry.h:98-99, src/laser_odometry.cc:187-195).
 *
 * One handle drives one GPU and `n_streams` independent LiDAR streams that advance in
 * lock-step (every kernel is launched once over all streams).  n_streams = 1 is the drop-in
 * case for liodom_node; n_streams > 1 serves replay / multi-sensor batches.
 *
 * Threading.  The reference runs a FeatureExtractor thread and a LaserOdometer thread side by side
 * (src/liodom_node.cc:89-91) and hands edge clouds over through a queue (src/shared_data.cc:64-89).
 * The handle mirrors that with two sides: liodom_extract_edges works on the extraction side (its own
 * HIP stream, scratch and edge buffer), liodom_odometry_step on the odometry side (window, local-map
 * hash, pose state, result records).  One thread may call liodom_extract_edges while another calls
 * liodom_odometry_step on the same handle: extraction of scan k+1 then overlaps the odometry of scan
 * k on the GPU, and the poses are bit-identical to the serial order (tests/test_gpu_threads.py).
 * Each side serialises its own callers with a mutex; every other entry point takes both mutexes,
 * i.e. is safe to call from any thread but does not overlap with anything.  While per-kernel
 * profiling is enabled (liodom_set_profiling) all entry points are serialised.
 */
#ifndef LIODOM_HIP_H
#define LIODOM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIODOM_OK 0
#define LIODOM_ERR_INVALID_ARG (-1)
#define LIODOM_ERR_UNSUPPORTED (-2)   /* call not valid for the way the handle was created (e.g. mapping = 0) */
#define LIODOM_ERR_CAPACITY (-3)      /* caller buffer or configured capacity too small */
#define LIODOM_ERR_HIP (-4)           /* HIP runtime failure; see liodom_last_error() */
#define LIODOM_ERR_NO_DEVICE (-5)
#define LIODOM_ERR_BUSY (-6)          /* device-resident hand-off: every slot holds an edge cloud that has not been consumed yet (retry
                                         after liodom_odometry_step_device), or tickets are outstanding where none may be */
#define LIODOM_ERR_NEEDS_SYNC (-7)    /* liodom_extract_edges_device while scans of a resident / host replay (liodom_process_resident*,
                                         liodom_replay_*) still occupy the pipeline edge buffers: retrying cannot help — call liodom_sync()
                                         (or liodom_reset()) first, then hand clouds over by ticket */

/* Sticky per-stream status bits reported in liodom_step_info_t.status */
#define LIODOM_STATUS_RING_OVERFLOW 1u  /* deprecated, never raised (rings of any length are processed); kept so that callers
                                           that test the bit keep compiling */
#define LIODOM_STATUS_EDGE_OVERFLOW 2u
#define LIODOM_STATUS_HASH_FULL 4u
#define LIODOM_STATUS_LM_SYNC_TIMEOUT 8u  /* cooperating LM workgroups did not all arrive (result invalid) */
#define LIODOM_STATUS_PIPE_TIMEOUT 16u    /* pipelined replay: a kernel waited ~0.3 s in vain for the other HIP stream of the handle
                                             (kernels serialised across streams by a profiler / debugger, or a GPU saturated by
                                             another process).  The waiting workgroups skipped their work: the scan's result is
                                             invalid, the entry point that collects it returns LIODOM_ERR_HIP, and the handle
                                             switches to event-based stream dependencies; liodom_reset() before reusing the stream */

/* Field-for-field mirror of liodom::Params (include/liodom/params.h:33-49); defaults are
 * those of Params::readParams (src/params.cc:40-109). */
typedef struct liodom_params_t {
  double min_range;              /* params.h:33  default 3.0  */
  double max_range;              /* params.h:34  default 75.0 */
  int32_t lidar_type;            /* params.h:35  0 Velodyne (elevation binning), 1 Ouster (row = ring) */
  int32_t scan_lines;            /* params.h:36  default 64 */
  int32_t scan_regions;          /* params.h:37  default 8  */
  int32_t edges_per_region;      /* params.h:38  default 10 */
  uint64_t min_points_per_scan;  /* params.h:39  scan_regions*edges_per_region + 10 (params.cc:63) */
  uint64_t local_map_size;       /* params.h:40  "prev_frames", default 5 */
  int32_t save_results;          /* params.h:41 */
  char results_dir[256];         /* params.h:42  default "~/" */
  char fixed_frame[64];          /* params.h:43  default "odom" */
  char base_frame[64];           /* params.h:44  default "base_link" */
  char laser_frame[64];          /* params.h:45  default "" (taken from the header) */
  int32_t use_imu;               /* params.h:46 */
  int32_t filter_local_map;      /* params.h:47 */
  int32_t mapping;               /* params.h:48 */
  int32_t publish_tf;            /* params.h:49  default true */
} liodom_params_t;

/* Engine configuration that has no counterpart in the reference. */
typedef struct liodom_config_t {
  int32_t device;            /* HIP device ordinal */
  int32_t n_streams;         /* independent streams advanced in lock-step (>= 1) */
  int32_t max_points;        /* capacity: points per scan (H*W) */
  int32_t max_width;         /* expected points per ring (0 = max_points / scan_lines): picks the extraction kernel instance whose
                                register tile covers the longest region, (max_width - 10) / scan_regions + remainder items;
                                not a capacity — longer rings are processed by the generic path of the same kernel */
  union {                    /* (anonymous union: C11 / C++) */
    int32_t reserved1;       /* ignored */
    int32_t max_ring_points; /* deprecated name of the same field (earlier headers: capacity of a ring): ignored, rings have no
                                capacity any more; kept so that callers that set it keep compiling */
  };
  int32_t lm_apply_step_on_ftol; /* 0 = Ceres >= 1.12 behaviour (LM section) */
  int32_t pose_log_capacity; /* scans kept in the device-side pose log (resident replay) */
  int32_t debug_buffers;     /* 1 = keep per-ring smoothness dumps for liodom_get_curvature */
  int32_t lm_workgroups;     /* workgroups (CUs) per stream for the pose solve: 0 = auto (<= 4 streams: 8 for >= 8192 possible edges, 4 for >= 4096; else 1), or 1 .. 8 */
  int32_t recv_capacity;     /* mapping = 1: points of the received ~map cloud the kNN structure can take (0 = 262144) */
  int32_t pose_rotation_mode; /* what Eigen::Transform::rotation() returns at src/laser_odometry.cc:164,186,403,420:
                                 1 (default) = Eigen 3.3.x, the README's platform: orthonormal polar factor of linear()
                                 (computeRotationScaling, JacobiSVD) for every Mode; 0 = Eigen >= 3.4: alias of linear()
                                 for an Isometry.  See DESIGN.md §4. */
  int32_t pose_covariance;   /* 1 = per-scan pose covariance records (liodom_pose_cov_t below); 0 (default) = none: the handle launches
                                exactly what it launches without the feature and allocates nothing for it */
} liodom_config_t;

typedef struct liodom_lm_trace_t {
  int32_t iterations;        /* trust-region iterations used (<= 4, src/laser_odometry.cc:214) */
  int32_t accepted;
  int32_t termination;       /* 0 max-iter 1 param-tol 2 func-tol 3 grad-tol 4 no-residuals 5 eval-failure 6 radius 7 invalid-steps */
  int32_t pad;
  double initial_cost;
  double final_cost;
} liodom_lm_trace_t;

/* Per-scan diagnostics (what the reference logs with ROS_DEBUG at
 * feature_extractor.cc:62, laser_odometry.cc:279,297,365). */
typedef struct liodom_step_info_t {
  int32_t n_edges;
  int32_t map_points;        /* local-map points searched by this scan */
  int32_t matches[2];        /* "Correct matchings" of the two outer iterations */
  liodom_lm_trace_t lm[2];
  uint32_t status;
  int32_t scan_index;
} liodom_step_info_t;

/* ---- per-scan pose covariance (config.pose_covariance = 1) ----
 * One record per scan per stream, written for every scan that gets a pose-log entry.  It describes the pose the finalising solve
 * returned, in the solver's own tangent space — the one ceres::Covariance::GetCovarianceMatrixInTangentSpace would use for this
 * problem: (d0 d1 d2 dtx dty dtz).  The rotation part is the EigenQuaternionParameterization increment
 * q <- [sin|d| d/|d|, cos|d|] (x) q (left multiplication, world frame): the ROTATION ANGLE IS 2|d| — a half-angle tangent (for
 * rotation variances in radians^2 multiply the rotation block by 4; pose_cov_to_ros in liodom_math.h converts the whole matrix
 * to nav_msgs/Odometry order for the pose published with laser_to_base).  The translation part is additive, world coordinates.
 *   information   H = sum rho' J^T J over the valid residual blocks at the returned pose: the loss-corrected Gauss-Newton matrix the
 *                 LM controller holds there (Huber a = 0.2).
 *   sigma2        2 final_cost / (3 C - 6), the a-posteriori variance factor.  The residuals are weighted point-to-line distances
 *                 (factors.hpp: distance x (1.01 - normalised range)), not whitened measurements: sigma2 scales H^-1 to the
 *                 observed residual level, it does not make the covariance a calibrated measurement covariance.
 *   covariance    sigma2 H^-1.
 *   eigenvalues / eigenvectors of H: the small eigenvalues and their vectors name the directions the scan leaves unconstrained
 *                 (a corridor, vertical edges only, the mapping-mode degeneracy of DESIGN.md).
 * Undefined values are NaN. */
typedef struct liodom_pose_cov_t {
  int32_t scan_index;        /* = liodom_step_info_t.scan_index of the same scan */
  uint32_t flags;            /* LIODOM_COV_* below */
  int32_t n_residuals;       /* C: valid residual blocks of the finalising solve */
  int32_t termination;       /* = info.lm[1].termination */
  double final_cost;         /* 0.5 * sum rho at the returned pose (bit-equal to info.lm[1].final_cost) */
  double sigma2;             /* 2 * final_cost / (3 C - 6); NaN if 3 C <= 6 */
  double information[36];    /* H = sum rho' J^T J at the returned pose, full symmetric, row-major */
  double covariance[36];     /* sigma2 * H^-1; NaN-filled unless flags has LIODOM_COV_VALID and not SINGULAR */
  double eigenvalues[6];     /* of H, ascending */
  double eigenvectors[36];   /* row-major; column j belongs to eigenvalues[j]; unit length; sign: largest-|.| component > 0 */
} liodom_pose_cov_t;
#define LIODOM_COV_VALID 1u          /* a solve ran and its evaluation at the returned pose was finite (and had residual blocks) */
#define LIODOM_COV_SINGULAR 2u       /* Cholesky of H failed: covariance is NaN; eigen-decomposition still valid */
#define LIODOM_COV_NO_SOLVE 4u       /* first scan of a stream (or first after liodom_reset): no H, everything NaN */
#define LIODOM_COV_EVAL_FAILURE 8u   /* termination 5 (non-finite blocks): H is meaningless, everything NaN */
#define LIODOM_COV_FEW_RESIDUALS 16u /* 3 C <= 6: sigma2 and covariance NaN */

typedef struct liodom_handle liodom_handle_t;
typedef struct liodom_map liodom_map_t;

/* Params::readParams defaults (src/params.cc:40-109). */
void liodom_params_default(liodom_params_t* p);
void liodom_config_default(liodom_config_t* c);

/* Replaces the construction of FeatureExtractor + LaserOdometer
 * (src/liodom_node.cc:85-86; feature_extractor.cc:24-37; laser_odometry.cc:71-95). */
int liodom_create(const liodom_params_t* params, const liodom_config_t* config, liodom_handle_t** out);
void liodom_destroy(liodom_handle_t* h);
const char* liodom_last_error(void);

/* FeatureExtractor::splitPointCloud + extractFeatures (src/feature_extractor.cc:104-254) for one
 * cloud of stream `stream`.  Extraction side: may run concurrently with liodom_odometry_step.  xyzi: n points (host).  For lidar_type 1, height*width == n and
 * the cloud is row-major organised.  Outputs (host, capacity `cap` edges): edges in the
 * reference's output order (ring-major, region-major, pick order); edge_ring / edge_idx /
 * edge_src (each optional) = ring id, index inside the compacted ring, index into xyzi. */
int liodom_extract_edges(liodom_handle_t* h, int stream, const float* xyzi, int64_t n,
                         int height, int width, float* edges_xyzi, int32_t* edge_ring,
                         int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges);

/* One iteration of LaserOdometer::operator() (src/laser_odometry.cc:107-267) on an edge cloud
 * (sensor frame, host memory; odometry side: may run concurrently with liodom_extract_edges): first call initialises the window, later calls predict, run
 * 2 x [addEdgeConstraints + solve], and append the transformed edges to the sliding window. */
int liodom_odometry_step(liodom_handle_t* h, int stream, const float* edges_xyzi, int n_edges,
                         double stamp, double* pose_out, liodom_step_info_t* info);

/* ---- the same two entry points with the edge cloud staying on the device ----
 * The reference hands every edge cloud from the FeatureExtractor thread to the LaserOdometer thread through a queue
 * (src/shared_data.cc:64-89: pushFeatures / popFeatures).  With the two calls above that queue element is a host cloud: a
 * device-to-host copy on the extraction side, a host-to-device copy on the odometry side, both synchronous, per scan.  Here the
 * queue element is a TICKET: the edges stay in one of three device buffers, the scan's upload is asynchronous, nothing on the
 * extraction side blocks, and the odometry's first kernel waits on the device for the extraction it needs.  One-stream handles.
 *
 *   liodom_extract_edges_device   FeatureExtractor::operator() body up to the hand-over (feature_extractor.cc:49-77): enqueues
 *       upload + extraction of one cloud and returns at once.  LIODOM_ERR_BUSY when all three slots hold clouds that
 *       liodom_odometry_step_device has not taken yet (the reference's queue is unbounded: keep the cloud and retry).
 *       xyzi: any host memory; a buffer from liodom_scan_buffer or one registered with liodom_pin_host_buffer is read
 *       asynchronously (no staging copy) and must then stay untouched until liodom_wait_edges or liodom_odometry_step_device of
 *       the ticket has returned.
 *   liodom_wait_edges             the cloud for the ~edges topic (feature_extractor.cc:70-75): waits until the extraction has
 *       completed and copies the edges out of host-mapped memory the extraction kernel wrote (no device-to-host copy call).
 *       Optional; any thread; before the ticket's liodom_odometry_step_device call returns or — from the extractor thread — before
 *       the ticket is pushed into the queue.
 *   liodom_odometry_step_device   LaserOdometer::operator() body (laser_odometry.cc:107-267) on the ticket's cloud; tickets must
 *       be consumed in the order they were issued.  = liodom_odometry_submit_device + liodom_odometry_collect: a thread that finds
 *       the next ticket already in its queue may submit it before it collects (and publishes) the previous pose — the device then
 *       needs nothing from the host between two scans; at most two scans in flight (LIODOM_ERR_BUSY beyond).  A slot becomes free
 *       for the extraction side when the pose of its scan has been collected.
 *   liodom_scan_buffer            a page-locked buffer (capacity max_points) to assemble the next cloud in — the place of
 *       pcl::fromROSMsg's target in lidarClb (src/liodom_node.cc:43-44); valid until the extraction it is passed to.
 * Poses are bit-identical to liodom_process_scan on the same clouds (tests/test_gpu_threads.py). */
typedef struct liodom_edge_ticket_t {
  uint32_t seq;              /* sequence number of the extraction (never 0) */
  int32_t slot;              /* device edge buffer that holds the cloud */
  int32_t stream;
  int32_t reserved;
} liodom_edge_ticket_t;
int liodom_scan_buffer(liodom_handle_t* h, int stream, float** xyzi, int64_t* capacity_points);
int liodom_extract_edges_device(liodom_handle_t* h, int stream, const float* xyzi, int64_t n, int height, int width,
                                liodom_edge_ticket_t* ticket);
int liodom_wait_edges(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, float* edges_xyzi, int32_t* edge_ring,
                      int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges);
int liodom_odometry_step_device(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, double stamp, double* pose_out,
                                liodom_step_info_t* info);
int liodom_odometry_submit_device(liodom_handle_t* h, const liodom_edge_ticket_t* ticket, double stamp);
int liodom_odometry_collect(liodom_handle_t* h, int stream, double* pose_out, liodom_step_info_t* info);

/* lidarClb -> FeatureExtractor -> LaserOdometer for one scan without leaving the device
 * (src/liodom_node.cc:40-55 + the two worker loops).  pose_out / info / edges outputs optional. */
int liodom_process_scan(liodom_handle_t* h, int stream, const float* xyzi, int64_t n, int height,
                        int width, double stamp, double* pose_out, liodom_step_info_t* info);

/* ---- polar scans: upload range counts, project to XYZI on the device ----
 * No sensor produces packed XYZI.  A Velodyne firing is a 16-bit distance and an 8-bit intensity per laser plus one encoder azimuth
 * per column; an Ouster column is a 32- or 16-bit range and a 16-bit signal per row plus one encoder tick.  In front of the reference
 * the sensor driver projects every return to Cartesian coordinates on a CPU core and pcl::fromROSMsg copies the result into the
 * cloud (lidarClb, src/liodom_node.cc:40-44): 16 bytes per point reach the device.  The calls below take the sensor's own numbers —
 * 3 to 6 bytes per point — and do that projection on the device, on the stream that carries the upload, in front of the unchanged
 * extraction.  Opt-in: a handle that never sets a polar geometry allocates and launches exactly what it does without them.
 *
 * The geometry is made of tables, not angles: the library does no trigonometry and the projected cloud is defined bit for bit.
 * For a point of row `row` with range count c, in a column with encoder tick t (float arithmetic, every product and sum rounded
 * on its own; polar_project_point in liodom_math.h):
 *     r = (float)c * range_unit      d = r - beam_origin      h = d * cos_alt[row]
 *     ct = cos_enc[t] * cos_baz[row] - sin_enc[t] * sin_baz[row]        st = sin_enc[t] * cos_baz[row] + cos_enc[t] * sin_baz[row]
 *     x = h * ct + beam_origin * cos_enc[t]      y = h * st + beam_origin * sin_enc[t]      z = d * sin_alt[row]
 *     w = (float)intensity  (0 without an intensity section)
 * c == 0 (no return) or t >= ticks (then for the whole column): x = y = z = the quiet NaN 0x7FC00000, w is kept; isValidPoint
 * (src/feature_extractor.cc:84-102) drops such points as it drops a driver's NaN returns.
 *
 * A scan is one contiguous little-endian blob (one copy): uint32 tick[width], then the counts [height * width] of range_bits,
 * then the intensities [height * width] of intensity_bits (nothing for 0 bits); every section starts on a 16-byte boundary
 * (liodom_polar_layout).  Point i of the two [height * width] sections is the point i of the packed cloud the handle's lidar_type
 * expects: lidar_type 0: i = col * height + row (firing order); lidar_type 1: i = row * width + col.  Downstream nothing changes:
 * lidar_type 0 still finds the rings by the elevation binning of the projected points, the row is not used as the ring. */
typedef struct liodom_polar_geometry_t {
  int32_t height, width;         /* H rows (beams), W columns; n = H * W points per scan, at most config.max_points; H <= 2048 */
  int32_t range_bits;            /* 16 or 32 */
  int32_t intensity_bits;        /* 0, 8 or 16 */
  float range_unit;              /* metres per count */
  float beam_origin;             /* distance from the lidar origin to the beam origin (Ouster's n); 0 for a Velodyne */
  const float* cos_alt;          /* [H] beam altitude */
  const float* sin_alt;
  const float* cos_baz;          /* [H] azimuth offset of the beam */
  const float* sin_baz;
  int32_t ticks;                 /* T: entries of the encoder table (>= 1) */
  int32_t reserved;
  const float* cos_enc;          /* [T] azimuth of encoder tick t */
  const float* sin_enc;
} liodom_polar_geometry_t;
typedef struct liodom_polar_layout_t {
  int64_t tick_offset;           /* 0 */
  int64_t range_offset;
  int64_t intensity_offset;      /* = total_bytes when intensity_bits is 0 */
  int64_t total_bytes;           /* a multiple of 16 */
} liodom_polar_layout_t;
/* Offsets and size of a blob of this geometry (the tables are not looked at).  Needs no handle and no device.  No counterpart in
 * the reference.  LIODOM_ERR_INVALID_ARG for a range_bits / intensity_bits / height / width the geometry calls refuse. */
int liodom_polar_layout(const liodom_polar_geometry_t* geom, liodom_polar_layout_t* out);
/* Sets (or replaces) the handle's polar geometry — the calibration a sensor driver reads once (beam_altitude_angles /
 * beam_azimuth_angles / lidar_origin_to_beam_origin_mm of an Ouster, the laser corrections of a Velodyne); no counterpart in the
 * reference, which sees projected clouds only.  Copies the tables to the device, allocates three compact staging slots there and
 * a page-locked ring of three blobs on the host.  Not on the per-scan path: takes both sides of the handle and waits for its
 * streams.  LIODOM_ERR_INVALID_ARG: a null table, range_bits not 16 / 32, intensity_bits not 0 / 8 / 16, ticks < 1, height < 1 or
 * > 2048, width < 1; LIODOM_ERR_CAPACITY: height * width > config.max_points; LIODOM_ERR_BUSY: edge tickets are outstanding.  The
 * handle is untouched in every error case (an earlier geometry stays).  Every other polar call returns LIODOM_ERR_UNSUPPORTED until
 * a geometry has been set; n, height and width of a polar scan are the geometry's. */
int liodom_set_polar_geometry(liodom_handle_t* h, const liodom_polar_geometry_t* geom);
/* The driver's projection + pcl::fromROSMsg (src/liodom_node.cc:43-44) alone: projects one blob (host) and returns the packed cloud
 * (host, height * width points) — for callers that publish the cloud, and for tests.  Extraction side. */
int liodom_project_polar(liodom_handle_t* h, const void* blob, float* xyzi_out);
/* liodom_upload_scan for a blob: uploads it and projects it into resident slot `slot` of stream `stream`.  Replaces the driver's
 * projection + pcl::fromROSMsg in front of a resident replay.  Any n_streams; everything resident stays XYZI, so
 * liodom_process_resident* and the subset steps read the slot as they read one written by liodom_upload_scan, and the two may be
 * mixed on one handle. */
int liodom_upload_scan_polar(liodom_handle_t* h, int stream, int slot, const void* blob);
/* liodom_process_scan for a blob: the driver's projection + lidarClb -> FeatureExtractor -> LaserOdometer for one scan
 * (src/liodom_node.cc:40-55 + the two worker loops).  Poses, edges and infos are those of liodom_process_scan on the projected cloud. */
int liodom_process_scan_polar(liodom_handle_t* h, int stream, const void* blob, double stamp, double* pose_out, liodom_step_info_t* info);
/* The ticket path for blobs (one-stream handles): liodom_scan_buffer_polar hands out a page-locked blob (*bytes =
 * liodom_polar_layout's total) to assemble the next scan in — the place of the driver's output buffer and of pcl::fromROSMsg's
 * target in lidarClb; liodom_extract_edges_device_polar is liodom_extract_edges_device (feature_extractor.cc:49-77) with the
 * projection between the upload and the extraction, same slots, same back-pressure (LIODOM_ERR_BUSY), same rules for page-locked,
 * registered and pageable memory.  Its tickets are consumed by liodom_wait_edges and liodom_odometry_*_device like any other. */
int liodom_scan_buffer_polar(liodom_handle_t* h, int stream, void** blob, int64_t* bytes);
int liodom_extract_edges_device_polar(liodom_handle_t* h, int stream, const void* blob, liodom_edge_ticket_t* ticket);

/* mapClb -> SharedData::setLocalMap (src/liodom_node.cc:57-64).  Only with mapping = 1: the next
 * scan's kNN cloud is window ++ this cloud (src/laser_odometry.cc:276-278,310-314). */
int liodom_set_received_map(liodom_handle_t* h, int stream, const float* xyzi, int64_t n);
/* imuClb -> SharedData::setLastIMUOri (src/liodom_node.cc:66-70): latest IMU orientation [x y z w].
 * With use_imu = 1 the roll and pitch of every predicted pose are replaced by the IMU's before the
 * solve (src/laser_odometry.cc:152-183).  Identity until first set.  The quaternion need not be
 * normalised (tf's setRotation divides |q|^2 out; q and -q are the same orientation), but a non-finite
 * component or a norm whose square is 0 — tf would divide by it and every later pose of the stream would
 * be NaN — is LIODOM_ERR_INVALID_ARG: the stored orientation and the stream stay as they were. */
int liodom_set_imu_orientation(liodom_handle_t* h, int stream, const double* q_xyzw);
/* laser_to_base_ (TF lookup at src/laser_odometry.cc:110-119): 3 x 4 row-major, identity by default.
 * It enters the IMU override only; poses are returned in the laser frame (odom_). */
int liodom_set_laser_to_base(liodom_handle_t* h, const double* T);
/* The last received ~map cloud of a stream (inspection). */
int liodom_get_received_map(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points);

/* ---- resident replay (bench / batched streams): scans live in HBM before timing starts ---- */
int liodom_alloc_resident(liodom_handle_t* h, int n_slots);
int liodom_upload_scan(liodom_handle_t* h, int stream, int slot, const float* xyzi, int64_t n);
/* Advance every stream by one scan read from resident slot `slot` (n, height, width as above,
 * identical for all streams).  If poses_out != NULL (n_streams*7 doubles) the call waits for
 * the poses (per-scan synchronous, as the node publishes ~odom per scan); otherwise it only
 * enqueues and poses are read later from the device-side log. */
int liodom_process_resident(liodom_handle_t* h, int slot, int64_t n, int height, int width,
                            double* poses_out, liodom_step_info_t* infos_out);
/* Same, and additionally issues the extraction of resident slot `next_slot` (if >= 0) on a second
 * HIP stream so that it overlaps this scan's odometry — the reference's own two-thread pipeline
 * (FeatureExtractor / LaserOdometer threads, src/liodom_node.cc:89-91).  The following call must
 * then name that slot. */
int liodom_process_resident_pipelined(liodom_handle_t* h, int slot, int next_slot, int64_t n, int height,
                                      int width, double* poses_out, liodom_step_info_t* infos_out);
/* liodom_process_resident_pipelined for some of the streams: the streams in streams[0 .. n_active) — strictly ascending indices
 * in [0, n_streams) — advance by one scan, every other stream sits the step out and keeps its state to the bit.  Stream s reads
 * its scan from resident slot `slot` at its own place (as liodom_upload_scan(h, s, slot, ...) wrote it); n, height and width are
 * per step, not per stream.  The step is ONE launch sequence over n_active rows, whatever the list looks like, and each listed
 * stream's result is bit-identical to the same stream fed the same scans by full steps.  poses_out (n_active * 7 doubles) and
 * infos_out (n_active records) are in list order; both NULL: the step is enqueued only (pose log).  The per-stream getters
 * (liodom_get_edges, liodom_get_correspondences, ...) return a stream's own latest scan, however many steps it has sat out.
 * next_slot >= 0 issues the extraction of that slot ahead for next_streams[0 .. n_next) (NULL: the same list as this step); the
 * next call should name that slot and that list — if it names anything else the extraction is issued again for what it names,
 * results never depend on the hint.  (A hint that names a stream which then sits out overwrites that stream's scratch edges in
 * the pipeline buffer, i.e. what liodom_get_edges shows for it, nothing else.)
 * A list that is not strictly ascending or leaves [0, n_streams), n_active < 0 or n_active > n_streams: LIODOM_ERR_INVALID_ARG,
 * nothing enqueued.  n_active == 0: LIODOM_OK, no stream advances (the extraction ahead is still issued).  The full list
 * 0 .. n_streams-1 (with a full or no list ahead) IS liodom_process_resident_pipelined.  liodom_get_modes: subset_steps counts
 * the steps that ran over a list. */
int liodom_process_resident_subset(liodom_handle_t* h, int slot, const int32_t* streams, int n_active,
                                   int next_slot, const int32_t* next_streams, int n_next,
                                   int64_t n, int height, int width, double* poses_out, liodom_step_info_t* infos_out);
/* The consumer loop of the pipelined replay, in C: resident slots first_slot .. first_slot + count - 1 in order, every
 * scan exactly as liodom_process_resident_pipelined (the extraction of scan k+1 is issued beside the odometry of scan k)
 * and every pose read back, in order — like the LaserOdometer thread that publishes ~odom per scan
 * (src/liodom_node.cc:89-91 / laser_odometry.cc:100-107,403-430).
 * depth = 0: strictly synchronous — pose k is read back before the odometry of scan k+1 is submitted (the GPU idles
 * for the host's turn-around, ~6 us per scan).  depth = 1: the odometry of scan k+1 is submitted before pose k is
 * waited for (the device needs nothing from the host between two scans; poses arrive exactly when they would anyway).
 * `ahead` != 0 also issues the extraction of slot first_slot + count at the end (the next call must start there).
 * poses_out: count * n_streams * 7 doubles; infos_out: count * n_streams records (either may be NULL: then the poses
 * are only waited for). */
int liodom_replay_resident(liodom_handle_t* h, int first_slot, int count, int ahead, int depth, int64_t n, int height, int width,
                           double* poses_out, liodom_step_info_t* infos_out);

/* Host-fed replay: the shape the patched liodom_node sees (scans arrive in HOST memory, one per PointCloud2 message,
 * src/liodom_node.cc:40-55 -> shared_data.cc:37-42).  Scan i of stream s is read from
 * xyzi_base + ((size_t)i * n_streams + s) * scan_stride_floats (n points of packed float4).  The upload of scan k+1
 * (hipMemcpyAsync on the extraction stream into a ring of device staging slots) and its extraction overlap the
 * odometry of scan k; every pose is read back, in order (depth as in liodom_replay_resident).  For the copies to be
 * asynchronous the host buffer must be page-locked: liodom_pin_host_buffer / liodom_unpin_host_buffer register a
 * caller-owned buffer (pageable memory works, the copies then stage through the runtime).  The handle's resident
 * scan buffer is (re)allocated as the staging ring (liodom_alloc_resident(h, 3)) if it has fewer than 3 slots; resident slots
 * 0 .. 2 are overwritten by the replayed scans either way. */
int liodom_replay_host(liodom_handle_t* h, const float* xyzi_base, int64_t scan_stride_floats, int count, int depth,
                       int64_t n, int height, int width, double* poses_out, liodom_step_info_t* infos_out);
int liodom_pin_host_buffer(void* p, int64_t bytes);
int liodom_unpin_host_buffer(void* p);
int liodom_sync(liodom_handle_t* h);
int liodom_get_pose_log(liodom_handle_t* h, int stream, int first, int count, double* poses_out,
                        liodom_step_info_t* infos_out);
/* Pose covariance records (handles created with pose_covariance = 1; else LIODOM_ERR_UNSUPPORTED).
 * liodom_get_pose_covariance_log: entries first .. first + count - 1 of a stream's device-side log, indexed like the pose log
 * (scan k at entry k, scans k >= pose_log_capacity are not logged); same range rules and synchronisation as liodom_get_pose_log.
 * liodom_wait_pose_covariance: the record of scan `scan_index` from host-mapped memory the device writes after every scan (two
 * records per stream: the latest two scans), waited for with a bounded spin — the call for the per-scan paths
 * (liodom_process_scan, liodom_odometry_step, liodom_odometry_collect), after the pose of that scan has been returned.  A scan
 * older than the two kept records, or one not enqueued yet, returns LIODOM_ERR_INVALID_ARG; a wait that runs out returns
 * LIODOM_ERR_HIP, never stale data.  liodom_reset clears the records. */
int liodom_get_pose_covariance_log(liodom_handle_t* h, int stream, int first, int count, liodom_pose_cov_t* out);
int liodom_wait_pose_covariance(liodom_handle_t* h, int stream, int scan_index, liodom_pose_cov_t* out);
/* Resets the odometry state (pose, window, map) of every stream; capacities are kept. */
int liodom_reset(liodom_handle_t* h);

/* ---- streams with a life of their own (no counterpart in the reference: one LaserOdometer object is one stream there) ----
 * The streams of a handle step in lock-step, but each one's odometry state is its own.  The four calls below reset one stream,
 * take its state out of a handle and put a state in, while the other streams keep theirs.  None of them is on the per-scan path:
 * each takes both sides of the handle, waits for all its HIP streams (the other streams stall for the duration of the call) and
 * returns LIODOM_ERR_BUSY while edge tickets of liodom_extract_edges_device are outstanding.  An extraction already issued ahead
 * by the pipelined replay (next_slot) stays valid for every stream.
 *
 *   liodom_reset_stream          what liodom_reset does, for one stream (no counterpart in the reference): the stream's next
 *       scan is its first — window initialisation, no solve, scan_index 0, LIODOM_COV_NO_SOLVE on its covariance record; its
 *       sticky status bits are cleared.  The handle's pipeline (edge buffers, slots, sequence numbers) is left alone, and the
 *       call never switches the handle to safe mode: after LIODOM_STATUS_PIPE_TIMEOUT the recovery remains liodom_reset.
 *   liodom_stream_state_size     upper bound, in bytes, of a state blob of this handle (no counterpart in the reference).
 *   liodom_export_stream_state   the stream's logical state as one blob (no counterpart in the reference): header (magic
 *       "LIODOMST", version, size, and the parameters that must match on import: local_map_size, mapping, filter_local_map,
 *       use_imu, pose_rotation_mode, lm_apply_step_on_ftol), poses, counters and flags, the window frames oldest first as
 *       liodom_get_window orders them, with mapping the received map, with use_imu the last IMU orientation; layout in
 *       DESIGN.md §3.  Derived structures (cell hash, filtered local map) and tuning state do not travel, so a blob fits any
 *       handle with the same parameters, whatever its n_streams and code paths.  An attached liodom_map_t is not part of it: it has a
 *       blob of its own (liodom_map_export_state / liodom_map_import_state below).
 *       cap too small: LIODOM_ERR_CAPACITY with *bytes = the size needed.
 *   liodom_import_stream_state   puts a blob's state into a stream (no counterpart in the reference) and rebuilds what the
 *       stream's next scan searches.  The stream's scan_index, pose log and covariance log carry on from the blob's scan count.
 *       Bad magic / version / size or other parameters: LIODOM_ERR_INVALID_ARG; a frame larger than the handle's edge capacity
 *       or a map larger than recv_capacity: LIODOM_ERR_CAPACITY; the handle is untouched in both cases.  Importing the state of
 *       a stream that never ran equals liodom_reset_stream.
 * A continuation after export / import is bit-identical to the uninterrupted run on a handle of the same shape
 * (tests/test_gpu_stream_state.py). */
int liodom_reset_stream(liodom_handle_t* h, int stream);
int liodom_stream_state_size(liodom_handle_t* h, int64_t* max_bytes);
int liodom_export_stream_state(liodom_handle_t* h, int stream, void* blob, int64_t cap, int64_t* bytes);
int liodom_import_stream_state(liodom_handle_t* h, int stream, const void* blob, int64_t bytes);

/* ---- inspection (tests, parity checks) ---- */
/* Edges of the last scan of a stream as left on the device by process_scan / process_resident. */
int liodom_get_edges(liodom_handle_t* h, int stream, float* edges_xyzi, int32_t* edge_ring,
                     int32_t* edge_idx, int32_t* edge_src, int cap, int* n_edges);
/* Sliding-window points in LocalMapManager order (oldest frame first). */
int liodom_get_window(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points,
                      int* n_frames);
/* The cloud the next scan's kNN will search (computeLocalMap, src/laser_odometry.cc:274-298): the
 * window, or — with filter_local_map and a full window — its VoxelGrid(0.4) down-sampling in
 * PCL's output order (ascending leaf index).  *filtered tells which. */
int liodom_get_local_map(liodom_handle_t* h, int stream, float* xyzi, int64_t cap, int64_t* n_points, int* filtered);
/* Correspondences of outer iteration `it` (0/1) of the last step: valid flag and window
 * indices (as in liodom_get_window; PCL leaf indices when the local map is filtered) of the two
 * line points per edge. */
int liodom_get_correspondences(liodom_handle_t* h, int stream, int it, int32_t* valid,
                               int32_t* idx_a, int32_t* idx_b, int cap, int* n);
/* World-frame float queries (edges transformed by the pose entering outer iteration `it`,
 * src/laser_odometry.cc:307-308) of the last step: n x float[4] (x y z 0).  debug_buffers = 1 only.
 * Together with liodom_get_local_map (taken before the step) they are the exact inputs of the 5-NN +
 * line-gate kernel, so that its output can be compared bit for bit with the oracle on identical inputs. */
int liodom_get_knn_queries(liodom_handle_t* h, int stream, int it, float* xyz0, int cap, int* n);
/* Smoothness values of the last extracted scan, ring-major over the compacted rings; also the
 * ring offsets (scan_lines + 1 entries).  NaN where the stencil is undefined. */
int liodom_get_curvature(liodom_handle_t* h, int stream, double* curv, int64_t cap,
                         int32_t* ring_offsets);

/* ---- measurement ---- */
/* When enabled every kernel launch is bracketed by HIP events on the handle's stream. */
int liodom_set_profiling(liodom_handle_t* h, int enable);
#define LIODOM_NUM_KERNELS 12
typedef struct liodom_kernel_stat_t {
  char name[32];
  int64_t launches;
  double total_ms;
} liodom_kernel_stat_t;
/* Drains recorded events (synchronises) and accumulates into the per-kernel table. */
int liodom_get_kernel_stats(liodom_handle_t* h, liodom_kernel_stat_t* stats /*LIODOM_NUM_KERNELS*/);
int liodom_reset_kernel_stats(liodom_handle_t* h);
/* Number of HIP devices visible to this process (0 without a GPU). */
int liodom_device_count(int* count);
/* PCI bus id ("0000:c1:00.0") of HIP device `device`: lets a launcher place the host thread that
 * polls the result records on the GPU's NUMA node (/sys/bus/pci/devices/<id>/local_cpulist). */
int liodom_device_pci_bus_id(int device, char* bus_id, int cap);
/* Device name and compute-unit count of the handle's GPU. */
int liodom_device_info(liodom_handle_t* h, char* name, int name_cap, int* compute_units);
/* The code paths this handle runs, as "key=value key=value ..." (stream-dependency mechanism, hash rebuild variant,
 * workgroups per solve, kNN tuning, test switches picked up from the environment at liodom_create).  Every variant
 * produces the same results (each has an equality test); measurements quote this string next to their numbers. */
int liodom_get_modes(liodom_handle_t* h, char* buf, int cap);


/* ---- liodom::Map on the device (mapping node, src/map.cc, src/liodom_mapping_node.cc) ---- */
typedef struct liodom_map_config_t {
  int32_t device;              /* HIP device ordinal */
  int32_t max_cells;           /* coarse cells the map can hold (cells_vector_) */
  double voxel_xysize;         /* ~voxel_xysize, liodom_mapping_node.cc:115-117  default 40 */
  double voxel_zsize;          /* ~voxel_zsize,  :119-121  default 50 */
  double resolution;           /* ~resolution,   :123-125  default 0.4 */
  int32_t cell_capacity;       /* points per cell (after filtering, and filtered + appended during an update) */
  int32_t max_update_points;   /* points per updateMap call; any value >= 1, whatever the other capacities are */
  int32_t max_modified_cells;  /* cells touched by one updateMap call (<= 256) */
  int32_t reserved;
} liodom_map_config_t;
/* status bits of liodom_map_status */
#define LIODOM_MAP_UPDATE_OVERFLOW 1u
#define LIODOM_MAP_CELLS_FULL 2u
#define LIODOM_MAP_MODIFIED_FULL 4u
#define LIODOM_MAP_CELL_OVERFLOW 8u
#define LIODOM_MAP_LEAF_RANGE 16u
#define LIODOM_MAP_KEY_RANGE 32u
#define LIODOM_MAP_RESULT_OVERFLOW 64u
/* LIODOM_MAP_RESULT_OVERFLOW says that a getLocalMap left the device incomplete.  Sticky like the other bits (liodom_map_reset
 * clears them; an import takes the blob's).  Raised when
 *   - a STEP's local map (an attached mapper's or a map reader's, after every scan) is larger than the handle's recv_capacity: the
 *     stream receives the first recv_capacity points in visit order (the reference's loops, a cell cut where the capacity ends), its
 *     received map holds exactly recv_capacity points, and the next scan searches window ++ that truncated cloud.  The host getters
 *     (liodom_map_get_local, liodom_map_get_local_batch, liodom_seed_stream) do NOT raise it for a result larger than the
 *     caller's buffer: they return LIODOM_ERR_CAPACITY with the full size, copy nothing and leave the status alone;
 *   - one visit finds more than 4096 cells: the result holds the first 4096 found cells in visit order;
 *   - a visit is cut by the planners' loop guard, 65536 iterations of the visit's loops (the inner and the outer ones counted
 *     together): the result holds the cells found up to the cut.  cells_xy * 2 + 1 = 255 keys a side (cells_xy = 127 on 1 m
 *     cells) is the largest square that stays under it.
 * The last two are raised by steps and host getters alike, and the call returns what it has. */

void liodom_map_config_default(liodom_map_config_t* c);
/* Map::Map (src/map.cc:70-81) */
int liodom_map_create(const liodom_map_config_t* config, liodom_map_t** out);
void liodom_map_destroy(liodom_map_t* m);
/* Map::updateMap (src/map.cc:90-129): xyzi = n sensor-frame points (host), T = world<-sensor
 * isometry as 12 doubles, row-major 3 x 4 (the Eigen::Isometry3d of liodom_mapping_node.cc:63-64). */
int liodom_map_update(liodom_map_t* m, const float* xyzi, int64_t n, const double* T);
/* Map::getLocalMap (src/map.cc:141-189) with the node's ~cells_xy / ~cells_z
 * (liodom_mapping_node.cc:130-134, defaults 2 and 1).  Output order = the reference's loops. */
int liodom_map_get_local(liodom_map_t* m, const double* T, int cells_xy, int cells_z, float* xyzi,
                         int64_t cap, int64_t* n_points);
/* Map::getMap (src/map.cc:131-139): every cell in creation order, for any number of cells up to max_cells: the point section
 * of liodom_map_export_state's blob.  *n_points is the size of the whole result; LIODOM_ERR_CAPACITY (nothing written) if it
 * is larger than cap. */
int liodom_map_get_all(liodom_map_t* m, float* xyzi, int64_t cap, int64_t* n_points);
int liodom_map_num_cells(liodom_map_t* m, int* n_cells);
/* Wires a map to stream `stream` of an odometry handle created with mapping = 1, replaying the
 * two-node loop of launch/liodom.launch:41-56 synchronously on the device: after every scan k the
 * handle enqueues updateMap(edges_k, pose_k) (lidarClb, liodom_mapping_node.cc:45-69) and
 * getLocalMap(pose_k, cells_xy, cells_z) (:78-86) whose result becomes the received map of scan
 * k+1 (mapClb, liodom_node.cc:57-64) without leaving HBM.  (The reference's two nodes run
 * asynchronously, so which map a scan sees is timing dependent there; this is the zero-latency
 * case.)  The map must live on the handle's device; from here on it uses the handle's HIP stream.
 * Pass map = NULL to detach. */
int liodom_attach_mapper(liodom_handle_t* h, int stream, liodom_map_t* m, int cells_xy, int cells_z);
/* How a map is wired to a stream (no counterpart in the reference: its mapper is a node of its own, fed every scan). */
typedef struct liodom_mapper_options_t {
  int32_t cells_xy, cells_z;   /* getLocalMap extent, as liodom_attach_mapper (defaults 2, 1) */
  int32_t lag;                 /* 0 (default): the reference replay, insert scan k after scan k.
                                  1: insert a frame when it leaves the sliding window */
  int32_t prune_period;        /* 0 (default): never.  n > 0: prune after the map update of every scan
                                  with (scan_index + 1) % n == 0, around that scan's pose */
  int32_t keep_cells_xy, keep_cells_z;   /* the box pruning keeps (liodom_map_prune) */
  int32_t reserved[2];
} liodom_mapper_options_t;
/* cells 2 / 1, lag 0, no pruning: what liodom_attach_mapper does (no counterpart in the reference). */
void liodom_mapper_options_default(liodom_mapper_options_t* options);
/* liodom_attach_mapper with options (no counterpart in the reference); liodom_attach_mapper(h, s, m, cxy, cz) IS this call with
 * the defaults and those two extents.  options = NULL: the defaults.  map = NULL detaches.
 *   lag = 0  the synchronous replay above.  Faithful, and degenerate: single-point leaves of the map are bit-copies of window
 *            points, the line through NN0 == NN1 has zero length, both solves end with termination 5 and every pose is the
 *            constant-velocity prediction.
 *   lag = 1  scan-to-map odometry that solves: the map holds only what has LEFT the sliding window.  One step of stream s, scan k:
 *            (1) if the window is full, the frame scan k's append will overwrite — the oldest frame liodom_get_window shows before
 *            the step — is copied aside with its count; (2) scan k's odometry runs as ever, against window ++ received map;
 *            (3) the copy enters the map as it is: the window's own world-frame float points, bit for bit, no transform (nothing
 *            while the window is not full); (4) the optional prune; (5) getLocalMap(pose_k, cells_xy, cells_z) into the stream's
 *            received-map buffer.  Ordered by HIP stream order alone; nothing is pending between two steps, so the blobs of
 *            liodom_export_stream_state / liodom_map_export_state and the checkpoint order stay as they are — give the options
 *            again at attach.  Costs one edge-capacity frame per stream of the handle, allocated by the first such attach.
 *   prune_period = n > 0  liodom_map_prune(pose_k, keep_cells_xy, keep_cells_z) on the device after the map update of every scan
 *            with (scan_index + 1) % n == 0.  Needs keep_cells_xy >= cells_xy and keep_cells_z * voxel_zsize >= cells_z *
 *            voxel_xysize (the reference's z column takes its extent from the xy size): the keep box then holds every cell
 *            getLocalMap visits for the same pose, and pruning cannot change what the next scan sees.
 * LIODOM_ERR_INVALID_ARG (attachment unchanged) for a negative extent or period, lag other than 0 / 1, or options that break the
 * auto-prune conditions.  Streams without a mapper, streams that sit a subset step out and liodom_reset_stream are untouched by
 * all of this.  liodom_get_modes reports mapper_lag=<streams with a lagged mapper>. */
int liodom_attach_mapper_ex(liodom_handle_t* h, int stream, liodom_map_t* m, const liodom_mapper_options_t* options);
/* ---- localising in a saved map (no counterpart in the reference: its odometer starts at the identity and its mapper always
 * writes).  mapping = 1 handles only; nothing of the kNN passes, the solve or the rebuild changes: a seeded stream's first scan
 * and every scan of a reader are ordinary steady-state scans against window ++ received map. ----
 *
 *   liodom_attach_map_reader   wires a map to a stream READ-ONLY (no counterpart in the reference).  After every scan k of the
 *       stream the handle enqueues getLocalMap(pose_k, cells_xy, cells_z) into the stream's received-map buffer and nothing else:
 *       no update, no prune, nothing set aside.  The map stays fixed: liodom_map_export_state before and after a run is the same
 *       bytes.  One map may be read by any number of streams of ONE handle; a step costs one launch per distinct map over the
 *       step's reader rows (k_map_local_rows; a reader whose extents visit more than 1024 keys takes the two launches of
 *       liodom_map_get_local).  The map uses the handle's HIP stream from its first attachment until its last one goes.  A map
 *       is read or written, not both: attaching a reader to a map that liodom_attach_mapper[_ex] holds, or the reverse, in
 *       either order, is LIODOM_ERR_INVALID_ARG with the attachments unchanged; so are a negative extent and a map another handle
 *       holds.  liodom_attach_mapper(h, s, NULL, ..) detaches either kind, as does map = NULL here.  liodom_map_update, _prune,
 *       _evict and _merge_state from the host keep working on a read-attached map between steps, as on any attached map (a pager
 *       can window a site map under its readers).  Streams that sit a subset step out are untouched.  liodom_get_modes reports
 *       map_readers=<streams with a reader>.
 *   liodom_seed_stream         the stream's next scan is its first AND it solves (no counterpart in the reference).  pose =
 *       [qx qy qz qw tx ty tz]; the quaternion is normalised in double, the matrix T made from it as the solve makes its own.
 *       The call takes both sides of the handle and waits for its HIP streams, like liodom_reset_stream, then installs a fresh
 *       state: initialised, an empty window, scan_index 0, odom = prev_odom = final_odom = T, the solve's start point = the
 *       seed.  The first scan therefore searches and solves from the seed itself (a zero-velocity prediction, no arithmetic
 *       applied to it), gets a pose-log entry and — with pose_covariance = 1 — a LIODOM_COV_VALID record.  If a mapper or a
 *       reader is attached to the stream, its received map becomes getLocalMap(T, cells_xy, cells_z) of that map; a result
 *       larger than recv_capacity is LIODOM_ERR_CAPACITY and leaves the stream untouched.  Without an attachment the received
 *       map is empty and liodom_set_received_map may follow.  mapping = 0: LIODOM_ERR_UNSUPPORTED; a non-finite pose or
 *       | |q| - 1 | > 1e-6: LIODOM_ERR_INVALID_ARG; outstanding edge tickets: LIODOM_ERR_BUSY.  The other streams keep
 *       everything to the bit.  The state of a seeded stream exports and imports like any other, before its first scan too.
 *   liodom_map_get_local_batch liodom_map_get_local for n poses in one launch (no counterpart in the reference).  T = n x 12
 *       doubles; row i's cloud goes to xyzi + 4 * i * cap_per_row, its FULL size to n_points[i].  Every row is what
 *       liodom_map_get_local returns for that pose, bit for bit.  If any row is larger than cap_per_row the call returns
 *       LIODOM_ERR_CAPACITY with every size reported and nothing written to xyzi (cap_per_row = 0, xyzi = NULL asks for the
 *       sizes).  Works on a detached map and on an attached one, with the threading rule of liodom_map_export_state. */
int liodom_attach_map_reader(liodom_handle_t* h, int stream, liodom_map_t* m, int cells_xy, int cells_z);
int liodom_seed_stream(liodom_handle_t* h, int stream, const double* pose /*[7]*/);
int liodom_map_get_local_batch(liodom_map_t* m, const double* T /*n x 12*/, int n, int cells_xy, int cells_z, float* xyzi,
                               int64_t cap_per_row, int64_t* n_points /*[n]*/);
/* ---- knowing that a reader is lost: per-scan map-hit records (no counterpart in the reference; DESIGN.md §3 "Knowing that a
 * reader is lost").  liodom_step_info_t counts matches against window ++ received map: a stream that slides
 * along its own window keeps them high while it leaves the map.  These records hold, per scan and from the device, the two counts
 * the relocaliser ranks by, taken at the pose the scan returned.  Everything is opt-in: a handle that never calls
 * liodom_set_map_hits allocates and launches what it always did.
 *
 *   liodom_set_map_hits     radius 0 | 1 switches the records of one stream on (or changes the radius), -1 switches them off.
 *       mapping = 1 handles only (else LIODOM_ERR_UNSUPPORTED).  The call takes both sides of the handle and waits for its HIP
 *       streams, like liodom_attach_map_reader; LIODOM_ERR_BUSY while edge tickets are outstanding; a bad stream or radius is
 *       LIODOM_ERR_INVALID_ARG with the handle untouched.  The first enabling call allocates the log: pose_log_capacity records
 *       of 128 bytes per stream, indexed like the pose log.  While it is on, the stream gets one record for every scan that gets
 *       a pose-log entry (scans at or beyond pose_log_capacity are not logged; a stream that sits a subset step out gets none
 *       for that step).  The setting survives liodom_reset, liodom_reset_stream, liodom_seed_stream and
 *       liodom_import_stream_state, which move the log index exactly as they move the pose-log index.  liodom_get_modes reports
 *       map_hits=<streams with it on> when that is not 0.
 *   the record              edges = scan k's edge cloud as it lies in the handle's edge buffer (sensor frame: what the stream's
 *       mapper would be given), T = the stream's final pose of scan k as the 3 x 4 matrix the device holds, copied into the
 *       record.  hits_r, hits_0 are what liodom_map_score_poses(map, edges_k, n_edges, rec.T, 1, radius) returns: same probes,
 *       keys, leaf test and finiteness rules.  Nothing of the map is written.  The occupancy is kept between scans while the
 *       map does not change: every call and every enqueue that can change the map's cells (liodom_map_update, _prune, _evict,
 *       _merge_state, _import_state, _reset, a writing mapper's step) invalidates it, and the next step that needs it builds it
 *       again, on the handle's stream.  It has a row for each of the map's max_cells cells (4 bytes per 32 leaves each),
 *       allocated when hits are first on for a stream that reads the map, never inside a step.
 *       A stream without a reader — none attached, or a WRITING mapper (liodom_attach_mapper[_ex]) — gets LIODOM_HIT_NO_READER
 *       records with zero counts and n_edges 0: counting against a map that changes every scan is out of scope.
 *   liodom_get_map_hit_log  records first .. first + count - 1 of a stream, with the range rules and the synchronisation of
 *       liodom_get_pose_log; LIODOM_ERR_UNSUPPORTED on a handle that never switched the records on.  Entries no scan has
 *       written have flags 0.  (An un-synchronised per-scan wait, as liodom_wait_pose_covariance is for its record, does not exist.)
 *   liodom_map_hit_rows     the kernel's public form: row i probes its own cloud, edges_xyzi + 4 * i * edge_stride_points with
 *       n_edges[i] points, under T + 12 i; hits[2 i], hits[2 i + 1] = hits_r, hits_0.  Works on detached and attached maps.
 *       Limits, argument rules, threading rule, read-only guarantee and error codes are those of liodom_map_score_poses:
 *       n <= 2^20, 0 <= n_edges[i] <= edge_stride_points <= max_update_points, radius 0 | 1.  n = 0, or an n_edges that is 0
 *       everywhere: LIODOM_OK with zero counts.  It rebuilds the occupancy on every call, as liodom_map_score_poses does. */
typedef struct liodom_map_hit_t {
  int32_t scan_index;      /* = liodom_step_info_t.scan_index of the same scan */
  uint32_t flags;          /* LIODOM_HIT_* */
  int32_t n_edges;         /* edges of the scan that were probed */
  int32_t hits_r, hits_0;  /* as liodom_map_score_poses defines them */
  int32_t radius;          /* 0 | 1 */
  int32_t reserved[2];
  double T[12];            /* the matrix the counts were taken under: the stream's final pose of this scan, 3 x 4 row-major */
} liodom_map_hit_t;        /* 128 bytes */
#define LIODOM_HIT_VALID 1u      /* a reader was attached and the scan was counted */
#define LIODOM_HIT_NO_READER 2u  /* no reader on the stream at this scan: counts 0 */
#define LIODOM_HIT_NO_SOLVE 4u   /* first scan of an unseeded stream: counted under the initial pose (may accompany VALID) */
int liodom_set_map_hits(liodom_handle_t* h, int stream, int radius /* -1 off, 0, 1 */);
int liodom_get_map_hit_log(liodom_handle_t* h, int stream, int first, int count, liodom_map_hit_t* out);
int liodom_map_hit_rows(liodom_map_t* m, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges /*[n]*/,
                        const double* T /*n x 12*/, int n, int radius /*0 | 1*/, int32_t* hits /*n x 2: hits_r, hits_0*/);
/* Sticky LIODOM_MAP_* bits raised by the device since creation. */
int liodom_map_status(liodom_map_t* m, uint32_t* status);

/* ---- the map as a blob (no counterpart in the reference: a Map lives and dies with its node there) ----
 * A map's LOGICAL state as one blob: header (magic "LIODOMMP", version, size, and the three sizes voxel_xysize, voxel_zsize,
 * resolution, which must match bit for bit on import; n_cells, the sticky LIODOM_MAP_* bits, n_points), one 32-byte record per
 * cell in creation order (key, leaf coordinates of the cell's lower corner, count, index of its first point), then the cells'
 * clouds back to back: the bytes liodom_map_get_all returns.  Layout in liodom_amd/csrc/map_state_format.h and DESIGN.md §3.
 * Capacities do not travel: the importing map may have another max_cells, cell_capacity, max_update_points and
 * max_modified_cells than the exporting one.  None of these calls is on the per-scan path.
 *
 *   liodom_map_state_size     exact size, in bytes, of a blob of the map as it is now (no counterpart in the reference).
 *       Synchronises the stream the map's work is enqueued on.
 *   liodom_map_export_state   writes the blob (no counterpart in the reference).  Works on a detached map and on one attached to
 *       a handle; it synchronises the stream the map's work is enqueued on, and — as with liodom_map_update — the caller must not
 *       step the handle from another thread during the call.  cap too small: LIODOM_ERR_CAPACITY with *bytes = the size needed
 *       and nothing written to the buffer.
 *   liodom_map_import_state   makes the map what the blob says (no counterpart in the reference).  The blob is validated on the
 *       host before anything is launched: truncation, bad magic / version / sizes, a negative count, counts that do not add up,
 *       a key beyond +-2^20, a duplicate key or other voxel sizes / resolution: LIODOM_ERR_INVALID_ARG; more cells than max_cells
 *       or a cell larger than cell_capacity: LIODOM_ERR_CAPACITY.  On any error the map is untouched and liodom_last_error names
 *       the reason.  Importing a blob of 0 cells equals liodom_map_reset.
 *   liodom_map_reset          the map as liodom_map_create left it — no cells, status 0 (no counterpart in the reference);
 *       capacities and allocations are kept.
 * Import and reset on a map that is attached to a handle return LIODOM_ERR_BUSY: detach (liodom_attach_mapper with NULL), import,
 * attach.  A mapping-mode stream is checkpointed with liodom_export_stream_state + liodom_map_export_state and resumed with
 * liodom_map_import_state, liodom_import_stream_state, liodom_attach_mapper, in this order.
 * After an import, the imported map and an uninterrupted one give bit-identical answers to every later liodom_map_update,
 * liodom_map_get_all, liodom_map_get_local and liodom_map_num_cells (tests/test_gpu_map_state.py). */
int liodom_map_state_size(liodom_map_t* m, int64_t* bytes);
int liodom_map_export_state(liodom_map_t* m, void* blob, int64_t cap, int64_t* bytes);
int liodom_map_import_state(liodom_map_t* m, const void* blob, int64_t bytes);
int liodom_map_reset(liodom_map_t* m);

/* Drops every cell outside a box of cells around a pose (no counterpart in the reference, whose map only grows until
 * LIODOM_MAP_CELLS_FULL).  T = 3 x 4 pose, row-major; the centre cell (vx, vy, vz) is computed from it as Map::getLocalMap does
 * (src/map.cc:144-151: the translation truncated to int first, then the cell key).  A cell with key (kx, ky, kz) is kept iff
 * |kx - vx| <= keep_cells_xy * voxel_xysize, |ky - vy| <= keep_cells_xy * voxel_xysize and |kz - vz| <= keep_cells_z * voxel_zsize
 * (compared in double; a plain box, not getLocalMap's cross-shaped visit).  Afterwards the map is what liodom_map_import_state
 * would make of its own exported blob with the dropped cells' records and points taken out: survivors keep their relative
 * creation order, slots an earlier LIODOM_MAP_CELLS_FULL marked "no room" are gone (new cells can be created again), sticky status
 * bits stay.  *n_removed (optional) = cells dropped.  Works on a detached map and on an attached one, where it is enqueued on the
 * stream the map's work is on; it synchronises, with the threading rule of liodom_map_export_state.  LIODOM_ERR_INVALID_ARG for a
 * null map or T or a negative keep: the map is untouched.  The first prune of a map allocates 16 bytes per max_cells. */
int liodom_map_prune(liodom_map_t* m, const double* T /*3x4*/, int keep_cells_xy, int keep_cells_z, int* n_removed);

/* Paging: the device map as a window onto a larger map the caller keeps on the host (liodom_amd/pager.py, liodom::MapPager).
 *
 *   liodom_map_evict          liodom_map_prune whose dropped cells come out (no counterpart in the reference).  Same centre cell and
 *       keep box, bit for bit.  `blob` receives a well-formed map-state blob of this map's three sizes that holds exactly the
 *       dropped cells, in their relative creation order: each with its own key and corner_leaf and the points of its current cloud,
 *       `first` recomputed, status 0 (a tile has no history).  Afterwards the map is what liodom_map_prune would have left.
 *       *bytes is always the size needed, and it is known before anything is modified: with cap too small the call returns
 *       LIODOM_ERR_CAPACITY, writes nothing to `blob` and leaves the map untouched (cap = 0, blob = NULL asks for the size).  When
 *       nothing is dropped the blob is a 64-byte header with 0 cells.  *n_evicted (optional) = cells dropped.  Works on a detached
 *       map and on an attached one, where it is enqueued on the stream the map's work is on; it synchronises, with the threading
 *       rule of liodom_map_export_state.  LIODOM_ERR_INVALID_ARG for a null map, T or bytes, or a negative keep.
 *   liodom_map_merge_state    appends a blob's cells to a map that may already hold cells (no counterpart in the reference).  The
 *       blob is validated on the host first, as liodom_map_import_state does: LIODOM_ERR_INVALID_ARG for malformed bytes or other
 *       sizes, LIODOM_ERR_CAPACITY for a cell larger than cell_capacity or more cells than max_cells.  A blob cell whose key is
 *       already a cell of the map is skipped (taken[i] = 0; that cell of the map is untouched); the others (taken[i] = 1) are
 *       appended behind the map's cells in blob order.  Afterwards the map is what liodom_map_import_state would make of its own
 *       blob with the taken cells' records and points appended; sticky status = the map's OR the blob's.  Not enough free cell ids
 *       for the taken cells: LIODOM_ERR_CAPACITY, map untouched.  Merging into an empty map equals liodom_map_import_state; a blob
 *       of 0 cells is a no-op.  `taken` (optional) has room for the blob's n_cells entries; *n_added (optional) = cells taken.
 *       Allowed on an attached map (unlike liodom_map_import_state), enqueued and synchronised as liodom_map_prune is. */
int liodom_map_evict(liodom_map_t* m, const double* T /*3x4*/, int keep_cells_xy, int keep_cells_z, void* blob, int64_t cap,
                     int64_t* bytes, int* n_evicted);
int liodom_map_merge_state(liodom_map_t* m, const void* blob, int64_t bytes, int32_t* taken /*optional, [blob n_cells]*/, int* n_added);

/* ---- relocalising in a saved map: candidate poses of one scan's edge cloud scored against the map's leaf occupancy (no
 * counterpart in the reference).  liodom_seed_stream wants a pose right to within decimetres; these calls find one from a guess
 * that is metres and tenths of a radian off (DESIGN.md §3 "Relocalising in a saved map").
 *
 * Occupancy: for every cell of the map and every finite point p of its current cloud, the leaf of p in the cell's dense leaf grid
 * (the grid liodom_map_update filters with: PCL VoxelGrid leaves of `resolution`) is occupied; a point whose leaf falls outside
 * the grid occupies nothing.  It is rebuilt from the map as it is by every call: nothing is cached between calls.
 * An edge e under a candidate T (3 x 4 doubles, row-major): q = float(T * e), computed as liodom_map_update transforms an inserted
 * point.  A probe at a float point p hits iff p is finite, its coarse-cell key lies within +-2^20, the map holds that cell, and
 * p's leaf lies inside the cell's grid and is occupied.  The centre probe is q; with radius = 1 there are 27 probes
 * q + d * float(resolution), d in {-1, 0, 1}^3 (float multiply, then float add, per axis), each keyed as a point in its own right:
 * a probe displaced across a coarse-cell face is looked up in the neighbour cell.  Per candidate two counts:
 *   hits_r = edges with at least one hitting probe, hits_0 = edges whose centre probe hits (radius = 0: hits_r == hits_0).
 * Ranking: score = hits_r + hits_0; the best candidate has the largest score, ties go to the lowest index.
 *
 *   liodom_map_score_poses   hits[2 i], hits[2 i + 1] = hits_r, hits_0 of candidate T + 12 i (no counterpart in the reference).
 *   liodom_pose_search_default   centre = identity, steps 0.4 m / 0.4 m / 0.02 rad, all half counts 0, radius 1 (no counterpart
 *       in the reference).
 *   liodom_map_search_pose   scores a grid of candidates around `centre` and returns the best (no counterpart in the reference).
 *       Candidate (ix, iy, ia, iz), each index from -n to n, ix fastest, then iy, then ia (yaw), iz slowest:
 *         T = [ Rz(ia * step_yaw) * R_c | t_c + (ix * step_xy, iy * step_xy, iz * step_z) ],
 *       yaw about the world z axis, R_c from the centre's quaternion, normalised in double, as liodom_seed_stream makes its matrix.
 *       The matrices are made on the host in double (liodom_amd/csrc/reloc_candidates.h); only the result record and the optional
 *       arrays come back.  out->pose is the best candidate as liodom_seed_stream takes it.
 * Limits: n_edges <= the map's max_update_points; n and n_candidates <= 2^20.  n = 0 or n_edges = 0: LIODOM_OK with zero counts
 * (the search then reports index 0).  LIODOM_ERR_INVALID_ARG, with nothing computed: a null where one is required, radius not 0 or
 * 1, a negative count, a non-positive (or non-finite) step whose half count is > 0, a non-finite centre, | |q| - 1 | > 1e-6,
 * anything beyond the limits.  Non-finite edges are no error: they miss.
 * Both calls only read the map (no status bit, no cell, no plan entry changes): they work on a detached map and on an attached one
 * — reading or writing — between steps, on the stream the map's work is on, and synchronise it before returning, with the threading
 * rule of liodom_map_export_state.  The first call allocates the occupancy, 4 bytes per 32 leaves of the cells the map holds. */
typedef struct liodom_pose_search_t {
  double centre[7];            /* qx qy qz qw tx ty tz; normalised in double as liodom_seed_stream does */
  double step_xy, step_z, step_yaw;
  int32_t nx, ny, nz, nyaw;    /* half counts: the grid has (2nx+1)(2ny+1)(2nz+1)(2nyaw+1) candidates */
  int32_t radius;              /* 0 | 1 */
  int32_t reserved[3];
} liodom_pose_search_t;
typedef struct liodom_pose_search_result_t {
  int32_t best_index, hits_r, hits_0, n_candidates;
  double pose[7];              /* best candidate, quaternion normalised: what liodom_seed_stream takes */
  double T[12];
} liodom_pose_search_result_t;
int liodom_map_score_poses(liodom_map_t* m, const float* edges_xyzi, int n_edges, const double* T /*n x 12*/, int n,
                           int radius /*0 | 1*/, int32_t* hits /*n x 2: hits_r, hits_0*/);
void liodom_pose_search_default(liodom_pose_search_t* s);
int liodom_map_search_pose(liodom_map_t* m, const float* edges_xyzi, int n_edges, const liodom_pose_search_t* s,
                           liodom_pose_search_result_t* out, double* T_out /*optional, n_candidates x 12*/,
                           int32_t* hits_out /*optional, n_candidates x 2*/);

/* ---- relocalising over a wide window: the same grid, the same ranking, by branch-and-bound (no counterpart in the reference;
 * DESIGN.md §3 "Branch-and-bound over the candidate grid").  liodom_map_search_pose scores every candidate and
 * takes at most 2^20; this call takes up to 2^31 - 1 (per axis and in all) and scores few of them.
 *
 * A node is a rectangle of candidates ix0..ix1 x iy0..iy1 that share ia and iz.  T_lo is the matrix of (ix0, iy0), t_hi = T[3], T[7]
 * of (ix1, iy1); the rest of the matrix is the same for the whole node.  Leaf of a float coordinate p: floorf(p * (1.f /
 * (float)resolution)), "in range" iff it lies in [-2^20, 2^20).  Block set B_h, h = 1 .. 21: the keys (lx >> h, ly >> h, lz) of every
 * finite point of the map whose three leaves are in range (arithmetic shift; blocks in x and y only), rebuilt from the map as it is by
 * every call, for the levels the call uses: nothing is cached.  Per edge e with q_lo = float(T_lo * e), q_hi = float(T_hi * e):
 *   ub_0 = 1 iff B_h holds a key (bx, by, lz) with bx in [leaf(q_lo.x) >> h, leaf(q_hi.x) >> h], by likewise, lz = leaf(q.z);
 *   ub_r = the same with the ranges [leaf(q_lo.x + (-1.f) * leaf) >> h, leaf(q_hi.x + 1.f * leaf) >> h] and lz among the leaves of
 *          q.z + (j - 1) * leaf, j = 0, 1, 2 (radius 0: ub_r = ub_0).
 * An edge with a non-finite coordinate counts in neither.  A finite edge counts in both, with no lookup, if one of the leaves above
 * is not in range (non-finite extremes included) or a range spans more than three blocks.  The node's bound is the sum of ub_r plus
 * the sum of ub_0 over the edges: it is >= hits_r + hits_0 of every candidate of the node, whatever the map, the edges and the level.
 *
 *   liodom_map_bound_nodes   ub[2 i], ub[2 i + 1] = sums of ub_r, ub_0 of node i (T_lo + 12 i, t_hi + 2 i) at one level 1 .. 21.
 *       n <= 2^20; n = 0 or n_edges = 0: LIODOM_OK (zero bounds).
 *   liodom_pose_search_bnb_default   batch = 1024.
 *   liodom_map_search_pose_bnb   the best candidate of the grid `s`: `out` is field for field what liodom_map_search_pose returns for
 *       the same inputs.  Roots: one node per (ia, iz), 2^K wide, covering the xy grid; a node splits into up to four children
 *       clipped to the grid, each bounded at the level liodom_amd/csrc/reloc_bnb.h gives for its width, a child's bound being
 *       min(its own, its parent's).  Rounds: drop the open nodes that cannot win (bound < the best score, or equal with a lowest
 *       index above the best's), take the `batch` with the largest bound (ties to the lowest index), score the width-1 nodes among
 *       them exactly (k_map_score_poses, unchanged) and bound the children of the others; stop when nothing is left.  Yaw and z are
 *       enumerated, not bounded.  opt = NULL or batch = 0: the default; batch 1 .. 65536.  stats (optional): what the search did.
 *       n_edges = 0 or a map without points: index 0 and zero counts, nothing is searched.
 * Argument rules, the limit on n_edges, the threading rule, the read-only guarantee and the error codes are those of
 * liodom_map_search_pose; a grid above 2^31 - 1 candidates and a batch outside its range are LIODOM_ERR_INVALID_ARG with nothing
 * computed.  The first call allocates the block tables: per level used, 8 bytes x the power of two >= 2 x the map's points. */
typedef struct liodom_pose_search_bnb_t {
  int32_t batch;               /* nodes taken per round; 0: the default */
  int32_t reserved[7];
} liodom_pose_search_bnb_t;
typedef struct liodom_pose_search_stats_t {
  int64_t n_candidates, nodes_bounded, candidates_scored;
  int32_t rounds, levels_built;
  int32_t reserved[2];
} liodom_pose_search_stats_t;
void liodom_pose_search_bnb_default(liodom_pose_search_bnb_t* opt);
int liodom_map_bound_nodes(liodom_map_t* m, const float* edges_xyzi, int n_edges, const double* T_lo /*n x 12*/,
                           const double* t_hi /*n x 2*/, int n, int level, int radius /*0 | 1*/, int32_t* ub /*n x 2: ub_r, ub_0*/);
int liodom_map_search_pose_bnb(liodom_map_t* m, const float* edges_xyzi, int n_edges, const liodom_pose_search_t* s,
                               const liodom_pose_search_bnb_t* opt /*NULL: defaults*/, liodom_pose_search_result_t* out,
                               liodom_pose_search_stats_t* stats /*optional*/);

/* ---- registering a scan to the map in 6-DoF (no counterpart in the reference; DESIGN.md §3 "Registering a scan to the map").
 * The searches above return a grid cell: x, y, yaw as fine as their step, no roll, pitch or z of their own.
 * liodom_map_register_poses carries the seeded first scan of liodom_seed_stream on, for n start poses at once, without a handle
 * and without writing anything of the map.  Each row is independent:
 *   start     the quaternion is normalised in double and T made from it, as liodom_seed_stream does.
 *   local map getLocalMap(T_start, cells_xy, cells_z), fetched ONCE: content and order of liodom_map_get_local; it is not fetched
 *             again as the pose moves.
 *   pass p    from (q, t): the edges transformed by T(q, t) and rounded to float; per edge the exact 5 nearest points of the row's
 *             local map (float squared distance, ties to the lower index); a correspondence is valid iff there are 5, the fifth is
 *             closer than 1 m (squared distance < 1.0f) and the line gate passes; the line is through the two nearest.  Then one LM
 *             solve from (q, t) as a scan's solve (4 iterations, Huber 0.2, min_range / max_range in the range weight).
 *   ending    an empty local map: LIODOM_REG_NO_MAP; a pass with fewer than min_matches valid correspondences:
 *             LIODOM_REG_FEW_MATCHES; a solve with termination 5: LIODOM_REG_EVAL_FAILURE — in all three the returned pose is the
 *             pose before that pass.  A pass that moved the pose by |dt| <= stop_translation and |vec(q_new (x) conj(q_old))| <=
 *             stop_rotation ends the row as LIODOM_REG_CONVERGED; otherwise LIODOM_REG_MAX_PASSES after the last pass.
 *   result    pose; passes = solves whose result was taken; matches = valid correspondences of the last pass that searched;
 *             last_move_t / last_move_r = the two norms of the last taken pass (0 if none); local_points.  When the last pass's
 *             solve was taken (CONVERGED, MAX_PASSES): information, final_cost, sigma2, cov_flags as liodom_pose_cov_t defines
 *             them — H at the returned pose over that pass's correspondences —, n_residuals = matches and last_lm the solve's
 *             trace.  Otherwise information and sigma2 are NaN, n_residuals = 0 and final_cost = 0 with cov_flags
 *             LIODOM_COV_NO_SOLVE (NO_MAP, FEW_MATCHES; last_lm zero) or LIODOM_COV_EVAL_FAILURE (last_lm = the failed solve's).
 *   corr      (optional) [n][n_edges][2]: the last searching pass's (a, b) indices into the row's local map, -1 where the edge had
 *             no valid correspondence (all -1 for NO_MAP).  An edge with a non-finite coordinate has none.
 * Coordinates beyond +-2^20 m take no part (the map holds no cell there).  Nothing of the map is written: its exported state, its
 * status and its generation are the same before and after, on a detached map, a map readers are attached to and a map a mapper
 * writes — between steps, under the threading rule of liodom_map_export_state.  Equal calls return equal bytes; row i of a batch
 * returns the bytes a one-row call with pose i returns.  The workspace belongs to the map: allocated by the first call, regrown
 * when n x local_capacity grows, freed with the map.
 * LIODOM_ERR_INVALID_ARG, nothing written, workspace untouched: a null where one is required; n < 1 or n > 64; n_edges < 0 or above
 * max_update_points; a non-finite pose or | |q| - 1 | > 1e-6; reserved != 0, max_passes outside 1 .. 16, min_matches < 1, negative
 * extents, capacity or thresholds, ranges that are not 0 <= min < max.  LIODOM_ERR_CAPACITY: a row's local map is larger than
 * local_capacity — the full sizes are in out[i].local_points (as liodom_map_get_local_batch reports sizes) and nothing else is
 * written.  n_edges = 0 is valid: every row ends as FEW_MATCHES (NO_MAP on an empty local map) with its start pose. */
#define LIODOM_REG_CONVERGED 0
#define LIODOM_REG_MAX_PASSES 1
#define LIODOM_REG_FEW_MATCHES 2
#define LIODOM_REG_NO_MAP 3
#define LIODOM_REG_EVAL_FAILURE 4
typedef struct liodom_map_register_t {
  int32_t cells_xy, cells_z;       /* getLocalMap extents around each start pose (defaults 2, 1) */
  int32_t max_passes;              /* 1 .. 16 correspondence passes (default 10) */
  int32_t min_matches;             /* a pass with fewer valid correspondences ends the row (default 6) */
  int32_t local_capacity;          /* points of one row's local map the workspace holds (0 = 65536) */
  int32_t reserved;                /* must be 0 */
  double  stop_translation;        /* [m]   a pass that moved the pose by <= both of these ends the row as converged (default 1e-4) */
  double  stop_rotation;           /* half-angle, as the solver's tangent (default 1e-5) */
  double  min_range, max_range;    /* the residual's range weight (defaults 3, 75) */
} liodom_map_register_t;           /* 56 bytes */
typedef struct liodom_map_registration_t {
  double  pose[7];                 /* [qx qy qz qw tx ty tz] */
  double  information[36];         /* H = sum rho' J^T J at `pose`, the tangent and order of liodom_pose_cov_t */
  double  final_cost, sigma2;      /* as liodom_pose_cov_t defines them */
  double  last_move_t, last_move_r;
  int32_t termination;             /* LIODOM_REG_* */
  int32_t passes, matches, n_residuals, local_points;
  uint32_t cov_flags;              /* LIODOM_COV_* of the final evaluation */
  liodom_lm_trace_t last_lm;
} liodom_map_registration_t;       /* 432 bytes */
void liodom_map_register_default(liodom_map_register_t* o);
int liodom_map_register_poses(liodom_map_t* m, const float* edges_xyzi, int n_edges, const double* poses /*n x 7*/, int n,
                              const liodom_map_register_t* opt /*NULL: defaults*/, liodom_map_registration_t* out /*[n]*/,
                              int32_t* corr /*optional, [n][n_edges][2]*/);

/* ---- finding the place: a database of binary polar descriptors (no counterpart in the reference; DESIGN.md §3 "Finding the
 * place", INTEGRATION.md §7 "Relocalising without a guess").  Every search above needs a pose to search around; a liodom_places_t
 * answers "near which key frame was this scan taken?" without one.  It is an object of its own: it touches no handle and no map,
 * has a HIP stream and a mutex of its own, and every call synchronises that stream before it returns.
 *
 * A place is one descriptor of a key frame's edge cloud IN THE SENSOR FRAME, plus the pose the key frame was taken at and a caller
 * tag.  The descriptor has W = n_rings * n_layers 64-bit words, 1 <= W <= 64; bit `sector` of word ring * n_layers + layer is set
 * iff a point of the cloud falls into that bin.  There are always 64 sectors: a sector is a bit and a yaw shift is a rotate.
 * All arithmetic is float32, no fused multiply-add.  Tables, made in double and rounded to float once (they travel in the blob):
 *   C_i, S_i = float(cos(i pi / 32)), float(sin(i pi / 32)), i = 1 .. 15;  R2_i = float((i r_max / n_rings)^2), i = 1 .. n_rings;
 *   Z_i = float(z_min + i (z_max - z_min) / n_layers), i = 0 .. n_layers.
 * A point (x, y, z) with a non-finite coordinate sets nothing.  j = #{i : |y| C_i >= |x| S_i}; the sector is j for x >= 0, y >= 0;
 * 31 - j for x < 0, y >= 0; 32 + j for x < 0, y < 0; 63 - j for x >= 0, y < 0 (-0 is not below 0).  r2 = x x + y y (two
 * multiplies, one add); ring = #{i : r2 >= R2_i}, and ring == n_rings sets nothing.  z < Z_0 sets nothing; layer = #{i >= 1 :
 * z >= Z_i}, and layer == n_layers sets nothing.
 * Distance of a query q and a place k: d(s) = sum over the words of popcount(rotl64(q[w], s) ^ k[w]), s = 0 .. 63; the place's
 * distance is the smallest d(s), its shift the lowest such s.  Places rank by (distance, index), lowest first.  The pose of a match
 * is place_pose o Rz(shift * 2 pi / 64), composed in double, the place's quaternion normalised as liodom_seed_stream does: a
 * query taken at the place's position with its heading turned by +a about z matches at shift = a / (2 pi / 64).
 * The descriptor has no roll or pitch term and no height term: it assumes a sensor that is level to within what a vehicle does
 * and mounted at the height the key frames were taken with.
 *
 *   liodom_place_geometry_default   16 rings, 4 layers, r_max 80 m, z from -4 to 12 m.
 *   liodom_places_create      max_places 1 .. 2^20, max_edges 1 .. 2^24 (points of one cloud); on the calling thread's current device.
 *   liodom_places_describe    desc_out[i * W ..] = the descriptor of row i (the cloud at edges_xyzi + 4 * i * edge_stride_points floats,
 *       n_edges[i] points), bits_out[i] (optional) = its popcount.
 *   liodom_places_add         describes one cloud and appends it with its pose [qx qy qz qw tx ty tz] and tag; *index (optional) =
 *       its index.  A full database: LIODOM_ERR_CAPACITY, database untouched.
 *   liodom_places_query       describes n rows and writes the k best places of each to out[i * k ..], best first; rows beyond the
 *       number of places have index -1 and every other field 0.  bits_query[i] (optional) = popcount of row i's descriptor.
 *   liodom_places_query_desc  the same for n descriptors the caller holds (n x W words).
 *   liodom_places_state_size / _export_state / _import_state   the database as one blob (layout: liodom_amd/csrc/
 *       place_state_format.h): magic "LIODOMPL", version, the geometry and its tables, then per place descriptor, bit count, tag and
 *       pose.  Export with cap too small: LIODOM_ERR_CAPACITY, *bytes = the size needed, nothing written.  Import validates on the
 *       host before anything is launched: truncation, bad magic / version, W outside 1 .. 64, sizes that do not add up, tables
 *       that are not the geometry's, a bit count that is not its descriptor's popcount, a pose liodom_places_add would refuse, or a
 *       geometry that differs in any bit from the database's: LIODOM_ERR_INVALID_ARG; more places than max_places:
 *       LIODOM_ERR_CAPACITY.  On any error the database is untouched.
 *   liodom_places_reset       no places; capacities and allocations are kept.
 * Limits: 1 <= k <= 16, n <= 2^20.  LIODOM_ERR_INVALID_ARG, with nothing computed: a null where one is required, a negative count
 * or stride, k out of range, n_edges[i] > edge_stride_points or > max_edges, a non-finite pose or | |q| - 1 | > 1e-6.
 * Non-finite edges are no error.  n = 0, or a database without places: LIODOM_OK (index -1 rows). */
typedef struct liodom_places liodom_places_t;
typedef struct liodom_place_geometry_t {
  int32_t n_rings, n_layers;
  double r_max, z_min, z_max;
  int64_t reserved;
} liodom_place_geometry_t;     /* 40 bytes */
typedef struct liodom_place_match_t {
  int32_t index;               /* of the place, -1: none */
  int32_t distance, shift;     /* Hamming distance at the best yaw shift; the lowest such shift, 0 .. 63 */
  int32_t bits_place;          /* popcount of the place's descriptor */
  int64_t id;                  /* the place's tag */
  double pose[7];              /* place_pose o Rz(shift * 2 pi / 64): what liodom_seed_stream or a search centre takes */
  double place_pose[7];        /* as given to liodom_places_add */
} liodom_place_match_t;        /* 136 bytes */
void liodom_place_geometry_default(liodom_place_geometry_t* g);
int liodom_places_create(const liodom_place_geometry_t* geom, int max_places, int max_edges, liodom_places_t** out);
void liodom_places_destroy(liodom_places_t* db);
int liodom_places_count(liodom_places_t* db, int32_t* count);
int liodom_places_reset(liodom_places_t* db);
int liodom_places_describe(liodom_places_t* db, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges /*[n]*/, int n,
                           uint64_t* desc_out /*n x W*/, int32_t* bits_out /*optional, [n]*/);
int liodom_places_add(liodom_places_t* db, const float* edges_xyzi, int n_edges, const double* pose /*[7]*/, int64_t id,
                      int32_t* index /*optional*/);
int liodom_places_query(liodom_places_t* db, const float* edges_xyzi, int64_t edge_stride_points, const int32_t* n_edges /*[n]*/, int n,
                        int k, liodom_place_match_t* out /*n x k*/, int32_t* bits_query /*optional, [n]*/);
int liodom_places_query_desc(liodom_places_t* db, const uint64_t* desc /*n x W*/, int n, int k, liodom_place_match_t* out /*n x k*/);
int liodom_places_state_size(liodom_places_t* db, int64_t* bytes);
int liodom_places_export_state(liodom_places_t* db, void* blob, int64_t cap, int64_t* bytes);
int liodom_places_import_state(liodom_places_t* db, const void* blob, int64_t bytes);

/* ---- closing loops: a pose graph over key frames, optimised on the device (no counterpart in the reference; DESIGN.md §3
 * "Closing loops", INTEGRATION.md §7 "Correcting a revisit").  A liodom_graph_t is an object of its own: it touches no handle and
 * no map, has a HIP stream and a mutex of its own, and every call synchronises that stream before it returns.
 *
 * A node is a pose X = (q, t), world <- frame, [qx qy qz qw tx ty tz]; it is free or fixed.  An edge (i, j, Z, Omega) says
 * "X_i^-1 o X_j was measured as Z, with information Omega (6 x 6, row-major)".  Its error: D = Z^-1 o X_i^-1 o X_j = (q_d, t_d),
 * e = [s vec(q_d); t_d], s = +1 for w_d >= 0, else -1 (the rotation part is the half angle: the rotation angle is 2 |vec|, as in
 * liodom_pose_cov_t).  The cost is chi2 = sum over the edges of e^T Omega e.  A node moves by delta = (d, dt):
 * q <- [sin|d| d/|d|, cos|d|] (x) q (left multiplication, world frame), t <- t + dt — the parameterisation of the scan solver.
 * With J the exact derivative of the stacked e by the stacked delta at 0: gradient g = J^T Omega e, H = J^T Omega J, and one
 * Levenberg-Marquardt step solves (H + lambda diag H) delta = -g by preconditioned conjugate gradients (6 x 6 blocks in the
 * coordinates of the chain of edges (n - 1, n), block-Jacobi where there is none: DESIGN.md §3 "Closing loops").  A fixed
 * node has delta = 0: its rows and columns drop out.  A free node without edges stays where it is (its block counts as the
 * identity).  All arithmetic is double; sums run in an order that depends on the graph alone (no atomics), so equal graphs give
 * equal bytes.  Quaternions are divided by their norm when they are taken in.
 *
 *   liodom_graph_create       1 <= max_nodes <= 65 536, 1 <= max_edges <= 262 144; on the calling thread's current device.  Device
 *       memory is taken here, about 1.3 KiB per edge and 1 KiB per node of capacity.  The solve is one launch of one workgroup
 *       per step, and nothing but max_pcg_iterations bounds how long it runs: about 60 us per iteration up to 1 024 nodes,
 *       1.5 ms at 16 384 (MI355X), so a step of a graph of that size can take seconds and one at full capacity minutes.
 *   liodom_graph_reset        no nodes, no edges; capacities and allocations are kept, and so is the table of losses
 *       (liodom_graph_set_loss): it is a setting of the graph, like its capacities.
 *   liodom_graph_count        *n_nodes, *n_edges (either optional).
 *   liodom_graph_add_nodes    appends n poses (n x 7); fixed[k] != 0 (optional, NULL: all free) fixes node k.  *first (optional) =
 *       the index of the first one; indices count up from 0 in the order of adding.
 *   liodom_graph_add_edges    appends n edge records.  kind is the caller's (0 odometry, 1 loop by convention; it selects the
 *       edge's loss, see "robust losses" below, and nothing else reads it); reserved must be 0.  An edge is active when added.
 *   liodom_graph_set_fixed / _get_poses / _set_poses   nodes first .. first + n - 1.
 *   liodom_graph_get_edges    edges first .. first + n - 1, as stored (Z's quaternion normalised), inactive ones too.
 *   liodom_graph_linearize    at the current poses: chi2_per_edge[n_edges], gradient[6 n_nodes] (0 for fixed nodes),
 *       diag[n_nodes x 36] (each node's 6 x 6 block of H, row-major; also for fixed nodes).  Every output is optional.
 *   liodom_graph_multiply     y = (H + lambda diag H) x at the current poses, x and y 6 n_nodes each; rows of fixed nodes are 0
 *       and their x is not read; a free node without edges: y = x.
 *   liodom_graph_options_default   max_iterations 20, max_pcg_iterations 0 (= 6 x free nodes, at most 65 536), pcg_tolerance 1e-8
 *       (on |r| / |g|), gradient_tolerance 1e-9 (on max |g|), cost_tolerance 1e-10 (on the relative decrease of chi2).
 *   liodom_graph_optimize     Levenberg-Marquardt from lambda = 1e-4.  A step is accepted iff chi2 decreases: lambda <-
 *       max(lambda / 10, 1e-12); otherwise lambda <- 10 lambda and the poses stay.  Ends (report->termination) with max |g| <=
 *       gradient_tolerance, a relative decrease of an accepted step <= cost_tolerance, after max_iterations steps tried, with
 *       lambda > 1e12, or with a breakdown of the conjugate gradients (p^T H p <= 0, or a diagonal block that is not positive
 *       definite: an information matrix that is not).  The poses are those of the last accepted step.  opt NULL: the defaults;
 *       report optional.  A graph without a fixed node: LIODOM_ERR_INVALID_ARG.  A graph without a free node or without an edge
 *       returns at once (LIODOM_GRAPH_TERM_GRADIENT, 0 iterations).
 *
 * Robust losses and switched-off edges (all opt-in: a graph on which none of these calls is made computes what it did before
 * they existed, byte for byte).  With s = e^T Omega e of an edge, a loss rho with scale c > 0 replaces s in the cost, and
 * w = rho'(s) weights the edge in g and H (first-order IRLS: no second-order term).  Every rho is concave in s, so the weighted
 * quadratic lies above the cost and touches it at the current poses: a large enough lambda always finds a decrease, and the
 * accept / reject rule of liodom_graph_optimize stays sound.
 *     LIODOM_GRAPH_LOSS_NONE 0            rho = s                                       w = 1
 *     LIODOM_GRAPH_LOSS_HUBER 1           rho = s if s <= c^2, else 2 c sqrt(s) - c^2   w = 1 if s <= c^2, else c / sqrt(s)
 *     LIODOM_GRAPH_LOSS_CAUCHY 2          rho = c^2 log1p(s / c^2)                      w = 1 / (1 + s / c^2)
 *     LIODOM_GRAPH_LOSS_GEMAN_MCCLURE 3   rho = s c^2 / (c^2 + s)                       w = (c^2 / (c^2 + s))^2
 * c is in units of sqrt(chi2): it must exceed what honest drift produces on a true edge, or a true edge is down-weighted with
 * the false ones (DESIGN.md §3 "Closing loops" has a designed graph on which Geman-McClure with c = 3 rejects every true loop).
 *   liodom_graph_set_loss / _get_loss   the graph keeps a table of (loss, scale) over kind 0 .. 15, all NONE at first; an edge
 *       whose kind is outside 0 .. 15 is always quadratic.  The scale is not read for NONE (it is then stored and returned as
 *       0).  _get_loss: either output optional.  liodom_graph_reset keeps the table.
 *   liodom_graph_set_edge_active / _get_edge_active   edges first .. first + n - 1, active[k] != 0: active.  An inactive edge
 *       gives nothing to the cost, g, H, a node's degree or the preconditioner's chain: a free node whose edges are all inactive
 *       is a node without edges (identity block, it stays where it is), and a node hangs on an edge (n - 1, n) only if that edge
 *       is active.
 *   liodom_graph_edge_weights   rho[n_edges] and weight[n_edges] at the current poses, either optional; both 0 for an inactive edge.
 *   liodom_graph_linearize    chi2_per_edge stays the raw s, for inactive edges too; gradient and diag are the weighted ones.
 *   liodom_graph_multiply     uses the weighted blocks.
 *   liodom_graph_optimize     the cost is the sum of rho over the active edges — in the accept test, initial_cost, final_cost
 *       and cost_tolerance —, max_gradient is that of the weighted g, and "without an edge" above reads "without an active edge".
 * Sums stay in an order that depends on the graph alone: equal graphs with equal settings give equal bytes.
 * LIODOM_ERR_INVALID_ARG, graph untouched: a null where one is required, a negative count, a range beyond the nodes or edges, a
 * non-finite pose or Z, | |q| - 1 | > 1e-6, an edge with i == j or an index that is no node, reserved != 0, an Omega with a
 * non-finite entry or one that is not symmetric bit for bit, options out of range (a negative count or tolerance, or a NaN),
 * a loss kind outside 0 .. 15, an unknown loss, a scale that is not finite and > 0 (with a loss other than NONE).
 * LIODOM_ERR_CAPACITY, graph untouched: more nodes than max_nodes or more edges than max_edges. */
typedef struct liodom_graph liodom_graph_t;
typedef struct liodom_graph_edge_t {
  int32_t i, j, kind, reserved;
  double z[7];
  double info[36];
} liodom_graph_edge_t;         /* 360 bytes */
typedef struct liodom_graph_options_t {
  int32_t max_iterations, max_pcg_iterations;
  double pcg_tolerance, gradient_tolerance, cost_tolerance;
} liodom_graph_options_t;      /* 32 bytes */
#define LIODOM_GRAPH_TERM_GRADIENT 0
#define LIODOM_GRAPH_TERM_COST 1
#define LIODOM_GRAPH_TERM_MAX_ITERATIONS 2
#define LIODOM_GRAPH_TERM_LAMBDA 3
#define LIODOM_GRAPH_TERM_BREAKDOWN 4
#define LIODOM_GRAPH_LOSS_NONE 0
#define LIODOM_GRAPH_LOSS_HUBER 1
#define LIODOM_GRAPH_LOSS_CAUCHY 2
#define LIODOM_GRAPH_LOSS_GEMAN_MCCLURE 3
typedef struct liodom_graph_report_t {
  double initial_cost, final_cost;   /* chi2 (with a loss: the sum of rho) at the poses the call found and at those it left */
  double max_gradient;               /* max |g| at the poses it left */
  double final_lambda;
  int32_t iterations;                /* steps tried */
  int32_t accepted_steps;
  int32_t pcg_iterations;            /* over all steps */
  int32_t termination;               /* LIODOM_GRAPH_TERM_* */
} liodom_graph_report_t;       /* 48 bytes */
int liodom_graph_create(int max_nodes, int max_edges, liodom_graph_t** out);
void liodom_graph_destroy(liodom_graph_t* g);
int liodom_graph_reset(liodom_graph_t* g);
int liodom_graph_count(liodom_graph_t* g, int32_t* n_nodes, int32_t* n_edges);
int liodom_graph_add_nodes(liodom_graph_t* g, const double* poses /*n x 7*/, const int32_t* fixed /*optional, [n]*/, int n,
                           int32_t* first /*optional*/);
int liodom_graph_add_edges(liodom_graph_t* g, const liodom_graph_edge_t* edges, int n);
int liodom_graph_set_fixed(liodom_graph_t* g, int first, int n, const int32_t* fixed);
int liodom_graph_get_poses(liodom_graph_t* g, int first, int n, double* poses /*n x 7*/);
int liodom_graph_set_poses(liodom_graph_t* g, int first, int n, const double* poses /*n x 7*/);
int liodom_graph_get_edges(liodom_graph_t* g, int first, int n, liodom_graph_edge_t* edges);
int liodom_graph_linearize(liodom_graph_t* g, double* chi2_per_edge, double* gradient, double* diag);
int liodom_graph_multiply(liodom_graph_t* g, double lambda, const double* x, double* y);
void liodom_graph_options_default(liodom_graph_options_t* opt);
int liodom_graph_optimize(liodom_graph_t* g, const liodom_graph_options_t* opt, liodom_graph_report_t* report);
int liodom_graph_set_loss(liodom_graph_t* g, int kind, int loss, double scale);
int liodom_graph_get_loss(liodom_graph_t* g, int kind, int32_t* loss /*optional*/, double* scale /*optional*/);
int liodom_graph_set_edge_active(liodom_graph_t* g, int first, int n, const int32_t* active);
int liodom_graph_get_edge_active(liodom_graph_t* g, int first, int n, int32_t* active);
int liodom_graph_edge_weights(liodom_graph_t* g, double* rho /*optional, [n_edges]*/, double* weight /*optional, [n_edges]*/);

/* ---- covariances of the graph and the loop gate (DESIGN.md §3 "Covariances of the graph and the loop gate").
 * All opt-in: a graph on which none of these calls is made computes what it did before they existed.  None of them changes poses,
 * edges or settings.
 *
 * H is the matrix liodom_graph_multiply(g, 0, ...) applies at the current poses: over the active edges, weighted where a robust
 * loss is set, rows and columns of fixed nodes dropped.  Sigma = H^-1 in the coordinates of delta — half-angle rotation first,
 * then translation, world frame: those of liodom_pose_cov_t.  Sigma[r, c] is the 6 x 6 block of nodes r and c, row-major.  A
 * column of Sigma is solved by preconditioned conjugate gradients, one workgroup per column, until |e_c - H x| <= pcg_tolerance
 * (by the solver's own recurrence) or max_pcg_iterations.
 *   liodom_graph_cov_options_default   max_pcg_iterations 0 (= 6 x free nodes, at most 65 536), batch_columns 0 (columns per
 *       launch; 0: as many as fit 256 MiB of workspace, at least 6), pcg_tolerance 1e-8.  opt NULL in a call: these.
 *   liodom_graph_solve_columns   x[k] (6 columns of 6 n_nodes doubles each, column b of node nodes[k] at x + (6 k + b) 6 n_nodes)
 *       and status[6 k + b] with the iterations, the LIODOM_GRAPH_COV_* status and the recurrence's |r| of that column.
 *   liodom_graph_covariance      blocks[k] = Sigma[rows[k], cols[k]] (36 doubles) and status[k].
 *   liodom_graph_gate_edges      for each candidate edge (i, j, Z, Omega; validated exactly as liodom_graph_add_edges validates,
 *       kind ignored): d2 = e^T S^-1 e, S = [A B] [[Sigma ii, Sigma ij], [Sigma ij^T, Sigma jj]] [A B]^T + Omega^-1 with e, A, B
 *       the edge's error and Jacobians at the current poses — the squared Mahalanobis distance between the measured Z and the
 *       relative pose the graph predicts; chi-square with 6 degrees of freedom if the graph's information matrices are honest.
 *   liodom_graph_cov_counters    how many column launches these calls have made on g and how many columns those solved, since
 *       liodom_graph_create (either optional).
 * Statuses — a block takes the worst of its six columns, a gate the worst of its two nodes' columns; the numbers ascend:
 *     LIODOM_GRAPH_COV_OK 0              solved                                             the block or d2
 *     LIODOM_GRAPH_COV_NOT_CONVERGED 1   the iterations ran out                             the last iterate
 *     LIODOM_GRAPH_COV_BREAKDOWN 2       the solve broke down (H not positive definite)     NaN
 *     LIODOM_GRAPH_COV_UNANCHORED 3      the node's connected component over the active edges holds no fixed node: it has no
 *                                        finite covariance; no solve is launched for it    NaN
 *     LIODOM_GRAPH_COV_NOT_PD 4          Omega of the candidate or S is not positive definite (gate only)   NaN
 * A fixed node gives zero columns and zero blocks, status OK, whatever the other node is.  Equal graphs, settings and queries give equal bytes,
 * whatever batch_columns is.  LIODOM_ERR_INVALID_ARG, graph untouched, as above; also an option that is negative or a NaN. */
typedef struct liodom_graph_cov_options_t {
  int32_t max_pcg_iterations, batch_columns;
  double pcg_tolerance;
} liodom_graph_cov_options_t;  /* 16 bytes */
#define LIODOM_GRAPH_COV_OK 0
#define LIODOM_GRAPH_COV_NOT_CONVERGED 1
#define LIODOM_GRAPH_COV_BREAKDOWN 2
#define LIODOM_GRAPH_COV_UNANCHORED 3
#define LIODOM_GRAPH_COV_NOT_PD 4
typedef struct liodom_graph_cov_status_t {
  int32_t iterations, status;
  double residual;
} liodom_graph_cov_status_t;   /* 16 bytes */
void liodom_graph_cov_options_default(liodom_graph_cov_options_t* opt);
int liodom_graph_solve_columns(liodom_graph_t* g, const int32_t* nodes, int n, const liodom_graph_cov_options_t* opt,
                               double* x /*n x 6 x 6 n_nodes*/, liodom_graph_cov_status_t* status /*n x 6*/);
int liodom_graph_covariance(liodom_graph_t* g, const int32_t* rows, const int32_t* cols, int n, const liodom_graph_cov_options_t* opt,
                            double* blocks /*n x 36*/, int32_t* status /*n*/);
int liodom_graph_gate_edges(liodom_graph_t* g, const liodom_graph_edge_t* candidates, int n, const liodom_graph_cov_options_t* opt,
                            double* d2 /*n*/, int32_t* status /*n*/);
int liodom_graph_cov_counters(liodom_graph_t* g, int64_t* launches /*optional*/, int64_t* columns /*optional*/);

/* ---- odometry edges from the scans' own covariances (DESIGN.md §3 "Odometry edges from the scans' covariances", INTEGRATION.md
 * §7).  Opt-in: a handle that never makes these calls allocates and launches what it did before they existed.
 *
 * For an interval (a, b), a < b, of a stream's scans — X_k = (q_k, t_k) the pose of scan k, its quaternion divided by its norm
 * when taken in, C_k the `covariance` of scan k's liodom_pose_cov_t in its tangent (d, dt) — the calls give the edge
 * "X_a^-1 o X_b was measured as Z with information Omega" in the form liodom_graph_add_edges takes:
 *   Z        q_z = conj(q_a) (x) q_b, t_z = R_a^T (t_b - t_a).
 *   usable   scan k is usable iff its record has scan_index == k, flags == LIODOM_COV_VALID exactly and 36 finite covariance
 *            entries (the lower triangle of C_k is what is read; sigma2 H^-1 is symmetric bit for bit).
 *   Sigma    the sum over the usable k = a + 1 .. b of M_k = T_k (inflation C_k + F) T_k^T, T_k = [[I, 0], [-2 [u_k]x, I]],
 *            u_k = t_b - t_k, F = diag(fr^2 x 3, ft^2 x 3): the error of scan k's solve is a world-frame tangent perturbation of X_k
 *            that every later pose rides on rigidly (d_b = d, dt_b = dt - 2 [u_k]x d), and the scans' errors are taken as
 *            independent — an approximation: a solve registers against a window of earlier scans; `inflation` is where a
 *            calibration puts what that costs.  Summation order, a function of (a, b) alone: lane l of 64 sums
 *            its scans k = l (mod 64) in ascending order from 0; the 64 partials v are combined as P1[r] = v[r] + v[r + 32]
 *            (r < 32), P2[r] = P1[r] + P1[r + 16], P3[r] = P2[r] + P2[15 - r], P4[r] = P3[r] + P3[7 - r], P5[r] = P4[r] + P4[r + 2],
 *            Sigma = P5[0] + P5[1].  Equal inputs give equal bytes.
 *   Omega    B = de/d(delta_j) of the edge's error at (X_a, X_b, Z); Sigma_e = B Sigma B^T (`covariance`), Omega = Sigma_e^-1 by
 *            Cholesky (`information`), both symmetric bit for bit.  Omega does not depend on the frame the poses are given in.
 * All arithmetic is double, no contraction.
 *
 *   liodom_odom_edge_options_default   inflation 1, floor_rotation 0 (fr, half-angle radians), floor_translation 0 (ft, metres):
 *       the raw records.  opt NULL in a call: these.  A non-finite or negative value, inflation 0 or reserved != 0:
 *       LIODOM_ERR_INVALID_ARG.
 *   liodom_chain_odometry_edges   the public form: host arrays poses[m x 7] and records[m], entry k is scan k; n intervals
 *       0 <= from[i] < to[i] < m, n <= 2^20 (else LIODOM_ERR_INVALID_ARG, nothing written; n = 0: LIODOM_OK).  Needs no handle: it runs on the
 *       calling thread's current device, with buffers of its own for the duration of the call.
 *   liodom_get_odometry_edges     the same kernel on the stream's own pose log and covariance log, in place on the device.
 *       It takes the locks and synchronises as liodom_get_pose_covariance_log does.  pose_covariance = 0: LIODOM_ERR_UNSUPPORTED.
 *       An interval must satisfy first <= from < to < min(scans enqueued, pose_log_capacity), first = the stream's scan count at
 *       its last liodom_reset, liodom_reset_stream, liodom_seed_stream or liodom_import_stream_state (0 after liodom_create): the
 *       log below it belongs to an earlier life of the stream.  Else LIODOM_ERR_INVALID_ARG, nothing written.
 * Flags of a record:
 *     LIODOM_ODOM_EDGE_VALID 1     Z and Omega are defined
 *     LIODOM_ODOM_EDGE_GAPS 2      n_missing > 0: unusable scans contributed nothing — the caller decides what to do
 *     LIODOM_ODOM_EDGE_NOT_PD 4    n_used == 0, Cholesky failed or Omega is not finite: covariance and information NaN, Z valid
 *     LIODOM_ODOM_EDGE_NO_POSE 8   a non-finite pose at a, at b or in between (or a zero quaternion at a or b): z, covariance and
 *                                  information NaN; no other flag is set */
typedef struct liodom_odom_edge_t {
  int32_t scan_from, scan_to;
  uint32_t flags;              /* LIODOM_ODOM_EDGE_* */
  int32_t n_used, n_missing;   /* usable / unusable scans among from + 1 .. to */
  int32_t reserved;            /* 0 */
  double z[7];
  double covariance[36];       /* Sigma_e, row-major */
  double information[36];      /* Omega, row-major */
} liodom_odom_edge_t;          /* 656 bytes */
#define LIODOM_ODOM_EDGE_VALID 1u
#define LIODOM_ODOM_EDGE_GAPS 2u
#define LIODOM_ODOM_EDGE_NOT_PD 4u
#define LIODOM_ODOM_EDGE_NO_POSE 8u
#define LIODOM_ODOM_EDGES_MAX (1 << 20)
typedef struct liodom_odom_edge_options_t {
  double inflation, floor_rotation, floor_translation;
  int32_t reserved[4];         /* 0 */
} liodom_odom_edge_options_t;  /* 40 bytes */
void liodom_odom_edge_options_default(liodom_odom_edge_options_t* opt);
int liodom_chain_odometry_edges(const double* poses /*m x 7*/, const liodom_pose_cov_t* records /*m*/, int m, const int32_t* from,
                                const int32_t* to, int n, const liodom_odom_edge_options_t* opt, liodom_odom_edge_t* out /*n*/);
int liodom_get_odometry_edges(liodom_handle_t* h, int stream, const int32_t* from, const int32_t* to, int n,
                              const liodom_odom_edge_options_t* opt, liodom_odom_edge_t* out /*n*/);

#ifdef __cplusplus
}
#endif
#endif /* LIODOM_HIP_H */
