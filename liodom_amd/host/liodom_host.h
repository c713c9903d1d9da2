// liodom_host.h — host-side C++ mirror of the reference's hot-path classes, implemented over the
// C-ABI of include/liodom_hip.h (no ROS, no PCL, no Eigen, no Ceres).
//
// Names, argument meaning and error behaviour follow the reference so that a maintainer can swap
// the bodies of the corresponding reference classes:
//   liodom::Params            include/liodom/params.h:30-70, src/params.cc:37-110
//   liodom::FeatureExtractor  include/liodom/feature_extractor.h:62-85, src/feature_extractor.cc
//   liodom::LaserOdometer     include/liodom/laser_odometry.h:79-121, src/laser_odometry.cc
//   liodom::LocalMapManager   include/liodom/laser_odometry.h:62-76 (read-only view of the device window)
//   liodom::Stats             include/liodom/stats.h:40-80, src/stats.cc (result files)
//   liodom::Map               include/liodom/map.h:93-116, src/map.cc (mapping node's map, on the device)
//   liodom::SharedData        include/liodom/shared_data.h:40-86, src/shared_data.cc (the two hand-over queues)
// Like the reference the hot-path methods return void and report problems through a log hook;
// unlike it, failures of the GPU library also raise std::runtime_error (nothing falls back to CPU).
#pragma once
#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <vector>

#include "../../include/liodom_hip.h"

namespace liodom {

typedef std::chrono::high_resolution_clock Clock;   // include/liodom/defs.h:38

// pcl::PointXYZI without padding: the packed float4 the C-ABI takes.
struct Point { float x, y, z, intensity; };
struct PointCloud {
  std::vector<Point> points;
  uint32_t width = 0, height = 1;     // organised clouds: height rows x width columns (row-major)
  size_t size() const { return points.size(); }
};

// Pose as the reference publishes it (world <- laser): quaternion [x y z w] + translation.
struct Pose { double q[4] = {0, 0, 0, 1}; double t[3] = {0, 0, 0}; std::array<double, 12> matrix34() const; };

// Same public fields as liodom::Params (include/liodom/params.h:33-49).
class Params {
 public:
  double min_range_ = 3.0;
  double max_range_ = 75.0;
  int lidar_type_ = 0;
  int scan_lines_ = 64;
  int scan_regions_ = 8;
  int edges_per_region_ = 10;
  size_t min_points_per_scan_ = 90;
  size_t local_map_size_ = 5;
  bool save_results_ = false;
  std::string results_dir_ = "~/";
  std::string fixed_frame_ = "odom";
  std::string base_frame_ = "base_link";
  std::string laser_frame_ = "";
  bool use_imu_ = false;
  bool filter_local_map_ = false;
  bool mapping_ = false;
  bool publish_tf_ = true;

  static Params* getInstance();
  // readParams(nh) of the reference reads ROS parameters; here the same names come from
  // "name=value" strings (launch-file values), unknown names are ignored like nh.param would.
  void readParams(const std::vector<std::string>& name_value_pairs);
  liodom_params_t toC() const;
};

class Stats {
 public:
  static Stats* getInstance();
  void addPose(const std::array<double, 12>& pose34);                                          // stats.cc:36
  void addFeatureExtractionTime(const Clock::time_point& start, const Clock::time_point& end);  // :40
  void addLaserOdometryTime(const Clock::time_point& start, const Clock::time_point& end);      // :45
  void addNumOfFeats(const size_t& nfeats);                                                     // :50
  void startFrame(const Clock::time_point& start);                                              // :54
  void stopFrame(const Clock::time_point& stop);                                                // :60
  void writeResults(const std::string& dir);                                                    // :73-132
  void clear();
  // takes the last fused scan's entries back (pose, odometry time, frame time, feature count): a scan that is processed again after
  // a relocalisation keeps one row in the result files
  void dropLastScan();
  size_t numPoses();
 private:
  std::vector<std::array<double, 12>> poses_;
  std::atomic<size_t> n_poses_{0};
  std::vector<double> feat_extr_, laser_odom_, frame_times_;
  std::vector<size_t> num_of_features_;
  std::mutex frame_mutex_;
  std::queue<Clock::time_point> start_times_;
};

// The mutex-guarded FIFOs between the ROS callback, the extractor thread and the odometer thread
// (src/shared_data.cc:37-89).  Headers carry only the stamp here.
// One element of the feature queue: the edge cloud as published on ~edges (host copy) and — with the device-resident
// hand-off — the ticket of the copy that stayed in HBM (liodom_extract_edges_device); ticket.seq == 0: host cloud only.
struct Features {
  PointCloud edges;
  double stamp = 0;
  liodom_edge_ticket_t ticket{0, 0, 0, 0};
};
class SharedData {
 public:
  static SharedData* getInstance();
  void pushPointCloud(const PointCloud& pc_in, double stamp);          // shared_data.cc:37-42
  bool popPointCloud(PointCloud& pc_out, double& stamp);               // :44-62
  void pushFeatures(const PointCloud& feat_in, double stamp);          // :64-69
  bool popFeatures(PointCloud& feat_out, double& stamp);               // :71-89
  void pushFeatures(Features&& f);                                     // the same with the device ticket
  bool popFeatures(Features& f);
  size_t numFeatures();
  void clear();
  // Poll interval of the two worker loops in microseconds (the reference sleeps 2 ms, feature_extractor.cc:80 /
  // laser_odometry.cc:270; 0 = yield only: throughput measurements)
  std::atomic<int> poll_us{2000};
 private:
  std::mutex pc_mutex_, feat_mutex_;
  std::queue<std::pair<PointCloud, double>> pc_buf_;
  std::queue<Features> feat_buf_;
};

// A polar scan's geometry (liodom_polar_geometry_t) with tables it owns: what a sensor driver keeps of the calibration.  A scan
// of it is one blob (std::vector<uint8_t> of blobBytes(), sections at layout()'s offsets) instead of a PointCloud: the driver's
// projection and pcl::fromROSMsg (liodom_node.cc:43-44) move onto the device.  No counterpart in the reference.
struct PolarGeometry {
  int height = 0, width = 0, range_bits = 16, intensity_bits = 8;
  float range_unit = 0.002f, beam_origin = 0.f;
  std::vector<float> cos_alt, sin_alt, cos_baz, sin_baz;     // [height]
  std::vector<float> cos_enc, sin_enc;                       // [ticks]
  // Tables from angles in radians (altitude and azimuth offset per row, azimuth per encoder tick): sines and cosines in double,
  // rounded to float once.
  static PolarGeometry fromAngles(int height, int width, const std::vector<double>& altitude, const std::vector<double>& beam_azimuth,
                                  const std::vector<double>& encoder, int range_bits = 16, int intensity_bits = 8,
                                  float range_unit = 0.002f, float beam_origin = 0.f);
  liodom_polar_geometry_t toC() const;                       // (points into this object)
  liodom_polar_layout_t layout() const;
  size_t blobBytes() const { return (size_t)layout().total_bytes; }
};

// Owns the GPU handle shared by the extractor and the odometer of one stream.
class Engine {
 public:
  // pose_rotation_mode: see liodom_config_t (1 = Eigen 3.3.x Transform::rotation(), the default)
  // pose_covariance: see liodom_config_t (1 = per-scan covariance records, OdometryMsg::pose_covariance)
  Engine(const Params& p, int device, int max_points, int max_width, int pose_rotation_mode = 1, int pose_covariance = 0);
  ~Engine();
  liodom_handle_t* handle() const { return h_; }
  int edge_capacity() const { return edge_cap_; }
  int rotation_mode() const { return rotation_mode_; }
  bool covariance() const { return covariance_; }
  // Streams with a life of their own (liodom_reset_stream / liodom_export_stream_state / liodom_import_stream_state; no
  // counterpart in the reference).  resetStream: the stream's next scan is its first.  saveState: the stream's odometry state as
  // one blob (layout: DESIGN.md §3).  loadState: puts such a blob — of any engine with the same parameters — into the stream.
  // liodom_set_polar_geometry: from here on the polar forms of FeatureExtractor / LaserOdometer take blobs of this geometry
  void setPolarGeometry(const PolarGeometry& g);
  int polarPoints() const { return polar_n_; }
  void resetStream(int stream = 0);
  std::vector<uint8_t> saveState(int stream = 0);
  void loadState(const std::vector<uint8_t>& blob, int stream = 0);
  // One lock-step step of resident slot `slot` for the streams in `streams` only (strictly ascending; liodom_process_resident_subset;
  // no counterpart in the reference): the other streams sit the step out.  Returns the listed streams' poses [x y z w tx ty tz]
  // in list order.  next_slot >= 0 issues that slot's extraction ahead for next_streams (null: the same list).
  std::vector<std::array<double, 7>> stepSubset(int slot, const std::vector<int32_t>& streams, int64_t n, int height, int width,
                                                int next_slot = -1, const std::vector<int32_t>* next_streams = nullptr);
  // The odometry edges of the intervals (scan_from[i], scan_to[i]) of a stream, Z and Omega chained on the device from the
  // stream's own pose log and covariance log (liodom_get_odometry_edges; pose_covariance = 1; no counterpart in the reference):
  // records in the form PoseGraph / liodom_graph_add_edges take z and information.  opt null: inflation 1, no floors.
  std::vector<liodom_odom_edge_t> odometryEdges(const std::vector<int32_t>& scan_from, const std::vector<int32_t>& scan_to,
                                                const liodom_odom_edge_options_t* opt = nullptr, int stream = 0);
 private:
  liodom_handle_t* h_ = nullptr;
  bool covariance_ = false;
  int edge_cap_ = 0;
  int rotation_mode_ = 1;
  int polar_n_ = 0;
};

class FeatureExtractor {
 public:
  explicit FeatureExtractor(std::shared_ptr<Engine> engine);
  // splitPointCloud + extractFeatures (feature_extractor.cc:104-254) for one cloud.
  void extractFeatures(const PointCloud& pc_in, PointCloud& pc_edges);
  // Polar forms (Engine::setPolarGeometry first).  projectPolar: the cloud the driver would have published (liodom_project_polar).
  // extractFeaturesPolar: one blob through liodom_extract_edges_device_polar + liodom_wait_edges — the ~edges cloud and the
  // ticket LaserOdometer::process takes; false when every hand-off slot is taken (keep the blob and retry).
  void projectPolar(const std::vector<uint8_t>& blob, PointCloud& pc_out);
  bool extractFeaturesPolar(const std::vector<uint8_t>& blob, double stamp, Features& f);
  // the edges of the last scan that went through LaserOdometer::processScan (the ~edges topic, :70-75)
  void lastEdges(PointCloud& pc_edges);
  // The worker loop of the extractor thread (feature_extractor.cc:42-82): pop a cloud, extract,
  // push the features; polls every 2 ms like the reference.  Runs on the extraction side of the
  // handle, concurrently with LaserOdometer::operator() (liodom_node.cc:89-91).
  void operator()(std::atomic<bool>& running);
  // Device-resident hand-off (default): the worker loop leaves every edge cloud on the device (liodom_extract_edges_device), takes
  // the host copy for ~edges from the extraction's host-mapped mirror (liodom_wait_edges) and queues the ticket with it.
  // false: liodom_extract_edges (host cloud out), as the first version of this binding did.
  void setDeviceHandoff(bool on) { device_handoff_ = on; }
 private:
  std::shared_ptr<Engine> eng_;
  Params* params;
  Stats* stats;
  bool device_handoff_ = true;
};

class LocalMapManager {
 public:
  explicit LocalMapManager(std::shared_ptr<Engine> engine) : eng_(std::move(engine)) {}
  // getLocalMap (laser_odometry.cc:62-65): window points oldest frame first; returns nframes_
  size_t getLocalMap(PointCloud& map);
 private:
  std::shared_ptr<Engine> eng_;
};

// liodom::Map (include/liodom/map.h:93-116) on the device.  Poses are 3 x 4 row-major isometries
// (Pose::matrix34()), the Eigen::Isometry3d of the reference.
class Map {
 public:
  explicit Map(const double xy_size, const double z_size, const double res, int device = 0);   // map.cc:70-81
  virtual ~Map();
  Map(const Map&) = delete;
  Map& operator=(const Map&) = delete;
  void updateMap(const PointCloud& pc_in, const std::array<double, 12>& pose);                  // :90-129
  PointCloud getMap();                                                                          // :131-139
  PointCloud getLocalMap(const std::array<double, 12>& pose, int cells_xy = 2, int cells_z = 1); // :141-189
  // getLocalMap for several poses in one launch (liodom_map_get_local_batch; no counterpart in the reference): one cloud per pose,
  // each what getLocalMap returns for it.
  std::vector<PointCloud> getLocalBatch(const std::vector<std::array<double, 12>>& poses, int cells_xy = 2, int cells_z = 1);
  // The map as one blob (no counterpart in the reference; layout in csrc/map_state_format.h).  exportState works on an attached
  // map too; importState and reset need a detached one (detach, import, attachMapper).
  std::vector<uint8_t> exportState();
  void importState(const std::vector<uint8_t>& blob);
  void reset();
  // Drops every cell outside the box of keep_xy / keep_z cells around the pose's cell (liodom_map_prune; no counterpart in the
  // reference); returns the number of cells removed.  Works on an attached map too.
  int prune(const std::array<double, 12>& pose, int keep_xy, int keep_z);
  // Paging (liodom_map_evict / liodom_map_merge_state; no counterpart in the reference).  evict: prune whose dropped cells come out
  // as a blob of their own (*n_evicted: how many).  mergeState: appends the cells of a blob whose keys are not cells of the map
  // yet; returns one taken flag per blob cell.  Both work on an attached map too.
  std::vector<uint8_t> evict(const std::array<double, 12>& pose, int keep_xy, int keep_z, int* n_evicted = nullptr);
  std::vector<int32_t> mergeState(const std::vector<uint8_t>& blob);
  // Relocalising (liodom_map_score_poses / liodom_map_search_pose; no counterpart in the reference).  scorePoses: hits_r, hits_0 of
  // each candidate pose for the edge cloud against the map's leaf occupancy, 2 ints per pose.  searchPose: the best candidate of the
  // grid `search` describes (liodom_pose_search_default fills one in); its pose is what LaserOdometer::seed takes.  Both only read
  // the map and work on an attached one between scans.
  std::vector<int32_t> scorePoses(const PointCloud& edges, const std::vector<std::array<double, 12>>& poses, int radius = 1);
  liodom_pose_search_result_t searchPose(const PointCloud& edges, const liodom_pose_search_t& search);
  // searchPoseBnb (liodom_map_search_pose_bnb): searchPose's result for the same grid by branch-and-bound, for grids of up to
  // 2^31 - 1 candidates; batch 0: the library's default; *stats (optional): what the search did.
  liodom_pose_search_result_t searchPoseBnb(const PointCloud& edges, const liodom_pose_search_t& search, int batch = 0,
                                            liodom_pose_search_stats_t* stats = nullptr);
  // registerPoses (liodom_map_register_poses; no counterpart in the reference): the edge cloud registered to the map in 6-DoF from
  // every start pose ([qx qy qz qw tx ty tz]) in one call; one record per pose.  opt = nullptr: liodom_map_register_default.
  // *corr (optional): per pose and edge the last pass's (a, b) indices into the row's local map, -1 without a correspondence.
  // Only reads the map; works on an attached one between scans.
  std::vector<liodom_map_registration_t> registerPoses(const PointCloud& edges, const std::vector<std::array<double, 7>>& poses,
                                                       const liodom_map_register_t* opt = nullptr, std::vector<int32_t>* corr = nullptr);
  int numCells();
  liodom_map_t* handle() const { return m_; }
  double xySize() const { return xy_; }
  double zSize() const { return z_; }
  double resolution() const { return res_; }
  int maxUpdatePoints() const { return max_update_points_; }
 private:
  PointCloud fetch(int which, const double* T, int cells_xy, int cells_z);
  liodom_map_t* m_ = nullptr;
  double xy_ = 0, z_ = 0, res_ = 0;
  int max_update_points_ = 0;
};

// The device map as a window onto a larger map on the host (no counterpart in the reference; the rule set of
// liodom_amd/pager.py).  step(pose) after a scan: the cells outside the keep box around the pose leave the
// device (Map::evict) and are stored; the stored cells inside the load box come back (Map::mergeState).  A stored cell whose key
// is a cell of the device map as well — a merge that reports taken = 0, or an evicted key that is stored already — is a conflict:
// the device keeps (gets back) its cell, the stored cell's points go through Map::updateMap with the identity pose in chunks of
// max_update_points, and the stored cell is dropped.  exportAll: the blob of device map U store, device cells first.
// keep >= load on both axes, else std::invalid_argument.
class MapPager {
 public:
  MapPager(Map* map, int keep_xy, int keep_z, int load_xy, int load_z);
  void step(const std::array<double, 12>& pose);
  std::vector<uint8_t> exportAll();
  size_t stored() const { return store_.size(); }
  long long evicted = 0, loaded = 0, conflicts = 0;
 private:
  struct Cell { std::array<int32_t, 3> key, corner_leaf; std::vector<float> xyzi; };
  bool inBox(const std::array<int32_t, 3>& key, const std::array<int32_t, 3>& centre, int n_xy, int n_z) const;
  void reobserve(const std::vector<float>& xyzi);
  Map* map_;
  int keep_xy_, keep_z_, load_xy_, load_z_;
  std::list<Cell> store_;                                                  // eviction order
  std::map<std::array<int32_t, 3>, std::list<Cell>::iterator> index_;
};

// A place database (liodom_places_*; no counterpart in the reference): key frames' edge clouds in the sensor frame as binary polar
// descriptors, and the K nearest places of a query cloud with the yaw offset each matches at (include/liodom_hip.h "finding the
// place").  An object of its own: no Engine, no Map.  addIfKeyFrame applies the distance policy of csrc/place_policy.h.
class PlaceDb {
 public:
  PlaceDb(int max_places, int max_edges, const liodom_place_geometry_t* geom = nullptr);      // null: the default geometry
  ~PlaceDb();
  PlaceDb(const PlaceDb&) = delete;
  PlaceDb& operator=(const PlaceDb&) = delete;
  int add(const PointCloud& edges, const Pose& pose, int64_t id = 0);                          // the new place's index
  // add(), if `pose` has moved min_dist metres or min_yaw radians from the last key frame's (the first pose always has): the index, or -1
  int addIfKeyFrame(const PointCloud& edges, const Pose& pose, int64_t id, double min_dist, double min_yaw);
  std::vector<liodom_place_match_t> query(const PointCloud& edges, int k);                     // best first; index -1 beyond the places
  int count();
  void reset();
  std::vector<uint8_t> exportState();
  void importState(const std::vector<uint8_t>& blob);
  liodom_places_t* handle() const { return db_; }
 private:
  liodom_places_t* db_ = nullptr;
  bool has_key_ = false;
  double last_key_[7] = {0, 0, 0, 1, 0, 0, 0};
};

// A pose graph over key frames (liodom_graph_*; no counterpart in the reference): nodes, edges "X_i^-1 o X_j was measured as Z
// with information Omega", and their optimisation on the device (include/liodom_hip.h "closing loops").  An object of its own: no
// Engine, no Map.  The loop that feeds and applies it is Python's (liodom_amd/loop.py); this is the thin class.
class PoseGraph {
 public:
  PoseGraph(int max_nodes, int max_edges);
  ~PoseGraph();
  PoseGraph(const PoseGraph&) = delete;
  PoseGraph& operator=(const PoseGraph&) = delete;
  int addNode(const Pose& pose, bool fixed = false);                                            // the new node's index
  void addEdge(int i, int j, const Pose& z, const std::array<double, 36>& info, int kind = 0);
  void addEdges(const std::vector<liodom_graph_edge_t>& edges);
  void setFixed(int node, bool fixed);
  int nodes();
  int edges();
  Pose pose(int node);
  void setPose(int node, const Pose& pose);
  void reset();
  // chi2 per edge, gradient [6 N], diagonal blocks [N x 36] at the current poses; null: not wanted
  void linearize(std::vector<double>* chi2, std::vector<double>* gradient, std::vector<double>* diag);
  std::vector<double> multiply(const std::vector<double>& x, double lambda = 0.0);              // (H + lambda diag H) x
  liodom_graph_report_t optimize(const liodom_graph_options_t* options = nullptr);              // null: the defaults
  // robust losses and switched-off edges (include/liodom_hip.h "robust losses"): loss one of LIODOM_GRAPH_LOSS_*, per edge kind 0 .. 15
  void setLoss(int kind, int loss, double scale = 1.0);
  std::pair<int, double> loss(int kind);                                                        // (loss, scale)
  void setEdgeActive(int first, const std::vector<bool>& active);                               // edges first .. first + size - 1
  std::vector<bool> edgeActive();
  void edgeWeights(std::vector<double>* rho, std::vector<double>* weight);                      // per edge; null: not wanted
  // covariances and the loop gate (include/liodom_hip.h "covariances of the graph"); options null: the defaults.
  // covariance: blocks [n x 36] = Sigma[rows[k], cols[k]] of H^-1 at the current poses (cols empty: the marginals Sigma[n, n]) and
  // their LIODOM_GRAPH_COV_* statuses.  gateEdges: d2 per candidate edge (not added) and its status.
  void covariance(const std::vector<int32_t>& rows, const std::vector<int32_t>& cols, std::vector<double>* blocks, std::vector<int32_t>* status,
                  const liodom_graph_cov_options_t* options = nullptr);
  void gateEdges(const std::vector<liodom_graph_edge_t>& candidates, std::vector<double>* d2, std::vector<int32_t>* status,
                 const liodom_graph_cov_options_t* options = nullptr);
  liodom_graph_t* handle() const { return g_; }
 private:
  liodom_graph_t* g_ = nullptr;
};

// The numbers LaserOdometer::publishOdom puts into nav_msgs/Odometry, geometry_msgs/TwistStamped
// and the fixed_frame -> base_frame TF (laser_odometry.cc:395-446).
struct OdometryMsg {
  std::string frame_id, child_frame_id;   // params->fixed_frame_, params->base_frame_
  double stamp = 0;
  double orientation[4] = {0, 0, 0, 1};   // x y z w, pose * laser_to_base_
  double position[3] = {0, 0, 0};
  double linear[3] = {0, 0, 0};           // delta translation / delta stamp
  double angular[3] = {0, 0, 0};          // tf RPY of the delta rotation / delta stamp
  // pose.covariance in nav_msgs/Odometry order (x y z rotX rotY rotZ): zeros, as the reference publishes, unless the engine was
  // created with pose covariance; then the scan's record (liodom_pose_cov_t) converted by pose_cov_to_ros for the published
  // pose (pose * laser_to_base_) — NaN where the record has none (covariance_flags other than LIODOM_COV_VALID alone)
  double pose_covariance[36] = {0};
  bool has_covariance = false;
  uint32_t covariance_flags = 0;
};

class LaserOdometer {
 public:
  explicit LaserOdometer(std::shared_ptr<Engine> engine);
  // publishOdom (laser_odometry.cc:395-446) for the pose returned by the last process / processScan
  OdometryMsg publishOdom(double stamp, const Pose& pose);
  // SharedData::setLocalMap (shared_data.cc:91-96), fed by mapClb (liodom_node.cc:57-64); mapping_ only
  void setLocalMap(const PointCloud& map);
  // SharedData::setLastIMUOri (shared_data.cc:107-111), fed by imuClb (liodom_node.cc:66-70); use_imu_ only
  void setLastIMUOri(const double q_xyzw[4]);
  // laser_to_base_ (TF lookup, laser_odometry.cc:110-119); identity by default
  void setLaserToBase(const std::array<double, 12>& T);
  // Zero-latency on-device replay of the liodom_mapping node (liodom_attach_mapper); mapping_ only
  void attachMapper(Map* map, int cells_xy = 2, int cells_z = 1);
  // ... with options (liodom_attach_mapper_ex): lag = 1 makes the map take a frame when it leaves the sliding window — the mode
  // that solves; lag = 0 is the faithful, degenerate replay above —, prune_period > 0 prunes the map around the pose as it goes
  void attachMapper(Map* map, const liodom_mapper_options_t& options);
  // Localising in a saved map (liodom_attach_map_reader / liodom_seed_stream; no counterpart in the reference).  attachMapReader:
  // after every scan the odometer receives getLocalMap(pose) of `map`, which is never written; attachMapper(nullptr) detaches.
  // seed: the next scan is the first and solves from `pose`; with a map attached the odometer receives its local map there.
  void attachMapReader(Map* map, int cells_xy = 2, int cells_z = 1);
  void seed(const Pose& pose);
  // Knowing that a reader is lost (liodom_set_map_hits / liodom_get_map_hit_log; no counterpart in the reference).  setMapHits:
  // radius 0 | 1 gives every scan a hit record against the attached reader's map, -1 switches them off.  mapHit: the record of scan
  // `scan_index` (liodom_step_info_t::scan_index of the scan); liodom_amd/csrc/track_policy.h says what to make of it.
  void setMapHits(int radius);
  liodom_map_hit_t mapHit(int scan_index);
  // One pass of the loop body of LaserOdometer::operator() (laser_odometry.cc:107-267).
  Pose process(const PointCloud& feats, double stamp, liodom_step_info_t* info = nullptr);
  // The same on an edge cloud the extractor left on the device (Features::ticket)
  Pose process(const Features& feats, liodom_step_info_t* info = nullptr);
  // lidarClb -> extractor -> odometer without leaving the device (one H2D copy, one result record)
  Pose processScan(const PointCloud& pc_in, double stamp, liodom_step_info_t* info = nullptr);
  // The same for a polar blob (liodom_process_scan_polar): the driver's projection runs on the device as well
  Pose processScanPolar(const std::vector<uint8_t>& blob, double stamp, liodom_step_info_t* info = nullptr);
  // The worker loop of the odometer thread (laser_odometry.cc:100-272): pop features, process, publish.
  // `published` (optional) receives every message in order.
  void operator()(std::atomic<bool>& running, std::vector<OdometryMsg>* published = nullptr, std::vector<Pose>* poses = nullptr);
  // Checkpoint of this odometer: Engine::saveState's blob followed by what publishOdom keeps on the host (previous published pose
  // and stamp), so that the ~odom / ~twist numbers of a resumed run carry on exactly.  loadState takes it back; reset starts over.
  std::vector<uint8_t> saveState();
  void loadState(const std::vector<uint8_t>& state);
  void reset();
  LocalMapManager lmap_manager;
 private:
  std::shared_ptr<Engine> eng_;
  Params* params;
  Stats* stats;
  std::array<double, 12> prev_odom_{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};      // laser_odometry.h:95
  std::array<double, 12> laser_to_base_{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};  // laser_odometry.h:104
  double prev_stamp_ = 0.0;                                                     // laser_odometry.h:97
  bool published_ = false;
  int last_scan_ = -1;                     // scan_index of the pose returned last (its covariance record goes into publishOdom's message)
  // output-rate watchdog (laser_odometry.cc:239-256; state laser_odometry.h:105-111, initial values laser_odometry.cc:83-90)
  void updateFrequencies(double in_stamp_secs, double now_secs);
  Pose fusedScan(double stamp, liodom_step_info_t* info, const std::function<void(double*, liodom_step_info_t*)>& call);
  double in_freqs_[5], out_freqs_[5];
  double mean_in_freq_ = 100.0, mean_out_freq_ = 100.0;
  int num_freqs_ = 0;
  double last_in_time_secs_ = 0.0, last_out_time_secs_ = 0.0;
  int freq_warnings_ = 0;
  bool init_ = false;                                                           // laser_odometry.h:94
 public:
  // mean input / output frequency over the last five scans and the number of "Output frequency too low" warnings so far
  double meanInFreq() const { return mean_in_freq_; }
  double meanOutFreq() const { return mean_out_freq_; }
  int frequencyWarnings() const { return freq_warnings_; }
};

}  // namespace liodom
