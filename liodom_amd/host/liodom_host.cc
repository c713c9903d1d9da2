#include "liodom_host.h"
#include "../csrc/liodom_math.h"   // odom_message: the same header the kernels use
#include "../csrc/map_state_cells.h"   // blobs of paged-out cells, taken apart and put together
#include "../csrc/place_policy.h"      // when a scan becomes a key frame of a PlaceDb

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <thread>

namespace liodom {

namespace {
void check(int rc, const char* what) {
  if (rc != LIODOM_OK) throw std::runtime_error(std::string(what) + ": " + liodom_last_error());
}
}  // namespace

std::array<double, 12> Pose::matrix34() const {
  // Eigen::Quaterniond::toRotationMatrix + translation (laser_odometry.cc:225-227)
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  return {1 - (tyy + tzz), txy - twz, txz + twy, t[0],
          txy + twz, 1 - (txx + tzz), tyz - twx, t[1],
          txz - twy, tyz + twx, 1 - (txx + tyy), t[2]};
}

Params* Params::getInstance() { static Params inst; return &inst; }

void Params::readParams(const std::vector<std::string>& kv) {
  for (const std::string& s : kv) {
    const size_t eq = s.find('=');
    if (eq == std::string::npos) continue;
    const std::string k = s.substr(0, eq), v = s.substr(eq + 1);
    auto b = [&](const std::string& x) { return x == "true" || x == "1" || x == "True"; };
    if (k == "min_range") min_range_ = std::stod(v);                 // params.cc:40
    else if (k == "max_range") max_range_ = std::stod(v);            // :44
    else if (k == "lidar_type") lidar_type_ = std::stoi(v);          // :48
    else if (k == "scan_lines") scan_lines_ = std::stoi(v);          // :52
    else if (k == "scan_regions") scan_regions_ = std::stoi(v);      // :56
    else if (k == "edges_per_region") edges_per_region_ = std::stoi(v);   // :60
    else if (k == "save_results") save_results_ = b(v);              // :66
    else if (k == "save_results_dir") results_dir_ = v;              // :70
    else if (k == "fixed_frame") fixed_frame_ = v;                   // :74
    else if (k == "base_frame") base_frame_ = v;                     // :78
    else if (k == "laser_frame") laser_frame_ = v;                   // :82
    else if (k == "prev_frames") local_map_size_ = (size_t)std::stoi(v);  // :90-93
    else if (k == "use_imu") use_imu_ = b(v);                        // :96
    else if (k == "filter_local_map") filter_local_map_ = b(v);      // :100
    else if (k == "mapping") mapping_ = b(v);                        // :104
    else if (k == "publish_tf") publish_tf_ = b(v);                  // :108
  }
  min_points_per_scan_ = (size_t)(scan_regions_ * edges_per_region_ + 10);   // :63
}

liodom_params_t Params::toC() const {
  liodom_params_t c;
  liodom_params_default(&c);
  c.min_range = min_range_; c.max_range = max_range_;
  c.lidar_type = lidar_type_; c.scan_lines = scan_lines_;
  c.scan_regions = scan_regions_; c.edges_per_region = edges_per_region_;
  c.min_points_per_scan = min_points_per_scan_; c.local_map_size = local_map_size_;
  c.save_results = save_results_;
  std::strncpy(c.results_dir, results_dir_.c_str(), sizeof(c.results_dir) - 1);
  std::strncpy(c.fixed_frame, fixed_frame_.c_str(), sizeof(c.fixed_frame) - 1);
  std::strncpy(c.base_frame, base_frame_.c_str(), sizeof(c.base_frame) - 1);
  std::strncpy(c.laser_frame, laser_frame_.c_str(), sizeof(c.laser_frame) - 1);
  c.use_imu = use_imu_; c.filter_local_map = filter_local_map_; c.mapping = mapping_; c.publish_tf = publish_tf_;
  return c;
}

Stats* Stats::getInstance() { static Stats inst; return &inst; }
void Stats::addPose(const std::array<double, 12>& p) { poses_.push_back(p); n_poses_.fetch_add(1, std::memory_order_release); }
size_t Stats::numPoses() { return n_poses_.load(std::memory_order_acquire); }
void Stats::addFeatureExtractionTime(const Clock::time_point& s, const Clock::time_point& e) {
  feat_extr_.push_back((double)std::chrono::duration_cast<std::chrono::milliseconds>(e - s).count());   // whole ms, stats.cc:42
}
void Stats::addLaserOdometryTime(const Clock::time_point& s, const Clock::time_point& e) {
  laser_odom_.push_back((double)std::chrono::duration_cast<std::chrono::milliseconds>(e - s).count());
}
void Stats::addNumOfFeats(const size_t& n) { num_of_features_.push_back(n); }
void Stats::startFrame(const Clock::time_point& s) { std::lock_guard<std::mutex> l(frame_mutex_); start_times_.push(s); }
void Stats::stopFrame(const Clock::time_point& stop) {
  std::lock_guard<std::mutex> l(frame_mutex_);
  if (!start_times_.empty()) {
    const Clock::time_point start = start_times_.front();
    start_times_.pop();
    frame_times_.push_back((double)std::chrono::duration_cast<std::chrono::milliseconds>(stop - start).count());
  }
}
void Stats::dropLastScan() {
  if (!poses_.empty()) { poses_.pop_back(); n_poses_.fetch_sub(1, std::memory_order_release); }
  if (!laser_odom_.empty()) laser_odom_.pop_back();
  if (!frame_times_.empty()) frame_times_.pop_back();
  if (!num_of_features_.empty()) num_of_features_.pop_back();
}
void Stats::clear() { n_poses_ = 0; poses_.clear(); feat_extr_.clear(); laser_odom_.clear(); frame_times_.clear(); num_of_features_.clear(); }

// File formats of Stats::writeResults (stats.cc:73-132): poses.txt = KITTI rows of the top 3x4 of
// the pose with default ostream precision; the other files one value per line.
void Stats::writeResults(const std::string& dir) {
  std::ofstream poses((dir + "poses.txt").c_str(), std::ios::out | std::ios::trunc);
  for (const auto& p : poses_) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 4; j++) {
        poses << p[i * 4 + j];
        if (j != 3) poses << " ";
        else if (i == 2) poses << std::endl;
        else poses << " ";
      }
  }
  auto dump = [&](const char* name, const std::vector<double>& v) {
    std::ofstream f((dir + name).c_str(), std::ios::out | std::ios::trunc);
    for (double x : v) f << x << std::endl;
  };
  dump("feat_ext_times.txt", feat_extr_);
  dump("laser_odom_times.txt", laser_odom_);
  {
    std::ofstream f((dir + "nfeats.txt").c_str(), std::ios::out | std::ios::trunc);
    for (size_t x : num_of_features_) f << x << std::endl;
  }
  dump("frame_times.txt", frame_times_);
}

SharedData* SharedData::getInstance() { static SharedData inst; return &inst; }
void SharedData::pushPointCloud(const PointCloud& pc_in, double stamp) {
  std::lock_guard<std::mutex> lk(pc_mutex_);
  pc_buf_.push(std::make_pair(pc_in, stamp));
}
bool SharedData::popPointCloud(PointCloud& pc_out, double& stamp) {
  std::lock_guard<std::mutex> lk(pc_mutex_);
  if (pc_buf_.empty()) return false;
  pc_out = std::move(pc_buf_.front().first); stamp = pc_buf_.front().second;
  pc_buf_.pop();
  return true;
}
void SharedData::pushFeatures(const PointCloud& feat_in, double stamp) {
  Features f; f.edges = feat_in; f.stamp = stamp;
  pushFeatures(std::move(f));
}
bool SharedData::popFeatures(PointCloud& feat_out, double& stamp) {
  Features f;
  if (!popFeatures(f)) return false;
  feat_out = std::move(f.edges); stamp = f.stamp;
  return true;
}
void SharedData::pushFeatures(Features&& f) {
  std::lock_guard<std::mutex> lk(feat_mutex_);
  feat_buf_.push(std::move(f));
}
bool SharedData::popFeatures(Features& f) {
  std::lock_guard<std::mutex> lk(feat_mutex_);
  if (feat_buf_.empty()) return false;
  f = std::move(feat_buf_.front());
  feat_buf_.pop();
  return true;
}
size_t SharedData::numFeatures() { std::lock_guard<std::mutex> lk(feat_mutex_); return feat_buf_.size(); }
void SharedData::clear() {
  std::lock_guard<std::mutex> a(pc_mutex_), b(feat_mutex_);
  pc_buf_ = {}; feat_buf_ = {};
}

Engine::Engine(const Params& p, int device, int max_points, int max_width, int pose_rotation_mode, int pose_covariance) {
  liodom_params_t cp = p.toC();
  liodom_config_t cfg;
  liodom_config_default(&cfg);
  cfg.device = device; cfg.n_streams = 1; cfg.max_points = max_points; cfg.max_width = max_width;
  cfg.pose_rotation_mode = pose_rotation_mode; rotation_mode_ = pose_rotation_mode != 0 ? 1 : 0;
  cfg.pose_covariance = pose_covariance != 0 ? 1 : 0; covariance_ = pose_covariance != 0;
  check(liodom_create(&cp, &cfg, &h_), "liodom_create");
  edge_cap_ = p.scan_lines_ * p.scan_regions_ * (p.edges_per_region_ + 1) + 64;
}
Engine::~Engine() { liodom_destroy(h_); }

PolarGeometry PolarGeometry::fromAngles(int height, int width, const std::vector<double>& altitude, const std::vector<double>& beam_azimuth,
                                        const std::vector<double>& encoder, int range_bits, int intensity_bits, float range_unit,
                                        float beam_origin) {
  if (height < 1 || altitude.size() != (size_t)height || beam_azimuth.size() != (size_t)height || encoder.empty())
    throw std::invalid_argument("PolarGeometry::fromAngles: altitude and beam_azimuth need one angle per row, encoder at least one tick");
  PolarGeometry g;
  g.height = height; g.width = width; g.range_bits = range_bits; g.intensity_bits = intensity_bits;
  g.range_unit = range_unit; g.beam_origin = beam_origin;
  for (double a : altitude) { g.cos_alt.push_back((float)std::cos(a)); g.sin_alt.push_back((float)std::sin(a)); }
  for (double a : beam_azimuth) { g.cos_baz.push_back((float)std::cos(a)); g.sin_baz.push_back((float)std::sin(a)); }
  for (double a : encoder) { g.cos_enc.push_back((float)std::cos(a)); g.sin_enc.push_back((float)std::sin(a)); }
  return g;
}
liodom_polar_geometry_t PolarGeometry::toC() const {
  liodom_polar_geometry_t c;
  std::memset(&c, 0, sizeof(c));
  c.height = height; c.width = width; c.range_bits = range_bits; c.intensity_bits = intensity_bits;
  c.range_unit = range_unit; c.beam_origin = beam_origin;
  const bool rows = (int)cos_alt.size() == height && (int)sin_alt.size() == height && (int)cos_baz.size() == height && (int)sin_baz.size() == height;
  if (rows) { c.cos_alt = cos_alt.data(); c.sin_alt = sin_alt.data(); c.cos_baz = cos_baz.data(); c.sin_baz = sin_baz.data(); }
  if (cos_enc.size() == sin_enc.size()) { c.ticks = (int32_t)cos_enc.size(); c.cos_enc = cos_enc.data(); c.sin_enc = sin_enc.data(); }
  return c;      // (tables of the wrong length stay null: liodom_set_polar_geometry refuses them)
}
liodom_polar_layout_t PolarGeometry::layout() const {
  const liodom_polar_geometry_t c = toC();
  liodom_polar_layout_t lay;
  check(liodom_polar_layout(&c, &lay), "liodom_polar_layout");
  return lay;
}
void Engine::setPolarGeometry(const PolarGeometry& g) {
  const liodom_polar_geometry_t c = g.toC();
  check(liodom_set_polar_geometry(h_, &c), "liodom_set_polar_geometry");
  polar_n_ = g.height * g.width;
}
void Engine::resetStream(int stream) { check(liodom_reset_stream(h_, stream), "liodom_reset_stream"); }
std::vector<uint8_t> Engine::saveState(int stream) {
  int64_t cap = 0, n = 0;
  check(liodom_stream_state_size(h_, &cap), "liodom_stream_state_size");
  std::vector<uint8_t> blob((size_t)cap);
  check(liodom_export_stream_state(h_, stream, blob.data(), cap, &n), "liodom_export_stream_state");
  blob.resize((size_t)n);
  return blob;
}
std::vector<liodom_odom_edge_t> Engine::odometryEdges(const std::vector<int32_t>& scan_from, const std::vector<int32_t>& scan_to,
                                                      const liodom_odom_edge_options_t* opt, int stream) {
  if (scan_from.size() != scan_to.size()) throw std::invalid_argument("Engine::odometryEdges: one scan_to per scan_from");
  std::vector<liodom_odom_edge_t> out(scan_from.size());
  check(liodom_get_odometry_edges(h_, stream, scan_from.data(), scan_to.data(), (int)scan_from.size(), opt, out.data()),
        "liodom_get_odometry_edges");
  return out;
}
void Engine::loadState(const std::vector<uint8_t>& blob, int stream) {
  check(liodom_import_stream_state(h_, stream, blob.data(), (int64_t)blob.size()), "liodom_import_stream_state");
}

std::vector<std::array<double, 7>> Engine::stepSubset(int slot, const std::vector<int32_t>& streams, int64_t n, int height, int width,
                                                      int next_slot, const std::vector<int32_t>* next_streams) {
  std::vector<std::array<double, 7>> poses(streams.size());
  std::vector<liodom_step_info_t> infos(streams.size());
  check(liodom_process_resident_subset(h_, slot, streams.data(), (int)streams.size(), next_slot,
                                       next_streams ? next_streams->data() : nullptr, next_streams ? (int)next_streams->size() : 0,
                                       n, height, width, poses.empty() ? nullptr : poses[0].data(), infos.empty() ? nullptr : infos.data()),
        "liodom_process_resident_subset");
  return poses;
}

FeatureExtractor::FeatureExtractor(std::shared_ptr<Engine> e)
    : eng_(std::move(e)), params(Params::getInstance()), stats(Stats::getInstance()) {}

void FeatureExtractor::extractFeatures(const PointCloud& pc_in, PointCloud& pc_edges) {
  const auto start_t = Clock::now();
  pc_edges.points.resize((size_t)eng_->edge_capacity());
  int n = 0;
  check(liodom_extract_edges(eng_->handle(), 0, reinterpret_cast<const float*>(pc_in.points.data()),
                             (int64_t)pc_in.size(), (int)pc_in.height, (int)pc_in.width,
                             reinterpret_cast<float*>(pc_edges.points.data()), nullptr, nullptr, nullptr,
                             eng_->edge_capacity(), &n), "liodom_extract_edges");
  pc_edges.points.resize((size_t)n);
  pc_edges.width = (uint32_t)n; pc_edges.height = 1;
  if (params->save_results_) {                                        // feature_extractor.cc:65-68
    stats->addFeatureExtractionTime(start_t, Clock::now());
    stats->addNumOfFeats(pc_edges.size());
  }
}

void FeatureExtractor::projectPolar(const std::vector<uint8_t>& blob, PointCloud& pc_out) {
  pc_out.points.resize((size_t)eng_->polarPoints());
  check(liodom_project_polar(eng_->handle(), blob.data(), reinterpret_cast<float*>(pc_out.points.data())), "liodom_project_polar");
  pc_out.width = (uint32_t)pc_out.points.size(); pc_out.height = 1;
}

bool FeatureExtractor::extractFeaturesPolar(const std::vector<uint8_t>& blob, double stamp, Features& f) {
  const auto start_t = Clock::now();
  f.stamp = stamp;
  const int rc = liodom_extract_edges_device_polar(eng_->handle(), 0, blob.data(), &f.ticket);
  if (rc == LIODOM_ERR_BUSY) return false;
  check(rc, "liodom_extract_edges_device_polar");
  f.edges.points.resize((size_t)eng_->edge_capacity());
  int n = 0;
  check(liodom_wait_edges(eng_->handle(), &f.ticket, reinterpret_cast<float*>(f.edges.points.data()), nullptr, nullptr, nullptr,
                          eng_->edge_capacity(), &n), "liodom_wait_edges");
  f.edges.points.resize((size_t)n);
  f.edges.width = (uint32_t)n; f.edges.height = 1;
  if (params->save_results_) {                                        // feature_extractor.cc:65-68
    stats->addFeatureExtractionTime(start_t, Clock::now());
    stats->addNumOfFeats(f.edges.size());
  }
  return true;
}

static void worker_pause(SharedData* sdata) {                          // feature_extractor.cc:80 / laser_odometry.cc:270
  const int us = sdata->poll_us.load(std::memory_order_relaxed);
  if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
  else std::this_thread::yield();
}

void FeatureExtractor::operator()(std::atomic<bool>& running) {
  SharedData* sdata = SharedData::getInstance();
  PointCloud pc_curr;
  double stamp = 0;
  bool have = false;             // a cloud popped while every hand-off slot was taken: retried, the reference's queue is unbounded
  while (running) {                                                   // feature_extractor.cc:46
    if (have || sdata->popPointCloud(pc_curr, stamp)) {               // :49
      if (!device_handoff_) {
        PointCloud pc_edges;
        extractFeatures(pc_curr, pc_edges);                           // :53-59
        sdata->pushFeatures(pc_edges, stamp);                         // :77
        have = false;
      } else {
        const auto start_t = Clock::now();
        Features f;
        f.stamp = stamp;
        const int rc = liodom_extract_edges_device(eng_->handle(), 0, reinterpret_cast<const float*>(pc_curr.points.data()),
                                                   (int64_t)pc_curr.size(), (int)pc_curr.height, (int)pc_curr.width, &f.ticket);
        if (rc == LIODOM_ERR_BUSY) { have = true; worker_pause(sdata); continue; }
        check(rc, "liodom_extract_edges_device");
        have = false;
        // the cloud for ~edges (:70-75) out of the extraction's host-mapped mirror
        f.edges.points.resize((size_t)eng_->edge_capacity());
        int n = 0;
        check(liodom_wait_edges(eng_->handle(), &f.ticket, reinterpret_cast<float*>(f.edges.points.data()), nullptr, nullptr, nullptr,
                                eng_->edge_capacity(), &n), "liodom_wait_edges");
        f.edges.points.resize((size_t)n);
        f.edges.width = (uint32_t)n; f.edges.height = 1;
        if (params->save_results_) {                                  // :65-68
          stats->addFeatureExtractionTime(start_t, Clock::now());
          stats->addNumOfFeats(f.edges.size());
        }
        sdata->pushFeatures(std::move(f));                            // :77
      }
    }
    worker_pause(sdata);                                              // :80
  }
}

void FeatureExtractor::lastEdges(PointCloud& pc_edges) {
  pc_edges.points.resize((size_t)eng_->edge_capacity());
  int n = 0;
  check(liodom_get_edges(eng_->handle(), 0, reinterpret_cast<float*>(pc_edges.points.data()), nullptr, nullptr, nullptr,
                         eng_->edge_capacity(), &n), "liodom_get_edges");
  pc_edges.points.resize((size_t)n);
  pc_edges.width = (uint32_t)n; pc_edges.height = 1;
}

size_t LocalMapManager::getLocalMap(PointCloud& map) {
  int64_t n = 0; int nf = 0;
  liodom_get_window(eng_->handle(), 0, nullptr, 0, &n, &nf);         // size query
  map.points.resize((size_t)n);
  check(liodom_get_window(eng_->handle(), 0, reinterpret_cast<float*>(map.points.data()), n, &n, &nf), "liodom_get_window");
  map.width = (uint32_t)n; map.height = 1;
  return (size_t)nf;
}

Map::Map(const double xy_size, const double z_size, const double res, int device) {
  liodom_map_config_t c;
  liodom_map_config_default(&c);
  c.device = device; c.voxel_xysize = xy_size; c.voxel_zsize = z_size; c.resolution = res;
  check(liodom_map_create(&c, &m_), "liodom_map_create");
  xy_ = xy_size; z_ = z_size; res_ = res; max_update_points_ = c.max_update_points;
}
Map::~Map() { liodom_map_destroy(m_); }

void Map::updateMap(const PointCloud& pc_in, const std::array<double, 12>& pose) {
  check(liodom_map_update(m_, reinterpret_cast<const float*>(pc_in.points.data()), (int64_t)pc_in.size(), pose.data()),
        "liodom_map_update");
}

PointCloud Map::fetch(int which, const double* T, int cells_xy, int cells_z) {
  PointCloud out;
  int64_t n = 0;
  // size query first (LIODOM_ERR_CAPACITY with the size filled in), then the copy
  if (which == 0) liodom_map_get_all(m_, nullptr, 0, &n); else liodom_map_get_local(m_, T, cells_xy, cells_z, nullptr, 0, &n);
  out.points.resize((size_t)n);
  float* dst = reinterpret_cast<float*>(out.points.data());
  if (n > 0) {
    if (which == 0) check(liodom_map_get_all(m_, dst, n, &n), "liodom_map_get_all");
    else check(liodom_map_get_local(m_, T, cells_xy, cells_z, dst, n, &n), "liodom_map_get_local");
  }
  out.width = (uint32_t)n; out.height = 1;
  return out;
}
PointCloud Map::getMap() { return fetch(0, nullptr, 0, 0); }
std::vector<uint8_t> Map::exportState() {
  int64_t n = 0;
  check(liodom_map_state_size(m_, &n), "liodom_map_state_size");
  std::vector<uint8_t> blob((size_t)n);
  check(liodom_map_export_state(m_, blob.data(), n, &n), "liodom_map_export_state");
  blob.resize((size_t)n);
  return blob;
}
void Map::importState(const std::vector<uint8_t>& blob) {
  check(liodom_map_import_state(m_, blob.data(), (int64_t)blob.size()), "liodom_map_import_state");
}
void Map::reset() { check(liodom_map_reset(m_), "liodom_map_reset"); }
PointCloud Map::getLocalMap(const std::array<double, 12>& pose, int cells_xy, int cells_z) {
  return fetch(1, pose.data(), cells_xy, cells_z);
}

void LaserOdometer::setLocalMap(const PointCloud& map) {
  check(liodom_set_received_map(eng_->handle(), 0, reinterpret_cast<const float*>(map.points.data()), (int64_t)map.size()),
        "liodom_set_received_map");
}
void LaserOdometer::setLastIMUOri(const double q_xyzw[4]) {
  check(liodom_set_imu_orientation(eng_->handle(), 0, q_xyzw), "liodom_set_imu_orientation");
}
void LaserOdometer::setLaserToBase(const std::array<double, 12>& T) {
  check(liodom_set_laser_to_base(eng_->handle(), T.data()), "liodom_set_laser_to_base");
  laser_to_base_ = T;
}

OdometryMsg LaserOdometer::publishOdom(double stamp, const Pose& pose) {
  OdometryMsg msg;
  msg.frame_id = params->fixed_frame_;             // :398
  msg.child_frame_id = params->base_frame_;        // :399
  msg.stamp = stamp;                               // :400
  const std::array<double, 12> cur = pose.matrix34();
  // first frame: prev_stamp_ is set to the frame's own stamp before publishing (:125,136), so the
  // first twist is 0 / 0 = NaN exactly as the reference publishes it
  if (!published_) { prev_stamp_ = stamp; published_ = true; }
  double out[13];
  liodom_dev::odom_message(prev_odom_.data(), cur.data(), laser_to_base_.data(), stamp - prev_stamp_, eng_->rotation_mode(), out);
  std::memcpy(msg.orientation, out, sizeof(double) * 4);
  std::memcpy(msg.position, out + 4, sizeof(double) * 3);
  std::memcpy(msg.linear, out + 7, sizeof(double) * 3);
  std::memcpy(msg.angular, out + 10, sizeof(double) * 3);
  if (eng_->covariance() && last_scan_ >= 0) {
    liodom_pose_cov_t rec;
    check(liodom_wait_pose_covariance(eng_->handle(), 0, last_scan_, &rec), "liodom_wait_pose_covariance");
    liodom_dev::pose_cov_to_ros(rec.covariance, cur.data(), laser_to_base_.data(), msg.pose_covariance);
    msg.has_covariance = true;
    msg.covariance_flags = rec.flags;
  }
  prev_odom_ = cur;                                // the reference's prev_odom_ (:149) is the pose of the previous scan here
  prev_stamp_ = stamp;                             // :266
  return msg;
}
// Host trailer behind the engine's blob: magic, prev_odom_ [12], prev_stamp_, published_ / init_ / last_scan_.
namespace {
struct HostTrailer { char magic[8]; double prev_odom[12]; double prev_stamp; int32_t published, init, last_scan, pad; };
}
std::vector<uint8_t> LaserOdometer::saveState() {
  std::vector<uint8_t> out = eng_->saveState(0);
  HostTrailer t;
  std::memset(&t, 0, sizeof(t));
  std::memcpy(t.magic, "LIODOMHS", 8);
  for (int i = 0; i < 12; i++) t.prev_odom[i] = prev_odom_[(size_t)i];
  t.prev_stamp = prev_stamp_; t.published = published_ ? 1 : 0; t.init = init_ ? 1 : 0; t.last_scan = last_scan_;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&t);
  out.insert(out.end(), p, p + sizeof(t));
  return out;
}
void LaserOdometer::loadState(const std::vector<uint8_t>& state) {
  HostTrailer t;
  if (state.size() < sizeof(t)) throw std::runtime_error("LaserOdometer::loadState: state too short");
  std::memcpy(&t, state.data() + state.size() - sizeof(t), sizeof(t));
  if (std::memcmp(t.magic, "LIODOMHS", 8) != 0) throw std::runtime_error("LaserOdometer::loadState: not a state written by LaserOdometer::saveState");
  eng_->loadState(std::vector<uint8_t>(state.begin(), state.end() - (std::ptrdiff_t)sizeof(t)), 0);
  for (int i = 0; i < 12; i++) prev_odom_[(size_t)i] = t.prev_odom[i];
  prev_stamp_ = t.prev_stamp; published_ = t.published != 0; init_ = t.init != 0;
  last_scan_ = -1;      // (the covariance record of the scan before the checkpoint stayed with the engine that solved it)
}
void LaserOdometer::reset() {
  eng_->resetStream(0);
  prev_odom_ = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  prev_stamp_ = 0.0; published_ = false; init_ = false; last_scan_ = -1;
}
int Map::prune(const std::array<double, 12>& pose, int keep_xy, int keep_z) {
  int n = 0;
  check(liodom_map_prune(m_, pose.data(), keep_xy, keep_z, &n), "liodom_map_prune");
  return n;
}

std::vector<uint8_t> Map::evict(const std::array<double, 12>& pose, int keep_xy, int keep_z, int* n_evicted) {
  int64_t need = 0;
  int n = 0;
  // the size query: LIODOM_ERR_CAPACITY with the size filled in and the map untouched
  const int rc = liodom_map_evict(m_, pose.data(), keep_xy, keep_z, nullptr, 0, &need, &n);
  if (rc != LIODOM_ERR_CAPACITY) check(rc, "liodom_map_evict");
  std::vector<uint8_t> blob((size_t)need);
  check(liodom_map_evict(m_, pose.data(), keep_xy, keep_z, blob.data(), need, &need, &n), "liodom_map_evict");
  blob.resize((size_t)need);
  if (n_evicted) *n_evicted = n;
  return blob;
}
std::vector<int32_t> Map::mergeState(const std::vector<uint8_t>& blob) {
  int32_t n_cells = 0;
  if (blob.size() >= 64) std::memcpy(&n_cells, blob.data() + 48, sizeof(n_cells));
  // (a count the blob's size cannot hold is rejected by the library before `taken` is written)
  std::vector<int32_t> taken((size_t)std::max<int64_t>(0, std::min<int64_t>(n_cells, ((int64_t)blob.size() - 64) / 32)));
  check(liodom_map_merge_state(m_, blob.data(), (int64_t)blob.size(), taken.empty() ? nullptr : taken.data(), nullptr), "liodom_map_merge_state");
  return taken;
}

PlaceDb::PlaceDb(int max_places, int max_edges, const liodom_place_geometry_t* geom) {
  liodom_place_geometry_t g;
  liodom_place_geometry_default(&g);
  check(liodom_places_create(geom ? geom : &g, max_places, max_edges, &db_), "liodom_places_create");
}
PlaceDb::~PlaceDb() { liodom_places_destroy(db_); }

int PlaceDb::add(const PointCloud& edges, const Pose& pose, int64_t id) {
  const double p[7] = {pose.q[0], pose.q[1], pose.q[2], pose.q[3], pose.t[0], pose.t[1], pose.t[2]};
  int32_t index = -1;
  check(liodom_places_add(db_, reinterpret_cast<const float*>(edges.points.data()), (int)edges.size(), p, id, &index), "liodom_places_add");
  return index;
}

int PlaceDb::addIfKeyFrame(const PointCloud& edges, const Pose& pose, int64_t id, double min_dist, double min_yaw) {
  const double p[7] = {pose.q[0], pose.q[1], pose.q[2], pose.q[3], pose.t[0], pose.t[1], pose.t[2]};
  liodom_dev::PlacePolicyState s;
  s.has = has_key_;
  std::memcpy(s.last, last_key_, sizeof(last_key_));
  if (!liodom_dev::place_policy_feed(liodom_dev::PlacePolicy{min_dist, min_yaw}, &s, p)) return -1;
  const int index = add(edges, pose, id);      // (throws: the last key frame stays)
  has_key_ = true;
  std::memcpy(last_key_, p, sizeof(last_key_));
  return index;
}

std::vector<liodom_place_match_t> PlaceDb::query(const PointCloud& edges, int k) {
  std::vector<liodom_place_match_t> out((size_t)std::max(k, 0));
  const int32_t n = (int32_t)edges.size();
  check(liodom_places_query(db_, reinterpret_cast<const float*>(edges.points.data()), (int64_t)n, &n, 1, k, out.data(), nullptr), "liodom_places_query");
  return out;
}

int PlaceDb::count() {
  int32_t n = 0;
  check(liodom_places_count(db_, &n), "liodom_places_count");
  return n;
}
void PlaceDb::reset() { check(liodom_places_reset(db_), "liodom_places_reset"); }

std::vector<uint8_t> PlaceDb::exportState() {
  int64_t bytes = 0;
  check(liodom_places_state_size(db_, &bytes), "liodom_places_state_size");
  std::vector<uint8_t> blob((size_t)bytes);
  check(liodom_places_export_state(db_, blob.data(), bytes, &bytes), "liodom_places_export_state");
  return blob;
}
void PlaceDb::importState(const std::vector<uint8_t>& blob) {
  check(liodom_places_import_state(db_, blob.data(), (int64_t)blob.size()), "liodom_places_import_state");
}

PoseGraph::PoseGraph(int max_nodes, int max_edges) { check(liodom_graph_create(max_nodes, max_edges, &g_), "liodom_graph_create"); }
PoseGraph::~PoseGraph() { liodom_graph_destroy(g_); }

int PoseGraph::addNode(const Pose& pose, bool fixed) {
  const double p[7] = {pose.q[0], pose.q[1], pose.q[2], pose.q[3], pose.t[0], pose.t[1], pose.t[2]};
  const int32_t f = fixed ? 1 : 0;
  int32_t first = -1;
  check(liodom_graph_add_nodes(g_, p, &f, 1, &first), "liodom_graph_add_nodes");
  return first;
}
void PoseGraph::addEdge(int i, int j, const Pose& z, const std::array<double, 36>& info, int kind) {
  liodom_graph_edge_t e;
  std::memset(&e, 0, sizeof(e));
  e.i = i; e.j = j; e.kind = kind;
  const double p[7] = {z.q[0], z.q[1], z.q[2], z.q[3], z.t[0], z.t[1], z.t[2]};
  std::memcpy(e.z, p, sizeof(p));
  std::memcpy(e.info, info.data(), sizeof(e.info));
  check(liodom_graph_add_edges(g_, &e, 1), "liodom_graph_add_edges");
}
void PoseGraph::addEdges(const std::vector<liodom_graph_edge_t>& edges) {
  check(liodom_graph_add_edges(g_, edges.data(), (int)edges.size()), "liodom_graph_add_edges");
}
void PoseGraph::setFixed(int node, bool fixed) {
  const int32_t f = fixed ? 1 : 0;
  check(liodom_graph_set_fixed(g_, node, 1, &f), "liodom_graph_set_fixed");
}
int PoseGraph::nodes() {
  int32_t n = 0;
  check(liodom_graph_count(g_, &n, nullptr), "liodom_graph_count");
  return n;
}
int PoseGraph::edges() {
  int32_t n = 0;
  check(liodom_graph_count(g_, nullptr, &n), "liodom_graph_count");
  return n;
}
Pose PoseGraph::pose(int node) {
  double p[7];
  check(liodom_graph_get_poses(g_, node, 1, p), "liodom_graph_get_poses");
  Pose out;
  for (int k = 0; k < 4; k++) out.q[k] = p[k];
  for (int k = 0; k < 3; k++) out.t[k] = p[4 + k];
  return out;
}
void PoseGraph::setPose(int node, const Pose& pose) {
  const double p[7] = {pose.q[0], pose.q[1], pose.q[2], pose.q[3], pose.t[0], pose.t[1], pose.t[2]};
  check(liodom_graph_set_poses(g_, node, 1, p), "liodom_graph_set_poses");
}
void PoseGraph::reset() { check(liodom_graph_reset(g_), "liodom_graph_reset"); }
void PoseGraph::linearize(std::vector<double>* chi2, std::vector<double>* gradient, std::vector<double>* diag) {
  int32_t n = 0, e = 0;
  check(liodom_graph_count(g_, &n, &e), "liodom_graph_count");
  if (chi2) chi2->assign((size_t)e, 0.0);
  if (gradient) gradient->assign(6 * (size_t)n, 0.0);
  if (diag) diag->assign(36 * (size_t)n, 0.0);
  check(liodom_graph_linearize(g_, chi2 ? chi2->data() : nullptr, gradient ? gradient->data() : nullptr, diag ? diag->data() : nullptr), "liodom_graph_linearize");
}
std::vector<double> PoseGraph::multiply(const std::vector<double>& x, double lambda) {
  if (x.size() != 6 * (size_t)nodes()) throw std::invalid_argument("PoseGraph::multiply: x needs 6 entries per node");
  std::vector<double> y(x.size(), 0.0);
  check(liodom_graph_multiply(g_, lambda, x.data(), y.data()), "liodom_graph_multiply");
  return y;
}
liodom_graph_report_t PoseGraph::optimize(const liodom_graph_options_t* options) {
  liodom_graph_report_t rep;
  check(liodom_graph_optimize(g_, options, &rep), "liodom_graph_optimize");
  return rep;
}
void PoseGraph::setLoss(int kind, int loss, double scale) { check(liodom_graph_set_loss(g_, kind, loss, scale), "liodom_graph_set_loss"); }
std::pair<int, double> PoseGraph::loss(int kind) {
  int32_t l = 0;
  double c = 0.0;
  check(liodom_graph_get_loss(g_, kind, &l, &c), "liodom_graph_get_loss");
  return {(int)l, c};
}
void PoseGraph::setEdgeActive(int first, const std::vector<bool>& active) {
  std::vector<int32_t> a(active.size());
  for (size_t k = 0; k < active.size(); k++) a[k] = active[k] ? 1 : 0;
  check(liodom_graph_set_edge_active(g_, first, (int)a.size(), a.data()), "liodom_graph_set_edge_active");
}
std::vector<bool> PoseGraph::edgeActive() {
  std::vector<int32_t> a((size_t)edges() + 1, 0);
  check(liodom_graph_get_edge_active(g_, 0, (int)a.size() - 1, a.data()), "liodom_graph_get_edge_active");
  std::vector<bool> out(a.size() - 1);
  for (size_t k = 0; k < out.size(); k++) out[k] = a[k] != 0;
  return out;
}
void PoseGraph::edgeWeights(std::vector<double>* rho, std::vector<double>* weight) {
  const size_t e = (size_t)edges();
  if (rho) rho->assign(e, 0.0);
  if (weight) weight->assign(e, 0.0);
  check(liodom_graph_edge_weights(g_, rho ? rho->data() : nullptr, weight ? weight->data() : nullptr), "liodom_graph_edge_weights");
}
void PoseGraph::covariance(const std::vector<int32_t>& rows, const std::vector<int32_t>& cols, std::vector<double>* blocks, std::vector<int32_t>* status,
                           const liodom_graph_cov_options_t* options) {
  const std::vector<int32_t>& c = cols.empty() ? rows : cols;
  if (c.size() != rows.size() || !blocks || !status) throw std::invalid_argument("PoseGraph::covariance: one column node per row node, and both outputs");
  blocks->assign(36 * rows.size(), 0.0);
  status->assign(rows.size(), 0);
  check(liodom_graph_covariance(g_, rows.data(), c.data(), (int)rows.size(), options, blocks->data(), status->data()), "liodom_graph_covariance");
}
void PoseGraph::gateEdges(const std::vector<liodom_graph_edge_t>& candidates, std::vector<double>* d2, std::vector<int32_t>* status,
                          const liodom_graph_cov_options_t* options) {
  if (!d2 || !status) throw std::invalid_argument("PoseGraph::gateEdges: both outputs are needed");
  d2->assign(candidates.size(), 0.0);
  status->assign(candidates.size(), 0);
  check(liodom_graph_gate_edges(g_, candidates.data(), (int)candidates.size(), options, d2->data(), status->data()), "liodom_graph_gate_edges");
}

MapPager::MapPager(Map* map, int keep_xy, int keep_z, int load_xy, int load_z)
    : map_(map), keep_xy_(keep_xy), keep_z_(keep_z), load_xy_(load_xy), load_z_(load_z) {
  if (!map || load_xy < 0 || load_z < 0 || keep_xy < load_xy || keep_z < load_z) throw std::invalid_argument("MapPager: needs keep >= load >= 0 on both axes");
}
bool MapPager::inBox(const std::array<int32_t, 3>& key, const std::array<int32_t, 3>& centre, int n_xy, int n_z) const {
  // the keep rule of liodom_map_prune, compared in double
  const double lim_xy = (double)n_xy * map_->xySize(), lim_z = (double)n_z * map_->zSize();
  return std::fabs((double)key[0] - (double)centre[0]) <= lim_xy && std::fabs((double)key[1] - (double)centre[1]) <= lim_xy &&
         std::fabs((double)key[2] - (double)centre[2]) <= lim_z;
}
void MapPager::reobserve(const std::vector<float>& xyzi) {
  const std::array<double, 12> I{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  const size_t n = xyzi.size() / 4, cap = (size_t)std::max(1, map_->maxUpdatePoints());
  for (size_t lo = 0; lo < n; lo += cap) {
    PointCloud pc;
    pc.points.resize(std::min(cap, n - lo));
    std::memcpy(pc.points.data(), xyzi.data() + 4 * lo, sizeof(Point) * pc.points.size());
    pc.width = (uint32_t)pc.points.size();
    map_->updateMap(pc, I);
  }
}
void MapPager::step(const std::array<double, 12>& pose) {
  using liodom_dev::MapStateCell;
  const double xy = map_->xySize(), z = map_->zSize(), res = map_->resolution();
  int n = 0;
  const std::vector<uint8_t> blob = map_->evict(pose, keep_xy_, keep_z_, &n);
  std::vector<MapStateCell> out;
  const char* why = "";
  if (liodom_dev::map_state_split(blob.data(), (int64_t)blob.size(), xy, z, res, &out, nullptr, &why) != LIODOM_OK)
    throw std::runtime_error(std::string("MapPager: evicted blob: ") + why);
  evicted += n;
  std::vector<MapStateCell> back;                  // evicted cells whose key is stored already
  for (MapStateCell& c : out) {
    if (index_.count(c.key)) { back.push_back(std::move(c)); continue; }
    store_.push_back(Cell{c.key, c.corner_leaf, std::move(c.xyzi)});
    index_[store_.back().key] = std::prev(store_.end());
  }
  if (!back.empty()) {                             // the device gets its cells back, the stored ones are re-observed into them
    std::vector<const MapStateCell*> ptrs;
    for (const MapStateCell& c : back) ptrs.push_back(&c);
    map_->mergeState(liodom_dev::map_state_join(xy, z, res, ptrs, 0));
    for (const MapStateCell& c : back) {
      auto it = index_.find(c.key);
      conflicts++;
      const std::vector<float> pts = std::move(it->second->xyzi);
      store_.erase(it->second);
      index_.erase(it);
      reobserve(pts);
    }
  }
  // the centre cell as liodom_map_prune / Map::getLocalMap compute it: the translation truncated to int first (map.cc:144-151)
  auto cell_key = [](double x, double size) { return (int32_t)(std::floor(x * (1.0 / size)) * size + size / 2.0); };
  const std::array<int32_t, 3> centre{{cell_key((double)(int)pose[3], xy), cell_key((double)(int)pose[7], xy), cell_key((double)(int)pose[11], z)}};
  std::vector<std::list<Cell>::iterator> want;
  for (auto it = store_.begin(); it != store_.end(); ++it)
    if (inBox(it->key, centre, load_xy_, load_z_)) want.push_back(it);
  if (want.empty()) return;
  std::vector<MapStateCell> cells(want.size());
  std::vector<const MapStateCell*> ptrs;
  for (size_t i = 0; i < want.size(); i++) {
    cells[i].key = want[i]->key; cells[i].corner_leaf = want[i]->corner_leaf; cells[i].xyzi = want[i]->xyzi;      // (a copy: a merge that fails leaves the store whole)
    ptrs.push_back(&cells[i]);
  }
  const std::vector<int32_t> taken = map_->mergeState(liodom_dev::map_state_join(xy, z, res, ptrs, 0));
  for (size_t i = 0; i < want.size(); i++) {
    index_.erase(want[i]->key);
    store_.erase(want[i]);
    if (taken[i]) { loaded++; continue; }
    conflicts++;
    reobserve(cells[i].xyzi);
  }
}
std::vector<uint8_t> MapPager::exportAll() {
  using liodom_dev::MapStateCell;
  const double xy = map_->xySize(), z = map_->zSize(), res = map_->resolution();
  const std::vector<uint8_t> dev = map_->exportState();
  std::vector<MapStateCell> cells;
  uint32_t status = 0;
  const char* why = "";
  if (liodom_dev::map_state_split(dev.data(), (int64_t)dev.size(), xy, z, res, &cells, &status, &why) != LIODOM_OK)
    throw std::runtime_error(std::string("MapPager: exported blob: ") + why);
  const size_t n_dev = cells.size();
  cells.resize(n_dev + store_.size());
  size_t i = n_dev;
  for (const Cell& c : store_) { cells[i].key = c.key; cells[i].corner_leaf = c.corner_leaf; cells[i].xyzi = c.xyzi; i++; }
  std::vector<const MapStateCell*> ptrs;
  for (const MapStateCell& c : cells) ptrs.push_back(&c);
  return liodom_dev::map_state_join(xy, z, res, ptrs, status);
}

int Map::numCells() {
  int n = 0;
  check(liodom_map_num_cells(m_, &n), "liodom_map_num_cells");
  return n;
}

void LaserOdometer::attachMapper(Map* map, const liodom_mapper_options_t& options) {
  check(liodom_attach_mapper_ex(eng_->handle(), 0, map ? map->handle() : nullptr, &options), "liodom_attach_mapper_ex");
}

void LaserOdometer::attachMapReader(Map* map, int cells_xy, int cells_z) {
  check(liodom_attach_map_reader(eng_->handle(), 0, map ? map->handle() : nullptr, cells_xy, cells_z), "liodom_attach_map_reader");
}

void LaserOdometer::seed(const Pose& pose) {
  const double p[7] = {pose.q[0], pose.q[1], pose.q[2], pose.q[3], pose.t[0], pose.t[1], pose.t[2]};
  check(liodom_seed_stream(eng_->handle(), 0, p), "liodom_seed_stream");
  // what publishOdom keeps on the host starts over, as after reset(); the seeded scan is no first frame of the reference's kind
  // (it solves), so the rate watchdog runs from it on
  prev_odom_ = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  prev_stamp_ = 0.0; published_ = false; init_ = true; last_scan_ = -1;
}

void LaserOdometer::setMapHits(int radius) { check(liodom_set_map_hits(eng_->handle(), 0, radius), "liodom_set_map_hits"); }

liodom_map_hit_t LaserOdometer::mapHit(int scan_index) {
  liodom_map_hit_t rec{};
  check(liodom_get_map_hit_log(eng_->handle(), 0, scan_index, 1, &rec), "liodom_get_map_hit_log");
  return rec;
}

std::vector<PointCloud> Map::getLocalBatch(const std::vector<std::array<double, 12>>& poses, int cells_xy, int cells_z) {
  const int n = (int)poses.size();
  std::vector<PointCloud> out((size_t)n);
  if (n == 0) return out;
  std::vector<double> T(12 * (size_t)n);
  for (int i = 0; i < n; i++) std::memcpy(&T[12 * (size_t)i], poses[(size_t)i].data(), sizeof(double) * 12);
  std::vector<int64_t> sizes((size_t)n, 0);
  // size query first (LIODOM_ERR_CAPACITY with the sizes filled in), then the copy
  const int rc = liodom_map_get_local_batch(m_, T.data(), n, cells_xy, cells_z, nullptr, 0, sizes.data());
  if (rc != LIODOM_ERR_CAPACITY) check(rc, "liodom_map_get_local_batch");
  const int64_t cap = *std::max_element(sizes.begin(), sizes.end());
  if (cap == 0) return out;
  std::vector<Point> buf((size_t)n * (size_t)cap);
  check(liodom_map_get_local_batch(m_, T.data(), n, cells_xy, cells_z, reinterpret_cast<float*>(buf.data()), cap, sizes.data()), "liodom_map_get_local_batch");
  for (int i = 0; i < n; i++) {
    out[(size_t)i].points.assign(buf.begin() + (std::ptrdiff_t)((size_t)i * (size_t)cap), buf.begin() + (std::ptrdiff_t)((size_t)i * (size_t)cap + (size_t)sizes[(size_t)i]));
    out[(size_t)i].width = (uint32_t)sizes[(size_t)i]; out[(size_t)i].height = 1;
  }
  return out;
}

std::vector<int32_t> Map::scorePoses(const PointCloud& edges, const std::vector<std::array<double, 12>>& poses, int radius) {
  const int n = (int)poses.size();
  std::vector<int32_t> hits(2 * (size_t)n, 0);
  std::vector<double> T(12 * (size_t)n);
  for (int i = 0; i < n; i++) std::memcpy(&T[12 * (size_t)i], poses[(size_t)i].data(), sizeof(double) * 12);
  check(liodom_map_score_poses(m_, reinterpret_cast<const float*>(edges.points.data()), (int)edges.points.size(), T.data(), n, radius, hits.data()),
        "liodom_map_score_poses");
  return hits;
}

liodom_pose_search_result_t Map::searchPose(const PointCloud& edges, const liodom_pose_search_t& search) {
  liodom_pose_search_result_t out{};
  check(liodom_map_search_pose(m_, reinterpret_cast<const float*>(edges.points.data()), (int)edges.points.size(), &search, &out, nullptr, nullptr),
        "liodom_map_search_pose");
  return out;
}

liodom_pose_search_result_t Map::searchPoseBnb(const PointCloud& edges, const liodom_pose_search_t& search, int batch, liodom_pose_search_stats_t* stats) {
  liodom_pose_search_result_t out{};
  liodom_pose_search_bnb_t opt;
  liodom_pose_search_bnb_default(&opt);
  if (batch) opt.batch = batch;
  check(liodom_map_search_pose_bnb(m_, reinterpret_cast<const float*>(edges.points.data()), (int)edges.points.size(), &search, &opt, &out, stats),
        "liodom_map_search_pose_bnb");
  return out;
}

std::vector<liodom_map_registration_t> Map::registerPoses(const PointCloud& edges, const std::vector<std::array<double, 7>>& poses,
                                                          const liodom_map_register_t* opt, std::vector<int32_t>* corr) {
  const int n = (int)poses.size(), n_edges = (int)edges.points.size();
  std::vector<double> p(7 * (size_t)std::max(n, 1));
  for (int i = 0; i < n; i++) std::copy(poses[(size_t)i].begin(), poses[(size_t)i].end(), p.begin() + 7 * (size_t)i);
  std::vector<liodom_map_registration_t> out((size_t)std::max(n, 1));
  if (corr) corr->assign(2 * (size_t)n * (size_t)n_edges, -1);
  check(liodom_map_register_poses(m_, reinterpret_cast<const float*>(edges.points.data()), n_edges, p.data(), n, opt, out.data(),
                                  corr && !corr->empty() ? corr->data() : nullptr),
        "liodom_map_register_poses");
  out.resize((size_t)n);
  return out;
}

void LaserOdometer::attachMapper(Map* map, int cells_xy, int cells_z) {
  check(liodom_attach_mapper(eng_->handle(), 0, map ? map->handle() : nullptr, cells_xy, cells_z), "liodom_attach_mapper");
}

static double wall_secs() {      // ros::Time::now().toSec() of the reference (wall clock unless /use_sim_time)
  return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
}

LaserOdometer::LaserOdometer(std::shared_ptr<Engine> e)
    : lmap_manager(e), eng_(e), params(Params::getInstance()), stats(Stats::getInstance()) {
  for (int i = 0; i < 5; i++) { in_freqs_[i] = 20.0; out_freqs_[i] = 20.0; }   // laser_odometry.cc:83-86 (100 / 5)
  last_in_time_secs_ = wall_secs();                                            // :89
  last_out_time_secs_ = last_in_time_secs_;                                    // :90
}

// laser_odometry.cc:239-256: running mean over five scans of the input rate (from the message stamps) and of the output
// rate (from the wall clock); a warning when the odometer keeps up with less than 80 % of the input.
void LaserOdometer::updateFrequencies(double in_stamp_secs, double now_secs) {
  mean_in_freq_ -= in_freqs_[num_freqs_];                                                   // :240
  in_freqs_[num_freqs_] = (1.0 / (in_stamp_secs - last_in_time_secs_)) / 5.0;               // :241
  mean_in_freq_ += in_freqs_[num_freqs_];                                                   // :242
  last_in_time_secs_ = in_stamp_secs;                                                       // :243
  mean_out_freq_ -= out_freqs_[num_freqs_];                                                 // :245
  out_freqs_[num_freqs_] = (1.0 / (now_secs - last_out_time_secs_)) / 5.0;                  // :246
  mean_out_freq_ += out_freqs_[num_freqs_];                                                 // :247
  last_out_time_secs_ = now_secs;                                                           // :248
  num_freqs_ = (num_freqs_ + 1) % 5;                                                        // :250-251
  if (mean_out_freq_ < mean_in_freq_ * 0.8) {                                               // :254-256 (ROS_WARN)
    freq_warnings_++;
    std::fprintf(stderr, "[ WARN] Output frequency too low: %2.2f (in: %2.2f)\n", mean_out_freq_, mean_in_freq_);
  }
}

Pose LaserOdometer::process(const PointCloud& feats, double stamp, liodom_step_info_t* info) {
  const auto start_t = Clock::now();
  double p[7];
  liodom_step_info_t local;
  check(liodom_odometry_step(eng_->handle(), 0, reinterpret_cast<const float*>(feats.points.data()),
                             (int)feats.size(), stamp, p, &local), "liodom_odometry_step");
  if (info) *info = local;
  last_scan_ = local.scan_index;
  Pose out;
  std::memcpy(out.q, p, sizeof(double) * 4); std::memcpy(out.t, p + 4, sizeof(double) * 3);
  const auto end_t = Clock::now();                                    // laser_odometry.cc:237
  if (init_) updateFrequencies(stamp, wall_secs());                   // :239-256 (the first frame takes the other branch, :108-136)
  init_ = true;                                                       // :124
  if (params->save_results_) {                                        // :259-263
    stats->addPose(out.matrix34());
    stats->addLaserOdometryTime(start_t, end_t);
    stats->stopFrame(end_t);
  }
  return out;
}

Pose LaserOdometer::process(const Features& feats, liodom_step_info_t* info) {
  if (feats.ticket.seq == 0u) return process(feats.edges, feats.stamp, info);
  const auto start_t = Clock::now();
  double p[7];
  liodom_step_info_t local;
  check(liodom_odometry_step_device(eng_->handle(), &feats.ticket, feats.stamp, p, &local), "liodom_odometry_step_device");
  if (info) *info = local;
  last_scan_ = local.scan_index;
  Pose out;
  std::memcpy(out.q, p, sizeof(double) * 4); std::memcpy(out.t, p + 4, sizeof(double) * 3);
  const auto end_t = Clock::now();                                    // laser_odometry.cc:237
  if (init_) updateFrequencies(feats.stamp, wall_secs());             // :239-256
  init_ = true;
  if (params->save_results_) {                                        // :259-263
    stats->addPose(out.matrix34());
    stats->addLaserOdometryTime(start_t, end_t);
    stats->stopFrame(end_t);
  }
  return out;
}

void LaserOdometer::operator()(std::atomic<bool>& running, std::vector<OdometryMsg>* published, std::vector<Pose>* poses) {
  SharedData* sdata = SharedData::getInstance();
  while (running) {                                                   // laser_odometry.cc:102
    Features feats;
    if (sdata->popFeatures(feats)) {                                  // :107
      const Pose p = process(feats);                                  // :108-235
      const OdometryMsg msg = publishOdom(feats.stamp, p);            // :265
      if (published) published->push_back(msg);
      if (poses) poses->push_back(p);
    }
    worker_pause(sdata);                                              // :270
  }
}

}  // namespace liodom

// ---- throughput of the two-thread binding, measured in C++ (bench.py's two_thread leg; liodom_replay threads=true) ----
// An extractor thread and an odometer thread drive ONE handle through the C-ABI exactly as the patched liodom_node would
// (INTEGRATION.md §2): liodom_extract_edges_device (+ liodom_wait_edges: the ~edges cloud) on one side, a queue of tickets,
// liodom_odometry_submit_device / liodom_odometry_collect on the other (depth 1: the next ticket, if it is already queued, is
// submitted before the previous pose is collected; depth 0: liodom_odometry_step_device).  No sleeps: both threads spin-yield.
// scans: count clouds of n points (packed XYZI) `stride_floats` apart in host memory — page-locked (liodom_pin_host_buffer)
// for asynchronous uploads.  The clock runs from the submission of scan `timed_from` to the collection of the last pose.
// extract(k, ticket): the extraction call of scan k (liodom_extract_edges_device or its polar form).
static int two_thread_replay(liodom_handle_t* h, int count, int timed_from, int fetch_edges, int depth, int edge_cap,
                             double* poses_out /*count x 7*/, double* seconds_out, int64_t* edges_total_out,
                             const std::function<int(int, liodom_edge_ticket_t*)>& extract) {
  if (!h || count <= 0 || !poses_out) return LIODOM_ERR_INVALID_ARG;
  std::mutex qm;
  std::queue<liodom_edge_ticket_t> q;
  std::atomic<int> rc_x{0}, rc_o{0};
  std::atomic<bool> abort_all{false};
  int64_t edges_total = 0;
  std::thread tx([&] {
    std::vector<float> ebuf((size_t)std::max(1, edge_cap) * 4);
    for (int k = 0; k < count && !abort_all; k++) {
      liodom_edge_ticket_t t;
      int rc;
      while ((rc = extract(k, &t)) == LIODOM_ERR_BUSY) {
        if (abort_all) return;
        std::this_thread::yield();
      }
      if (rc) { rc_x = rc; abort_all = true; return; }
      if (fetch_edges) {
        int ne = 0;
        rc = liodom_wait_edges(h, &t, ebuf.data(), nullptr, nullptr, nullptr, edge_cap, &ne);
        if (rc) { rc_x = rc; abort_all = true; return; }
        edges_total += ne;
      }
      std::lock_guard<std::mutex> lk(qm);
      q.push(t);
    }
  });
  std::chrono::steady_clock::time_point t0{}, t1{};
  std::thread to([&] {
    int submitted = 0, collected = 0;
    const int max_fly = depth ? 2 : 1;
    while (collected < count && !abort_all) {
      liodom_edge_ticket_t t;
      bool got = false;
      if (submitted < count && submitted - collected < max_fly) {
        std::lock_guard<std::mutex> lk(qm);
        if (!q.empty()) { t = q.front(); q.pop(); got = true; }
      }
      if (got) {                                     // a ticket is waiting: its odometry goes in behind the scan in flight
        if (submitted == timed_from) t0 = std::chrono::steady_clock::now();
        const int rc = liodom_odometry_submit_device(h, &t, 0.1 * submitted);
        if (rc) { rc_o = rc; abort_all = true; return; }
        submitted++;
      } else if (submitted > collected) {            // nothing (more) to submit: the oldest pose in flight is collected (and would be published)
        const int rc = liodom_odometry_collect(h, 0, poses_out + 7 * (size_t)collected, nullptr);
        if (rc) { rc_o = rc; abort_all = true; return; }
        collected++;
      } else {
        std::this_thread::yield();
      }
    }
    t1 = std::chrono::steady_clock::now();
  });
  tx.join();
  to.join();
  if (seconds_out) *seconds_out = std::chrono::duration<double>(t1 - t0).count();
  if (edges_total_out) *edges_total_out = edges_total;
  if (rc_x) return rc_x;
  return rc_o;
}
extern "C" int liodom_host_two_thread_replay(liodom_handle_t* h, const float* scans, int64_t stride_floats, int count, int64_t n,
                                             int height, int width, int timed_from, int fetch_edges, int depth, int edge_cap,
                                             double* poses_out /*count x 7*/, double* seconds_out, int64_t* edges_total_out) {
  if (!scans) return LIODOM_ERR_INVALID_ARG;
  return two_thread_replay(h, count, timed_from, fetch_edges, depth, edge_cap, poses_out, seconds_out, edges_total_out,
                           [&](int k, liodom_edge_ticket_t* t) { return liodom_extract_edges_device(h, 0, scans + (size_t)k * (size_t)stride_floats, n, height, width, t); });
}
// The same driver fed polar blobs (liodom_set_polar_geometry first): blob k at blobs + k * stride_bytes, page-locked for asynchronous
// uploads; same threads, same queue, same outputs.  What the patched liodom_node does when the driver hands it the sensor's packets.
extern "C" int liodom_host_two_thread_replay_polar(liodom_handle_t* h, const unsigned char* blobs, int64_t stride_bytes, int count,
                                                   int timed_from, int fetch_edges, int depth, int edge_cap,
                                                   double* poses_out /*count x 7*/, double* seconds_out, int64_t* edges_total_out) {
  if (!blobs) return LIODOM_ERR_INVALID_ARG;
  return two_thread_replay(h, count, timed_from, fetch_edges, depth, edge_cap, poses_out, seconds_out, edges_total_out,
                           [&](int k, liodom_edge_ticket_t* t) { return liodom_extract_edges_device_polar(h, 0, blobs + (size_t)k * (size_t)stride_bytes, t); });
}

namespace liodom {

// One scan through a fused call (liodom_process_scan or its polar form) and the bookkeeping around it.
Pose LaserOdometer::fusedScan(double stamp, liodom_step_info_t* info, const std::function<void(double*, liodom_step_info_t*)>& call) {
  const auto start_t = Clock::now();
  if (params->save_results_) stats->startFrame(start_t);              // liodom_node.cc:49-52
  double p[7];
  liodom_step_info_t local;
  call(p, &local);
  if (info) *info = local;
  last_scan_ = local.scan_index;
  Pose out;
  std::memcpy(out.q, p, sizeof(double) * 4); std::memcpy(out.t, p + 4, sizeof(double) * 3);
  if (init_) updateFrequencies(stamp, wall_secs());                   // laser_odometry.cc:239-256
  init_ = true;
  if (params->save_results_) {
    const auto end_t = Clock::now();
    stats->addNumOfFeats((size_t)local.n_edges);
    stats->addPose(out.matrix34());
    stats->addLaserOdometryTime(start_t, end_t);
    stats->stopFrame(end_t);
  }
  return out;
}

Pose LaserOdometer::processScan(const PointCloud& pc_in, double stamp, liodom_step_info_t* info) {
  return fusedScan(stamp, info, [&](double* p, liodom_step_info_t* local) {
    check(liodom_process_scan(eng_->handle(), 0, reinterpret_cast<const float*>(pc_in.points.data()),
                              (int64_t)pc_in.size(), (int)pc_in.height, (int)pc_in.width, stamp, p, local),
          "liodom_process_scan");
  });
}

Pose LaserOdometer::processScanPolar(const std::vector<uint8_t>& blob, double stamp, liodom_step_info_t* info) {
  return fusedScan(stamp, info, [&](double* p, liodom_step_info_t* local) {
    check(liodom_process_scan_polar(eng_->handle(), 0, blob.data(), stamp, p, local), "liodom_process_scan_polar");
  });
}

}  // namespace liodom
