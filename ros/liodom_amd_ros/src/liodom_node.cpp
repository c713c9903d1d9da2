// liodom_node — ROS 1 transport around the MI355X LiODOM path (SOURCE ONLY: never compiled in the
// build image, which has no ROS).  Same private-namespace topics and parameters as the reference
// node (src/liodom_node.cc:72-110, src/params.cc:37-110, src/laser_odometry.cc:395-446).
#include <memory>
#include <string>
#include <vector>

#include <geometry_msgs/TwistStamped.h>
#include <nav_msgs/Odometry.h>
#include <ros/ros.h>
#include <sensor_msgs/Imu.h>
#include <sensor_msgs/PointCloud2.h>
#include <tf/transform_broadcaster.h>
#include <tf/transform_listener.h>

#include "cloud_io.h"
#include "liodom_host.h"

// Polar path for an Ouster (-DLIODOM_WITH_OUSTER, needs ouster_ros + the ouster client library): the node subscribes to the
// driver's lidar PACKETS instead of its projected cloud, batches them into a LidarScan and hands the scan's ranges, signals and
// encoder ticks to the device as one blob — the projection to XYZ (the driver's cartesian() on a CPU core) and pcl::fromROSMsg
// run on the GPU (include/liodom_hip.h, "polar scans").
#ifdef LIODOM_WITH_OUSTER
#include <cmath>
#include <cstring>
#include <ouster/lidar_scan.h>
#include <ouster/types.h>
#include <ouster_ros/PacketMsg.h>
#endif

namespace {

struct Node {
  ros::NodeHandle nh{"~"};
  liodom::Params* params = liodom::Params::getInstance();
  std::shared_ptr<liodom::Engine> engine;
  std::unique_ptr<liodom::FeatureExtractor> extractor;
  std::unique_ptr<liodom::LaserOdometer> odometer;
  std::unique_ptr<liodom::Map> mapper;            // only with in_process_mapper
  ros::Publisher edges_pub, odom_pub, twist_pub;
  ros::Subscriber points_sub, map_sub, imu_sub;
  tf::TransformBroadcaster tf_broadcaster;
  tf::TransformListener tf_listener;
  bool have_laser_to_base = false;
  int max_points = 0, max_width = 0;

  // every parameter the reference reads, forwarded as name=value to the host mirror's readParams
  void read_params() {
    std::vector<std::string> kv;
    auto fwd_d = [&](const char* n, double d) { double v; nh.param(n, v, d); kv.push_back(std::string(n) + "=" + std::to_string(v)); };
    auto fwd_i = [&](const char* n, int d) { int v; nh.param(n, v, d); kv.push_back(std::string(n) + "=" + std::to_string(v)); };
    auto fwd_b = [&](const char* n, bool d) { bool v; nh.param(n, v, d); kv.push_back(std::string(n) + (v ? "=true" : "=false")); };
    auto fwd_s = [&](const char* n, const char* d) { std::string v; nh.param<std::string>(n, v, d); kv.push_back(std::string(n) + "=" + v); };
    fwd_d("min_range", 3.0); fwd_d("max_range", 75.0);
    fwd_i("lidar_type", 0); fwd_i("scan_lines", 64); fwd_i("scan_regions", 8); fwd_i("edges_per_region", 10);
    fwd_b("save_results", false); fwd_s("save_results_dir", "~/");
    fwd_s("fixed_frame", "odom"); fwd_s("base_frame", "base_link"); fwd_s("laser_frame", "");
    fwd_i("prev_frames", 5);
    fwd_b("use_imu", false); fwd_b("filter_local_map", false); fwd_b("mapping", false); fwd_b("publish_tf", true);
    params->readParams(kv);
    nh.param("max_points", max_points, 300000);          // capacities: no counterpart in the reference
    nh.param("max_width", max_width, 4096);
  }

  void lookup_laser_to_base(const std_msgs::Header& header) {
    // laser_odometry.cc:110-119: base_frame <- laser frame, once, at the first cloud
    const std::string laser = params->laser_frame_.empty() ? header.frame_id : params->laser_frame_;
    tf::StampedTransform t;
    try {
      tf_listener.waitForTransform(laser, params->base_frame_, ros::Time(0), ros::Duration(5.0));
      tf_listener.lookupTransform(laser, params->base_frame_, ros::Time(0), t);
    } catch (const tf::TransformException& ex) {
      ROS_ERROR("%s", ex.what());
      return;
    }
    const tf::Matrix3x3& R = t.getBasis();
    const tf::Vector3& o = t.getOrigin();
    std::array<double, 12> T{{R[0][0], R[0][1], R[0][2], o.x(), R[1][0], R[1][1], R[1][2], o.y(), R[2][0], R[2][1], R[2][2], o.z()}};
    odometer->setLaserToBase(T);
    have_laser_to_base = true;
  }

  void points_cb(const sensor_msgs::PointCloud2ConstPtr& msg) {
    liodom::PointCloud cloud;
    if (!liodom_ros::from_msg(*msg, cloud)) { ROS_ERROR_ONCE("~points needs float32 x, y, z fields"); return; }
    if (params->lidar_type_ != 1) { cloud.height = 1; cloud.width = (uint32_t)cloud.size(); }
    if (!have_laser_to_base) lookup_laser_to_base(msg->header);
    liodom_step_info_t info;
    liodom::Pose pose;
    try {
      pose = odometer->processScan(cloud, msg->header.stamp.toSec(), &info);
    } catch (const std::exception& e) {
      ROS_ERROR("%s", e.what());
      return;
    }
    ROS_DEBUG("Extracted edges: %d, correct matchings: %d", info.n_edges, info.matches[1]);
    publish_edges(msg->header);
    publish(msg->header, odometer->publishOdom(msg->header.stamp.toSec(), pose));
  }

  // ~edges of the scan that just went through the odometer (feature_extractor.cc:70-75); liodom_mapping subscribes to it
  void publish_edges(const std_msgs::Header& header) {
    if (edges_pub.getNumSubscribers() == 0) return;
    liodom::PointCloud edges;
    extractor->lastEdges(edges);
    sensor_msgs::PointCloud2 out;
    liodom_ros::to_msg(edges, header, out);
    edges_pub.publish(out);
  }

#ifdef LIODOM_WITH_OUSTER
  ros::Subscriber packets_sub;
  ouster::sensor::sensor_info ouster_info;
  std::unique_ptr<ouster::ScanBatcher> batcher;
  std::unique_ptr<ouster::LidarScan> ls;
  liodom_polar_layout_t lay;
  std::vector<uint8_t> blob;

  // ~ouster_metadata: the sensor's metadata file (beam angles, beam origin, columns per frame)
  void setup_ouster() {
    std::string meta;
    nh.param<std::string>("ouster_metadata", meta, "");
    ouster_info = ouster::sensor::metadata_from_json(meta);
    const int H = (int)ouster_info.format.pixels_per_column, W = (int)ouster_info.format.columns_per_frame;
    const int T = 90112;                                                     // encoder counts per revolution, clockwise
    const double rad = M_PI / 180.0;
    std::vector<double> alt, baz, enc;
    for (int r = 0; r < H; r++) { alt.push_back(ouster_info.beam_altitude_angles[r] * rad); baz.push_back(-ouster_info.beam_azimuth_angles[r] * rad); }
    for (int t = 0; t < T; t++) enc.push_back(-2.0 * M_PI * t / T);
    const liodom::PolarGeometry g = liodom::PolarGeometry::fromAngles(H, W, alt, baz, enc, 32, 16, 0.001f,
                                                                      (float)(ouster_info.lidar_origin_to_beam_origin_mm * 0.001));
    engine->setPolarGeometry(g);
    lay = g.layout();
    blob.assign(g.blobBytes(), 0);
    batcher.reset(new ouster::ScanBatcher(ouster_info));
    ls.reset(new ouster::LidarScan(W, H, ouster_info.format.udp_profile_lidar));
    packets_sub = nh.subscribe("lidar_packets", 2048, &Node::ouster_cb, this);
  }

  void ouster_cb(const ouster_ros::PacketMsg::ConstPtr& pm) {
    if (!(*batcher)(pm->buf.data(), *ls)) return;                            // scan not complete yet
    const int H = (int)ls->h, W = (int)ls->w;
    uint32_t* tick = reinterpret_cast<uint32_t*>(blob.data() + lay.tick_offset);
    uint32_t* range = reinterpret_cast<uint32_t*>(blob.data() + lay.range_offset);
    uint16_t* signal = reinterpret_cast<uint16_t*>(blob.data() + lay.intensity_offset);
    // a column the sensor did not deliver keeps status 0: its tick leaves the table, the column becomes NaN points
    for (int c = 0; c < W; c++) tick[c] = (ls->status()(c) & 1) ? (uint32_t)(((uint64_t)ls->measurement_id()(c) * 90112u) / (uint32_t)W) : 0xFFFFFFFFu;
    const auto rg = ls->field<uint32_t>(ouster::sensor::ChanField::RANGE);   // [H x W], row-major, staggered: beam_azimuth is in the tables
    const auto sg = ls->field<uint16_t>(ouster::sensor::ChanField::SIGNAL);
    std::memcpy(range, rg.data(), sizeof(uint32_t) * (size_t)H * W);
    std::memcpy(signal, sg.data(), sizeof(uint16_t) * (size_t)H * W);
    // the scan's stamp is its first delivered column's, on the sensor's clock (ouster_ros: timestamp_mode TIME_FROM_SENSOR-style
    // stamps; a node that wants ROS time adds its own offset here, as ouster_ros does)
    std_msgs::Header header;
    header.stamp = ros::Time::now();
    for (int c = 0; c < W; c++) if (ls->status()(c) & 1) { header.stamp.fromNSec(ls->timestamp()(c)); break; }
    header.frame_id = params->laser_frame_;
    if (!have_laser_to_base) lookup_laser_to_base(header);
    liodom_step_info_t info;
    liodom::Pose pose;
    try {
      pose = odometer->processScanPolar(blob, header.stamp.toSec(), &info);
    } catch (const std::exception& e) {
      ROS_ERROR("%s", e.what());
      return;
    }
    publish_edges(header);
    publish(header, odometer->publishOdom(header.stamp.toSec(), pose));
  }
#endif

  void publish(const std_msgs::Header& header, const liodom::OdometryMsg& m) {   // laser_odometry.cc:395-446
    nav_msgs::Odometry odom;
    odom.header.frame_id = m.frame_id; odom.child_frame_id = m.child_frame_id; odom.header.stamp = header.stamp;
    odom.pose.pose.orientation.x = m.orientation[0]; odom.pose.pose.orientation.y = m.orientation[1];
    odom.pose.pose.orientation.z = m.orientation[2]; odom.pose.pose.orientation.w = m.orientation[3];
    odom.pose.pose.position.x = m.position[0]; odom.pose.pose.position.y = m.position[1]; odom.pose.pose.position.z = m.position[2];
    odom.twist.twist.linear.x = m.linear[0]; odom.twist.twist.linear.y = m.linear[1]; odom.twist.twist.linear.z = m.linear[2];
    odom.twist.twist.angular.x = m.angular[0]; odom.twist.twist.angular.y = m.angular[1]; odom.twist.twist.angular.z = m.angular[2];
    // engine created with pose covariance: the scan's covariance where it is defined (flags == LIODOM_COV_VALID), else the
    // reference's all-zero covariance
    if (m.has_covariance && m.covariance_flags == LIODOM_COV_VALID)
      for (int i = 0; i < 36; i++) odom.pose.covariance[i] = m.pose_covariance[i];
    odom_pub.publish(odom);
    geometry_msgs::TwistStamped tw;
    tw.header.frame_id = m.child_frame_id; tw.header.stamp = header.stamp; tw.twist = odom.twist.twist;
    twist_pub.publish(tw);
    if (params->publish_tf_) {
      tf::Transform t;
      t.setOrigin(tf::Vector3(m.position[0], m.position[1], m.position[2]));
      t.setRotation(tf::Quaternion(m.orientation[0], m.orientation[1], m.orientation[2], m.orientation[3]));
      tf_broadcaster.sendTransform(tf::StampedTransform(t, header.stamp, m.frame_id, m.child_frame_id));
    }
  }

  void map_cb(const sensor_msgs::PointCloud2ConstPtr& msg) {      // mapClb, liodom_node.cc:57-64
    liodom::PointCloud map;
    if (liodom_ros::from_msg(*msg, map)) odometer->setLocalMap(map);
  }
  void imu_cb(const sensor_msgs::ImuConstPtr& msg) {              // imuClb, liodom_node.cc:66-70
    const double q[4] = {msg->orientation.x, msg->orientation.y, msg->orientation.z, msg->orientation.w};
    odometer->setLastIMUOri(q);
  }

  int run() {
    read_params();
    try {
      engine = std::make_shared<liodom::Engine>(*params, 0, max_points, max_width);
      extractor.reset(new liodom::FeatureExtractor(engine));
      odometer.reset(new liodom::LaserOdometer(engine));
      bool in_process = false;
      nh.param("in_process_mapper", in_process, false);
      if (params->mapping_ && in_process) {
        double xy, z, res;
        liodom_mapper_options_t mo;
        liodom_mapper_options_default(&mo);
        nh.param("voxel_xysize", xy, 40.0); nh.param("voxel_zsize", z, 50.0); nh.param("resolution", res, 0.4);
        nh.param("cells_xy", mo.cells_xy, 2); nh.param("cells_z", mo.cells_z, 1);
        // ~mapper_lag 1: the map takes a frame when it leaves the sliding window (the mode that solves; 0 replays the reference's
        // loop, whose poses are the prediction); ~map_prune_period n > 0: the map is pruned to ~map_keep_xy / ~map_keep_z cells
        // around the pose every n-th scan
        nh.param("mapper_lag", mo.lag, 0); nh.param("map_prune_period", mo.prune_period, 0);
        nh.param("map_keep_xy", mo.keep_cells_xy, 0); nh.param("map_keep_z", mo.keep_cells_z, 0);
        mapper.reset(new liodom::Map(xy, z, res));
        odometer->attachMapper(mapper.get(), mo);
      }
    } catch (const std::exception& e) {
      ROS_FATAL("%s", e.what());
      return 1;
    }
    edges_pub = nh.advertise<sensor_msgs::PointCloud2>("edges", 10);
    odom_pub = nh.advertise<nav_msgs::Odometry>("odom", 10);
    twist_pub = nh.advertise<geometry_msgs::TwistStamped>("twist", 10);
    bool polar = false;
    nh.param("polar_input", polar, false);                 // true: ~lidar_packets of an Ouster instead of ~points
#ifdef LIODOM_WITH_OUSTER
    if (polar) {
      try {                                                // a bad ~ouster_metadata or a geometry the handle refuses
        setup_ouster();
      } catch (const std::exception& e) {
        ROS_FATAL("polar_input: %s", e.what());
        return 1;
      }
    }
#else
    if (polar) { ROS_FATAL("polar_input needs a build with LIODOM_WITH_OUSTER"); return 1; }
#endif
    if (!polar) points_sub = nh.subscribe("points", 1, &Node::points_cb, this);
    if (params->mapping_ && !mapper) map_sub = nh.subscribe("map", 1, &Node::map_cb, this);
    if (params->use_imu_) imu_sub = nh.subscribe("imu", 1, &Node::imu_cb, this);
    ros::spin();
    if (params->save_results_) liodom::Stats::getInstance()->writeResults(params->results_dir_);   // liodom_node.cc:112-116
    if (mapper) odometer->attachMapper(nullptr);
    return 0;
  }
};

}  // namespace

int main(int argc, char** argv) {
  ros::init(argc, argv, "liodom");
  Node node;
  return node.run();
}
