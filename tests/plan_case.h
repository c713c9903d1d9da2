// Shared by the drivers of tests/test_handle_plan.py and tests/test_step_plan.py: one handle as a line of key=value words,
//   scan_lines ... mapping, min_range, max_range   liodom_params_t (local_map_size is the window)
//   n_streams ... pose_covariance                   liodom_config_t
//   cus, wgs_per_cu, instrumented                   HandleCaps
//   LIODOM_* and other upper-case names             environment switches, set for this case only and read by read_handle_env
//   then_safe=1                                     plan_enter_safe_mode on the finished plan (a timeout's liodom_reset)
#pragma once
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "handle_plan.h"

struct PlanCase {
  liodom_params_t prm;
  liodom_config_t cfg;
  liodom_dev::HandleCaps caps;
  liodom_dev::HandleEnv env;
  bool then_safe = false;
  std::string bad;      // the word that was not understood, if any
};

inline PlanCase read_plan_case(const std::string& line) {
  using namespace liodom_dev;
  PlanCase c;
  liodom_params_t& prm = c.prm;
  liodom_config_t& cfg = c.cfg;
  HandleCaps& caps = c.caps;
  bool& then_safe = c.then_safe;
  std::memset(&prm, 0, sizeof(prm));
  std::memset(&cfg, 0, sizeof(cfg));
  prm.min_range = 3.0; prm.max_range = 75.0; prm.scan_lines = 64; prm.scan_regions = 8; prm.edges_per_region = 10; prm.local_map_size = 5;
  cfg.n_streams = 1; cfg.max_points = 64 * 1800; cfg.max_width = 1800; cfg.pose_log_capacity = 1024; cfg.pose_rotation_mode = 1;
  std::vector<std::string> switches;
  std::istringstream words(line);
  std::string w;
  while (words >> w) {
    const size_t eq = w.find('=');
    if (eq == std::string::npos) { c.bad = w; break; }
    const std::string k = w.substr(0, eq), val = w.substr(eq + 1);
    const long long n = std::atoll(val.c_str());
    if (k[0] >= 'A' && k[0] <= 'Z') { setenv(k.c_str(), val.c_str(), 1); switches.push_back(k); }
    else if (k == "min_range") prm.min_range = std::atof(val.c_str());
    else if (k == "max_range") prm.max_range = std::atof(val.c_str());
    else if (k == "lidar_type") prm.lidar_type = (int32_t)n;
    else if (k == "scan_lines") prm.scan_lines = (int32_t)n;
    else if (k == "scan_regions") prm.scan_regions = (int32_t)n;
    else if (k == "edges_per_region") prm.edges_per_region = (int32_t)n;
    else if (k == "local_map_size") prm.local_map_size = (uint64_t)n;
    else if (k == "use_imu") prm.use_imu = (int32_t)n;
    else if (k == "filter_local_map") prm.filter_local_map = (int32_t)n;
    else if (k == "mapping") prm.mapping = (int32_t)n;
    else if (k == "n_streams") cfg.n_streams = (int32_t)n;
    else if (k == "max_points") cfg.max_points = (int32_t)n;
    else if (k == "max_width") cfg.max_width = (int32_t)n;
    else if (k == "pose_log_capacity") cfg.pose_log_capacity = (int32_t)n;
    else if (k == "debug_buffers") cfg.debug_buffers = (int32_t)n;
    else if (k == "lm_workgroups") cfg.lm_workgroups = (int32_t)n;
    else if (k == "recv_capacity") cfg.recv_capacity = (int32_t)n;
    else if (k == "pose_rotation_mode") cfg.pose_rotation_mode = (int32_t)n;
    else if (k == "pose_covariance") cfg.pose_covariance = (int32_t)n;
    else if (k == "cus") caps.cus = (int)n;
    else if (k == "wgs_per_cu") caps.ring_split_wgs_per_cu = (int)n;
    else if (k == "instrumented") caps.instrumented = n != 0;
    else if (k == "then_safe") then_safe = n != 0;
    else { c.bad = w; break; }
  }
  c.env = read_handle_env();
  for (const std::string& k : switches) unsetenv(k.c_str());
  return c;
}
