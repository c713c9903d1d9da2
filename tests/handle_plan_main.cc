// Driver of tests/test_handle_plan.py: plan_handle (liodom_amd/csrc/handle_plan.h) without a device.  Every line of standard input
// is one case, words of the form key=value:
//   scan_lines ... mapping, min_range, max_range   liodom_params_t (local_map_size is the window)
//   n_streams ... pose_covariance                   liodom_config_t
//   cus, wgs_per_cu, instrumented                   HandleCaps
//   LIODOM_* and other upper-case names             environment switches, set for this case only and read by read_handle_env
//   then_safe=1                                     plan_enter_safe_mode on the finished plan (a timeout's liodom_reset)
// and gives one line: "plan <the text of liodom_get_modes, no scan processed> || <what that text does not carry>" or
// "refused <code> <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "handle_plan.h"

using namespace liodom_dev;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    liodom_params_t prm;
    liodom_config_t cfg;
    std::memset(&prm, 0, sizeof(prm));
    std::memset(&cfg, 0, sizeof(cfg));
    prm.min_range = 3.0; prm.max_range = 75.0; prm.scan_lines = 64; prm.scan_regions = 8; prm.edges_per_region = 10; prm.local_map_size = 5;
    cfg.n_streams = 1; cfg.max_points = 64 * 1800; cfg.max_width = 1800; cfg.pose_log_capacity = 1024; cfg.pose_rotation_mode = 1;
    HandleCaps caps;
    bool then_safe = false;
    std::vector<std::string> switches;
    std::istringstream words(line);
    std::string w;
    bool bad = false;
    while (words >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) { bad = true; break; }
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
      else { bad = true; break; }
    }
    if (bad) { std::printf("bad-case %s\n", w.c_str()); return 2; }
    const HandleEnv env = read_handle_env();
    for (const std::string& k : switches) unsetenv(k.c_str());
    HandlePlan p;
    const char* why = "";
    const int rc = plan_handle(&prm, &cfg, caps, env, &p, &why);
    if (rc != LIODOM_OK) { std::printf("refused %d %s\n", rc, why); continue; }
    if (then_safe) plan_enter_safe_mode(&p);
    char buf[2048];
    plan_format_modes(p, ModesRuntime(), buf, (int)sizeof(buf));
    std::printf("plan %s || lockstep=%d lds_hash_build=%d use_flags=%d flag_gate_raw=%d ov_ok=%d chain_ok=%d knn8_grid=%d ring_split_wgs=%d "
                "map_rows=%d knn_save=%d pose_covariance=%d wait_ticks=%llu ring_lds_bytes=%zu slots_per_ring=%d edge_cap=%d map_cap=%d "
                "used_cap=%d ovf_base=%d recv_cap=%d ring_id_stride=%zu tile_cap=%d split_pad=%d lb_hpad=%d ring_pitch=%d ring_stride=%zu "
                "mask_stride=%d lds_cells_max=%d hb_slack_min=%d hb_new_room=%d spec_theta=%.6g spec_backoff=%d prev_frames=%d pose_log_cap=%d "
                "use_imu=%d ring_cap=%d max_points=%d\n",
                buf, p.lockstep, p.lds_hash_build, p.use_flags, p.flag_gate, p.ov_ok, p.chain_ok, p.knn8_grid, p.ring_split_max_wgs,
                p.map_rows, p.knn_save, p.pose_covariance, p.wait_ticks, p.ring_lds_bytes, p.slots_per_ring, p.edge_cap, p.map_cap,
                p.used_cap, p.ovf_base, p.recv_cap, p.ring_id_stride, p.tile_cap, p.split_pad, p.lb_hpad, p.ring_pitch, p.ring_stride,
                p.mask_stride, p.lds_cells_max, p.hb_slack_min, p.hb_new_room, p.spec_theta, p.spec_backoff, p.prev_frames, p.pose_log_cap,
                p.use_imu, p.ring_cap, p.max_points);
  }
  return 0;
}
