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
#include "plan_case.h"

using namespace liodom_dev;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    const PlanCase c = read_plan_case(line);
    if (!c.bad.empty()) { std::printf("bad-case %s\n", c.bad.c_str()); return 2; }
    const liodom_params_t& prm = c.prm;
    const liodom_config_t& cfg = c.cfg;
    const HandleCaps& caps = c.caps;
    const HandleEnv& env = c.env;
    const bool then_safe = c.then_safe;
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
