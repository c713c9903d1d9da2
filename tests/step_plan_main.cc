// Driver of tests/test_step_plan.py: the plan of a scan's launches (liodom_amd/csrc/step_plan.h) without a device.  Standard input
// is a sequence of blocks: "handle <case>" (tests/plan_case.h) plans a handle and starts over with a fresh StepState, then every
// line is one request of an entry point, as tests/step_scenarios.py writes them (its requests() describes them), plus
//   r                       liodom_reset: StepState::reset, the scan counts start over
//   set key=value ...       ov_seq, lb_tag, chain_count (state), alone, ov_suppress, reader (the request's surroundings)
// The driver models only what the entry points add around the plan functions: the scan counts, the sequence numbers of
// enqueue_pipeline_odometry, the verdict noted by wait_pose.  Output, per request: one line per planned entry,
//   L <instance> <queue> gx gy block lds scope bucket pass seq_k done_target scan_no nA with_pass with_fix alloc tiles lb_tag wait_edges signal_odo
//   O ev_ov | ev_ch | map_block <profiling scopes it opens>
// then "S <the state>".  "names" prints every instance name.  The driver fails (status 3) if a plan comes within 8 entries of
// the list's capacity.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "plan_case.h"
#include "step_plan.h"

using namespace liodom_dev;

static std::string instance_name(StepKernel k, bool list) {
  struct Row { const char* base; const char* args; bool rows; };      // args: the template arguments in front of the list flag
  static const Row rows[SK_KERNELS] = {
      {"k_row_compact", "", true}, {"k_ring_split_lb", "", true}, {"k_ring_split_fix", "", true}, {"k_ring_split", "", true},
      {"k_classify", "", true}, {"k_ring_scatter", "", true}, {"k_ring_extract", "256, 16", true}, {"k_ring_extract", "256, 24", true},
      {"k_ring_extract", "1024, 16", true}, {"k_ring_extract", "1024, 24", true}, {"k_compact_edges", "", true},
      {"k_imu_override", "", true}, {"k_window_stash", "", true}, {"k_knn", "256, false, true, false", false}, {"k_chain_redo0", "256", false},
      {"k_lm_solve", "0, true, false", false}, {"k_lm_solve", "1, true, false", false}, {"k_ov_gate", "", false},
      {"k_knn", "256, true, false, false", false}, {"k_knn_redo", "256", false}, {"k_rebuild_alloc", "false", false},
      {"k_rebuild_fin", "", false}, {"k_pose_cov", "false", false}, {"k_pose_cov", "", true}, {"k_knn8", "0", true}, {"k_knn8", "1", true}, {"k_knn8_exact", "", true}, {"k_line_gate", "", true},
      {"k_knn", "128, false, false", true}, {"k_knn", "256, false, false", true}, {"k_lm_solve", "0, false", true}, {"k_lm_solve", "1, false", true},
      {"k_hash_append", "", true}, {"k_hash_build", "", true}, {"k_window_insert", "", true}, {"k_hash_alloc", "", true}, {"k_hash_scatter", "", true},
      {"k_voxel_bbox", "", true}, {"k_voxel_insert", "", true}, {"k_voxel_alloc", "", true}, {"k_voxel_scatter", "", true},
      {"k_voxel_centroid", "", true}, {"k_filt_insert", "", true}, {"k_filt_alloc", "", true}, {"k_filt_scatter", "", true}};
  const Row& r = rows[k];
  std::string a = r.args;
  if (r.rows) a += std::string(a.empty() ? "" : ", ") + (list ? "true" : "false");
  return a.empty() ? std::string(r.base) : std::string(r.base) + "<" + a + ">";
}

struct Model {
  HandlePlan p;
  StepState st;
  ExtractState xs;
  std::vector<int> scans;
  unsigned int odo_seq = 0;
  bool profiling = false, ov_suppress = false, alone = true, mapper = false, lagged = false, reader = false;
  int max_width = 0;
};

static int print_plan(const Model& m, const StepPlan& plan, const char* qx, const StepRequest* rq) {
  for (int i = 0; i < plan.n; i++) {
    const StepLaunch& l = plan.e[i];
    if (l.k == SO_EV_OV) { std::printf("O ev_ov\n"); continue; }
    if (l.k == SO_EV_CH) { std::printf("O ev_ch\n"); continue; }
    if (l.k == SO_MAP_BLOCK) {
      int scopes = m.reader ? 1 : 0;
      for (int j = 0; rq && j < rq->count; j++) scopes += (m.mapper && rq->stream_at(j) == 0) ? 1 : 0;
      std::printf("O map_block %d\n", m.profiling ? scopes : 0);
      continue;
    }
    std::printf("L %s | %s %d %d %d %zu %d %d %d %u %u %d %d %d %d %d %d %u %u %u\n", instance_name(l.k, l.list).c_str(),
                l.q == SQ_ODO ? "o" : (l.q == SQ_K ? "k" : qx), l.gx, l.gy, l.block, l.lds, (int)l.scope, (int)l.bucket, l.pass, l.seq_k,
                l.done_target, l.scan_no, l.nA, l.with_pass, l.with_fix, l.alloc, l.tiles, l.lb_tag, l.wait_edges, l.signal_odo);
  }
  std::printf("S ov_warm=%d ov_prev=%d ov_seq=%u chain_prev=%d chain_count=%u fix=%d chain_used=%d lb_tag=%u hb=", m.st.ov_warm, m.st.ov_prev,
              m.st.ov_seq, m.st.chain_prev, m.st.chain_count, m.st.chain_fix_pending, m.st.chain_used, m.xs.lb_tag);
  for (size_t s = 0; s < m.st.hb_since.size(); s++) std::printf("%s%d", s ? "," : "", m.st.hb_since[s]);
  std::printf("\n");
  if (plan.overflow || plan.n + 8 > kStepPlanCap) { std::printf("plan of %d entries: too close to the capacity of %d\n", plan.n, kStepPlanCap); return 3; }
  return 0;
}

int main() {
  std::string line;
  Model m;
  bool have = false;
  while (std::getline(std::cin, line)) {
    std::istringstream words(line);
    std::string kind, w;
    words >> kind;
    if (kind == "names") {
      for (int k = 0; k < SK_KERNELS; k++) for (int l = 0; l < 2; l++) std::printf("%s\n", instance_name((StepKernel)k, l != 0).c_str());
      continue;
    }
    if (kind == "handle") {
      std::string rest;
      std::getline(words, rest);
      const PlanCase c = read_plan_case(rest);
      if (!c.bad.empty()) { std::printf("bad-case %s\n", c.bad.c_str()); return 2; }
      const char* why = "";
      m = Model();
      if (plan_handle(&c.prm, &c.cfg, c.caps, c.env, &m.p, &why) != LIODOM_OK) { std::printf("refused %s\n", why); return 2; }
      if (c.then_safe) plan_enter_safe_mode(&m.p);
      m.st.bind(m.p.n_streams);
      m.scans.assign((size_t)m.p.n_streams, 0);
      m.max_width = c.cfg.max_width;
      have = true;
      char buf[2048];
      plan_format_modes(m.p, ModesRuntime(), buf, (int)sizeof(buf));
      std::printf("H %s lockstep=%d lds_hash_build=%d use_flags=%d ov_ok=%d chain_ok=%d edge_cap=%d prev_frames=%d knn8_grid=%d map_cap=%d pose_covariance=%d\n", buf,
                  m.p.lockstep, m.p.lds_hash_build, m.p.use_flags, m.p.ov_ok, m.p.chain_ok, m.p.edge_cap, m.p.prev_frames, m.p.knn8_grid, m.p.map_cap, m.p.pose_covariance);
      continue;
    }
    if (!have) { std::printf("no handle\n"); return 2; }
    long long s0 = 0, count = 1, n = 0, width = 0, pipe = 0, lag = 0, confirmed = 0;
    std::string q = "o";
    std::vector<int32_t> list;
    while (words >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos) { std::printf("bad-word %s\n", w.c_str()); return 2; }
      const std::string k = w.substr(0, eq), val = w.substr(eq + 1);
      const long long x = std::atoll(val.c_str());
      if (k == "q") q = val;
      else if (k == "s0") s0 = x;
      else if (k == "count") count = x;
      else if (k == "n") n = x;
      else if (k == "width") width = x;
      else if (k == "pipe") pipe = x;
      else if (k == "lag") lag = x;
      else if (k == "confirmed") confirmed = x;
      else if (k == "lagged") m.lagged = x != 0;
      else if (k == "list") { std::istringstream ls(val); std::string t; while (std::getline(ls, t, ',')) list.push_back((int32_t)std::atoi(t.c_str())); }
      else if (k == "ov_seq") m.st.ov_seq = (unsigned int)std::strtoul(val.c_str(), nullptr, 10);
      else if (k == "lb_tag") m.xs.lb_tag = (unsigned int)std::strtoul(val.c_str(), nullptr, 10);
      else if (k == "chain_count") m.st.chain_count = (unsigned int)std::strtoul(val.c_str(), nullptr, 10);
      else if (k == "alone") m.alone = x != 0;
      else if (k == "ov_suppress") m.ov_suppress = x != 0;
      else if (k == "reader") m.reader = x != 0;
      else { std::printf("bad-word %s\n", w.c_str()); return 2; }
    }
    StepPlan plan;
    int rc = 0;
    if (kind == "x") {
      ExtractRequest rq;
      rq.count = (int)count; rq.list = s0 < 0; rq.n = (int)n; rq.width = (int)width; rq.max_width = m.max_width;
      plan_extract_step(m.p, &m.xs, rq, &plan);
      rc = print_plan(m, plan, q.c_str(), nullptr);
    } else if (kind == "o") {
      StepRequest rq;
      rq.s0 = (int)s0; rq.count = (int)count; rq.list = list.empty() ? nullptr : list.data();
      if (pipe && m.p.use_flags) {      // enqueue_pipeline_odometry: the flags travel in the first kNN launch unless a gate launch polls
        const unsigned int seq = ++m.odo_seq == 0 ? ++m.odo_seq : m.odo_seq;
        if (!m.p.flag_gate) { rq.wait_edges = seq; rq.signal_odo = seq - 1u; }
      }
      rq.profiling = m.profiling; rq.ov_suppress = m.ov_suppress; rq.alone = m.alone;
      rq.scans_enqueued = count > 0 ? m.scans[(size_t)rq.stream_at(0)] : 0;
      for (int i = 0; i < rq.count; i++) rq.lagged = rq.lagged || (m.mapper && m.lagged && rq.stream_at(i) == 0);
      plan_odometry_step(m.p, &m.st, rq, &plan);
      rc = print_plan(m, plan, "x", &rq);
      for (int i = 0; i < rq.count; i++) m.scans[(size_t)rq.stream_at(i)]++;
    } else if (kind == "f") {
      plan_chain_flush(m.p, &m.st, m.scans[0], &plan);
      rc = print_plan(m, plan, "x", nullptr);
    } else if (kind == "c") {
      m.st.verdict_scan = m.scans[0] - (int)lag; m.st.verdict_confirmed = confirmed != 0;
    } else if (kind == "p") {
      m.profiling = true;
    } else if (kind == "m") {
      m.mapper = true;
    } else if (kind == "r") {
      m.st.reset(); m.odo_seq = 0;
      std::fill(m.scans.begin(), m.scans.end(), 0);
    } else if (kind != "set") {
      std::printf("bad-request %s\n", kind.c_str()); return 2;
    }
    if (rc) return rc;
  }
  return 0;
}
