// tests/hostcheck.cc — compiles the product's arithmetic header (liodom_amd/csrc/liodom_math.h)
// for the host so that CPU tests can compare its leaf functions with the oracle without a GPU.
// Test tooling only: the shipped path runs these functions inside HIP kernels.
#include <cstring>
#include <vector>

#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

extern "C" {

int hc_velodyne_ring(double x, double y, double z, double min_r, double max_r, int lines) {
  double d;
  if (!valid_point(x, y, z, min_r, max_r, &d)) return -2;
  return velodyne_ring(z, d, lines);
}
double hc_curvature(const float* px, const float* py, const float* pz, int j) { return curvature(px, py, pz, j); }
void hc_eig3(const double* a, double* ev) { eig3_sym(a, ev); }
int hc_line_gate(const float* nx, const float* ny, const float* nz) { return line_gate(nx, ny, nz) ? 1 : 0; }
void hc_transform(const double* T, const float* in, int n, float* out) {
  for (int i = 0; i < n; i++) {
    transform_point(T, in[4 * i], in[4 * i + 1], in[4 * i + 2], &out[4 * i], &out[4 * i + 1], &out[4 * i + 2]);
    out[4 * i + 3] = in[4 * i + 3];
  }
}
void hc_pose_ops(const double* q, const double* t, double* T12, double* qback) {
  iso_from_qt(q, t, T12);
  quat_from_rot(T12, qback);
}
void hc_imu_override(const double* T12, const double* imu_q, const double* l2b, double* out12, int rotation_mode) { imu_override(T12, imu_q, l2b, rotation_mode, out12); }
void hc_rotation_of(const double* T12, int mode, double* out12) { rotation_of(T12, mode, out12); }
void hc_odom_message(const double* prev12, const double* cur12, const double* l2b, double dt, double* out13, int rotation_mode) {
  odom_message(prev12, cur12, l2b, dt, rotation_mode, out13);
}
void hc_predict(const double* odom, const double* prev, double* pred) {
  double inv[12], rel[12];
  iso_inverse(prev, inv);
  iso_mul(inv, odom, rel);
  iso_mul(odom, rel, pred);
}
void hc_quat_from_pose(const double* T12, int rotation_mode, double* q) { quat_from_pose(T12, rotation_mode, q); }
// predict_next's algebra (kernels_lm.h; the kernel's own function is __device__): the prediction, its quaternion, its translation
void hc_predict_next(const double* T, const double* prev, int rotation_mode, double* out19) {
  double inv[12], rel[12], pred[12];
  iso_inverse(prev, inv);
  iso_mul(inv, T, rel);
  iso_mul(T, rel, pred);
  for (int i = 0; i < 12; i++) out19[i] = pred[i];
  quat_from_pose(pred, rotation_mode, out19 + 12);
  out19[16] = pred[3]; out19[17] = pred[7]; out19[18] = pred[11];
}
// One scan without correspondences, in the order the kernels run it on a stream's state (odom = the prediction made when the
// previous scan finished, prev = the previous final pose, param_q / param_t = the solve's start point): k_imu_override, two solves
// that change nothing, iso_from_qt, finalize_scan's quat_from_pose and predict_next.  State updated in place; final12 and pose7
// (quaternion, translation: pose_out and the pose log) are what the scan returns.
void hc_scan_no_match(double* odom, double* prev, double* param_q, double* param_t, const double* imu_q, const double* l2b,
                      int rotation_mode, int use_imu, double* final12, double* pose7) {
  if (use_imu) {
    double out[12];
    imu_override(odom, imu_q, l2b, rotation_mode, out);
    for (int i = 0; i < 12; i++) odom[i] = out[i];
    quat_from_pose(out, rotation_mode, param_q);
    param_t[0] = out[3]; param_t[1] = out[7]; param_t[2] = out[11];
  }
  iso_from_qt(param_q, param_t, final12);
  quat_from_pose(final12, rotation_mode, pose7);
  pose7[4] = final12[3]; pose7[5] = final12[7]; pose7[6] = final12[11];
  double p19[19];
  hc_predict_next(final12, prev, rotation_mode, p19);
  for (int i = 0; i < 12; i++) { prev[i] = final12[i]; odom[i] = p19[i]; }
  for (int i = 0; i < 4; i++) param_q[i] = p19[12 + i];
  for (int i = 0; i < 3; i++) param_t[i] = p19[16 + i];
}
// accumulator (29 doubles) over n blocks of 9 doubles (p, a, b) at pose (q, t)
void hc_accumulate(const double* blocks9, int n, const double* q, const double* t, double min_d,
                   double max_d, double* acc) {
  double Rm[12];
  iso_from_qt(q, t, Rm);
  for (int i = 0; i < kAccN; i++) acc[i] = 0.0;
  for (int i = 0; i < n; i++) residual_accumulate(Rm, blocks9 + 9 * i, blocks9 + 9 * i + 3, blocks9 + 9 * i + 6, min_d, max_d, acc);
}
// full solve with the product's controller; returns termination; trace = iterations, accepted
int hc_lm_solve(const double* blocks9, int n, double* q, double* t, double min_d, double max_d,
                int apply_on_ftol, int* iterations, int* accepted, double* initial_cost, double* final_cost) {
  LmState st;
  double acc[kAccN];
  hc_accumulate(blocks9, n, q, t, min_d, max_d, acc);
  int flag = lm_begin(st, q, t, acc, n, apply_on_ftol);
  while (flag == LM_NEED_EVAL) {
    hc_accumulate(blocks9, n, st.cand_q, st.cand_t, min_d, max_d, acc);
    flag = lm_update(st, acc);
  }
  for (int k = 0; k < 4; k++) q[k] = st.q[k];
  for (int k = 0; k < 3; k++) t[k] = st.t[k];
  *iterations = st.iter; *accepted = st.accepted; *initial_cost = st.initial_cost; *final_cost = st.cost;
  return st.termination;
}
// The controller alone on a caller-supplied accumulator (same one for every evaluation): lets a test
// force TrustRegionMinimizer's invalid-step path (non-finite / non-positive-definite normal
// equations) and read the radius sequence.  radius_out[k] = radius after the k-th lm_* call.
int hc_lm_controller(const double* acc29, int n_blocks, const double* q, const double* t, double* radius_out, int cap,
                     int* iterations, int* n_calls) {
  LmState st;
  int k = 0;
  int flag = lm_begin(st, q, t, acc29, n_blocks, 0);
  if (k < cap) radius_out[k] = st.radius;
  k++;
  while (flag == LM_NEED_EVAL && k < 16) {
    flag = lm_update(st, acc29);
    if (k < cap) radius_out[k] = st.radius;
    k++;
  }
  *iterations = st.iter; *n_calls = k;
  return st.termination;
}
// lm_update's parameter-tolerance decision alone: the state is placed at (q, t) with the given |x|, the candidate at (cq, ct);
// the accumulator repeats the current cost, so a step that does not end by parameter tolerance (1) ends by function tolerance (2).
int hc_lm_ptol_decision(const double* q, const double* t, const double* cq, const double* ct, double x_norm) {
  LmState st;
  double acc[kAccN];
  for (int i = 0; i < kAccN; i++) acc[i] = 0.0;
  acc[0] = 1.0;
  const double q0[4] = {0, 0, 0, 1}, t0[3] = {0, 0, 0};
  (void)lm_begin(st, q0, t0, acc, 0, 0);          // (initialises every field; no residual blocks: returns at once)
  for (int k = 0; k < 4; k++) { st.q[k] = q[k]; st.cand_q[k] = cq[k]; }
  for (int k = 0; k < 3; k++) { st.t[k] = t[k]; st.cand_t[k] = ct[k]; }
  st.x_norm = x_norm; st.cost = 1.0; st.model_cost_change = 1.0;
  (void)lm_update(st, acc);
  return st.termination;
}
float hc_sqdist(const float* a, const float* b) { return sqdist_f(a[0], a[1], a[2], b[0], b[1], b[2]); }

}  // extern "C"
