// tests/covcheck.cc — compiles the pose-covariance arithmetic of liodom_amd/csrc/liodom_math.h (what k_pose_cov runs on the
// device) for the host, so that tests/test_pose_cov_math.py can compare it with numpy and the oracle without a GPU.
// Test tooling only.
#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

extern "C" {

// H: 21 upper-triangle entries (h_idx order).  Returns 1 if the Cholesky inverse exists.
int cc_inverse(const double* H21, double* inv36) { return spd_inverse6(H21, inv36) ? 1 : 0; }
int cc_eig(const double* A36, double* evals, double* evecs) { return sym_eig6(A36, evals, evecs); }
unsigned int cc_record(const double* H21, double final_cost, int n_res, int termination, int has_solve, double* sigma2,
                       double* info36, double* cov36, double* evals6, double* evecs36) {
  return pose_cov_compute(H21, final_cost, n_res, termination, has_solve, sigma2, info36, cov36, evals6, evecs36);
}
void cc_to_ros(const double* cov36, const double* T12, const double* L12, double* out36) { pose_cov_to_ros(cov36, T12, L12, out36); }
void cc_iso_from_qt(const double* q, const double* t, double* T12) { iso_from_qt(q, t, T12); }
// The information matrix the solver's accumulator forms at (q, t) over n blocks (p a b as 9 doubles each): entries 7 .. 27.
void cc_information(const double* blocks9, int n, const double* q, const double* t, double min_d, double max_d, double* H21) {
  double T[12], acc[kAccN];
  iso_from_qt(q, t, T);
  for (int i = 0; i < kAccN; i++) acc[i] = 0.0;
  for (int i = 0; i < n; i++) residual_accumulate(T, blocks9 + 9 * i, blocks9 + 9 * i + 3, blocks9 + 9 * i + 6, min_d, max_d, acc);
  for (int i = 0; i < 21; i++) H21[i] = acc[7 + i];
}

}  // extern "C"
