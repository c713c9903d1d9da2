// The odometry-edge leaf functions of liodom_amd/csrc/liodom_math.h compiled for the host (tests/odom_edge_host_lib.py builds
// this with -ffp-contract=off and calls it through ctypes): the reference tests/test_odom_edge_math_host.py holds to
// tests/odom_edge_model.py, and tests/test_gpu_odom_edges.py holds the device's bytes to.
#include "../include/liodom_hip.h"
#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

static_assert(sizeof(liodom_odom_edge_t) == 8 * kOdomEdgeWords, "record layout");

extern "C" {

// n intervals of the stream poses[m x 7] / recs[m] -> out[n] (656 bytes each); the caller has checked 0 <= from < to < m
void oeh_chain(const double* poses, const liodom_pose_cov_t* recs, const int* from, const int* to, int n, double inflation, double fr,
               double ft, liodom_odom_edge_t* out) {
  for (int i = 0; i < n; i++)
    odom_edge_host(poses, recs, from[i], to[i], inflation, fr, ft, reinterpret_cast<unsigned long long*>(out + i));
}
// the combined accumulator of one interval: 21 lower-triangle sums of Sigma, then the usable, unusable and non-finite-pose scans
void oeh_totals(const double* poses, const liodom_pose_cov_t* recs, int a, int b, double inflation, double fr, double ft, double* tot) {
  double part[64][kOdomAccN], col[64];
  for (int lane = 0; lane < 64; lane++) odom_lane_partial(poses, recs, a, b, lane, inflation, fr * fr, ft * ft, part[lane]);
  for (int e = 0; e < kOdomAccN; e++) {
    for (int lane = 0; lane < 64; lane++) col[lane] = part[lane][e];
    tot[e] = odom_combine64(col);
  }
}
void oeh_term(const double* C36, const double* u, double inflation, double fr2, double ft2, double* M21) {
  odom_transport_term(C36, u, inflation, fr2, ft2, M21);
}
int oeh_usable(const liodom_pose_cov_t* rec, int k) { return odom_scan_usable(rec->scan_index, rec->flags, rec->covariance, k) ? 1 : 0; }
void oeh_edge_covariance(const double* B36, const double* S21, double* Se36) { odom_edge_covariance(B36, S21, Se36); }
int oeh_information(const double* Se36, double* Om36) { return odom_edge_information(Se36, Om36) ? 1 : 0; }

}
