// The pose-graph leaf functions of liodom_amd/csrc/liodom_math.h compiled for the host (tests/test_graph_math_host.py builds this
// with -ffp-contract=off and calls it through ctypes).
#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

extern "C" {

void gmh_edge(const double* Xi, const double* Xj, const double* Z, double* e, double* A, double* B) { graph_edge_error(Xi, Xj, Z, e, A, B); }
void gmh_error(const double* Xi, const double* Xj, const double* Z, double* e) { graph_edge_error(Xi, Xj, Z, e, nullptr, nullptr); }
double gmh_chi2(const double* e, const double* Om) { return graph_edge_chi2(e, Om); }
void gmh_blocks(const double* e, const double* A, const double* B, const double* Om, double* chi2, double* gi, double* gj, double* Hii,
                double* Hij, double* Hjj) {
  graph_edge_blocks(e, A, B, Om, 1, chi2, gi, gj, Hii, Hij, Hjj);
}
void gmh_retract(const double* X, const double* delta, double* out) { graph_retract(X, delta, out); }
int gmh_damped_inverse(const double* D, double lambda, double* inv) { return graph_damped_inverse(D, lambda, inv) ? 1 : 0; }

}
