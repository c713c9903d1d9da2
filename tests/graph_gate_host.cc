// graph_gate of liodom_amd/csrc/liodom_math.h compiled for the host (tests/test_graph_cov_model.py builds this with
// -ffp-contract=off and calls it through ctypes).
#include "../liodom_amd/csrc/liodom_math.h"

using namespace liodom_dev;

extern "C" {

int ggh_gate(const double* Xi, const double* Xj, const double* Z, const double* Om, const double* Sii, const double* Sij, const double* Sjj,
             double* d2) {
  return graph_gate(Xi, Xj, Z, Om, Sii, Sij, Sjj, d2) ? 1 : 0;
}

}
