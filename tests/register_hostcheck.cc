// register_pass_converged of liodom_math.h compiled for the host (-ffp-contract=off), for tests/test_register_model.py.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../liodom_amd/csrc/liodom_math.h"

extern "C" int rh_pass_converged(const double* q_old, const double* t_old, const double* q_new, const double* t_new, double stop_t,
                                 double stop_r, double* moves) {
  return liodom_dev::register_pass_converged(q_old, t_old, q_new, t_new, stop_t, stop_r, moves, moves + 1) ? 1 : 0;
}
