// graph_lm.h — the Levenberg-Marquardt rules of liodom_graph_optimize (include/liodom_hip.h; DESIGN.md §3 "Closing loops", "Host
// side") apart from its launches and copies: the options' defaults and refusal, the cap on a solve's iterations, and a controller
// that is told what the device answered and says what to do next.  No HIP include and no liodom_graph: tests/graph_lm_main.cc
// compiles it for the host alone, plain and under sanitizers, and plays scripted answers to it (tests/test_graph_lm_host.py).
//
//   begin(initial cost)  ->  [ pcg_iterations(), lambda: gather + k_graph_pcg  ->  after_pcg(its status)
//                              ->  retract + cost: after_cost(candidate cost)  ->  accepted: swap, linearise, relinearized(cost) ] ...
//
// From lambda = 1e-4.  A step is accepted iff the candidate's cost is below the cost (a NaN is not): lambda <- max(lambda / 10,
// 1e-12), and a relative decrease <= cost_tolerance (0 where the cost is 0) ends with COST; otherwise lambda <- 10 lambda, and
// lambda > 1e12 ends with LAMBDA.  A solve ends the loop with GRADIENT (max |g| <= gradient_tolerance: the device decides), then
// MAX_ITERATIONS (that many steps tried), then BREAKDOWN (its iterations are counted).  After COST the poses have moved, so one
// more launch — with 0 iterations, as the launch that finds MAX_ITERATIONS has — reports max |g| at the poses left.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/liodom_hip.h"

namespace liodom_dev {

// what a solve reports (GraphPcgStatus::flag, kernels_graph.h)
enum { GRAPH_PCG_CONVERGED = 0, GRAPH_PCG_MAX_ITER = 1, GRAPH_PCG_BREAKDOWN = 2, GRAPH_PCG_GRADIENT = 3 };

inline void graph_lm_options_default(liodom_graph_options_t* o) {
  o->max_iterations = 20; o->max_pcg_iterations = 0;      // 0: 6 x free nodes, at most 65 536
  o->pcg_tolerance = 1e-8; o->gradient_tolerance = 1e-9; o->cost_tolerance = 1e-10;
}
// nullptr: fine; otherwise why not (static text)
inline const char* graph_lm_options_refusal(const liodom_graph_options_t* o) {
  if (o->max_iterations < 0 || o->max_pcg_iterations < 0 || !(o->pcg_tolerance >= 0.0) || !(o->gradient_tolerance >= 0.0) || !(o->cost_tolerance >= 0.0))
    return "an option is negative or not a number";
  return nullptr;
}
// the cap on the iterations of one solve over n_free free nodes (the covariance solves share it: graph_marginals.h)
inline int graph_pcg_cap(int max_pcg_iterations, int n_free) {
  if (max_pcg_iterations > 0) return max_pcg_iterations;
  const long long six = 6ll * n_free;
  return (int)(six < 65536 ? six : 65536);
}

enum GraphLmStep { GRAPH_LM_DONE = 0, GRAPH_LM_ACCEPTED = 1, GRAPH_LM_REJECTED = 2 };

struct GraphLm {
  liodom_graph_options_t opt;
  int max_pcg;
  double lambda, cost;
  int pending;                     // the termination found; one more launch reports max |g| at the poses left (-1: none)
  liodom_graph_report_t rep;       // complete once a transition has answered "done"

  // false: done — nothing is free or no edge is active
  bool begin(const liodom_graph_options_t& options, double initial_cost, int n_free, int n_active) {
    opt = options;
    max_pcg = graph_pcg_cap(opt.max_pcg_iterations, n_free);
    lambda = 1e-4; cost = initial_cost; pending = -1;
    memset(&rep, 0, sizeof(rep));
    rep.initial_cost = rep.final_cost = initial_cost;
    rep.final_lambda = lambda;
    rep.termination = LIODOM_GRAPH_TERM_GRADIENT;
    return n_free != 0 && n_active != 0;
  }
  // of the next solve, at `lambda`; 0: the launch only reports max |g|
  int pcg_iterations() const { return (pending >= 0 || rep.iterations >= opt.max_iterations) ? 0 : max_pcg; }
  // true: try the step the solve left; false: done
  bool after_pcg(int flag, int iterations, double gmax) {
    rep.max_gradient = gmax;
    if (pending >= 0) return done(pending);
    if (flag == GRAPH_PCG_GRADIENT) return done(LIODOM_GRAPH_TERM_GRADIENT);
    if (rep.iterations >= opt.max_iterations) return done(LIODOM_GRAPH_TERM_MAX_ITERATIONS);      // (that launch solved nothing)
    rep.pcg_iterations += iterations;
    if (flag == GRAPH_PCG_BREAKDOWN) return done(LIODOM_GRAPH_TERM_BREAKDOWN);
    rep.iterations++;
    return true;
  }
  // ACCEPTED: the candidate poses become the poses; linearise there and call relinearized().  REJECTED: the poses stay.
  GraphLmStep after_cost(double cand) {
    if (cand < cost) {                                // (false for a NaN)
      rep.accepted_steps++;
      const double decrease = cost != 0.0 ? (cost - cand) / fabs(cost) : 0.0;      // (an indefinite Omega can make chi2 negative)
      lambda = std::max(lambda / 10.0, 1e-12);
      rep.final_lambda = lambda;
      if (decrease <= opt.cost_tolerance) pending = LIODOM_GRAPH_TERM_COST;
      return GRAPH_LM_ACCEPTED;
    }
    lambda *= 10.0;
    rep.final_lambda = lambda;
    if (lambda > 1e12) { done(LIODOM_GRAPH_TERM_LAMBDA); return GRAPH_LM_DONE; }
    return GRAPH_LM_REJECTED;
  }
  // the cost at the accepted poses (the same edges summed in the same order: equal to the candidate's)
  void relinearized(double new_cost) { cost = rep.final_cost = new_cost; }

 private:
  bool done(int termination) { rep.termination = termination; return false; }
};

}  // namespace liodom_dev
