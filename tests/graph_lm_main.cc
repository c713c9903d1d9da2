// graph_lm.h in a program of its own (tests/test_graph_lm_host.py builds it plain and under ASan + UBSan and runs it).  Doubles go
// in as strtod takes them (hex floats, nan, inf) and come out as %a: bit for bit.
//   defaults                                    -> max_iterations max_pcg_iterations pcg_tol gradient_tol cost_tol
//   refusal mi mpi pcg_tol gradient_tol cost_tol   -> "ok" or "refused"
//   cap max_pcg_iterations n_free               -> the cap on a solve's iterations
//   run mi mpi pcg_tol gradient_tol cost_tol initial_cost n_free n_active
//       plays the device's answers, one line of standard input per step — "p flag iterations gmax" after a solve, "c candidate
//       [cost after linearising there]" after a cost — and prints what the controller does: "pcg <iterations> <lambda>" for each
//       solve it asks for, "try" / "accepted" / "rejected" / "done", and at the end
//       "report initial final max_gradient lambda iterations accepted pcg_iterations termination".  An answer of the wrong kind,
//       one too few or one too many: "script <why>", exit 3.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "graph_lm.h"

using namespace liodom_dev;

static bool read_answer(char kind, char* line, size_t size, char** rest) {
  if (!fgets(line, (int)size, stdin)) { printf("script ended early\n"); return false; }
  if (line[0] != kind || line[1] != ' ') { printf("script has the wrong answer: %s", line); return false; }
  *rest = line + 2;
  return true;
}

static int run(const liodom_graph_options_t& opt, double initial, int n_free, int n_active) {
  GraphLm lm;
  char line[256], *at;
  bool more = lm.begin(opt, initial, n_free, n_active);
  while (more) {
    printf("pcg %d %a\n", lm.pcg_iterations(), lm.lambda);
    if (!read_answer('p', line, sizeof(line), &at)) return 3;
    const int flag = (int)strtol(at, &at, 10), iterations = (int)strtol(at, &at, 10);
    const double gmax = strtod(at, &at);
    if (!lm.after_pcg(flag, iterations, gmax)) { printf("done\n"); break; }
    printf("try\n");
    if (!read_answer('c', line, sizeof(line), &at)) return 3;
    const double cand = strtod(at, &at);
    char* end = at;
    const double relin = strtod(at, &end);
    const GraphLmStep step = lm.after_cost(cand);
    if (step == GRAPH_LM_ACCEPTED) lm.relinearized(end != at ? relin : cand);
    puts(step == GRAPH_LM_ACCEPTED ? "accepted" : step == GRAPH_LM_REJECTED ? "rejected" : "done");
    more = step != GRAPH_LM_DONE;
  }
  if (fgets(line, sizeof(line), stdin)) { printf("script has answers left: %s", line); return 3; }
  const liodom_graph_report_t& r = lm.rep;
  printf("report %a %a %a %a %d %d %d %d\n", r.initial_cost, r.final_cost, r.max_gradient, r.final_lambda, r.iterations, r.accepted_steps,
         r.pcg_iterations, r.termination);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  int at = 2;
  auto next_int = [&]() -> int { return at < argc ? (int)strtol(argv[at++], nullptr, 10) : 0; };
  auto next_double = [&]() -> double { return at < argc ? strtod(argv[at++], nullptr) : 0.0; };
  liodom_graph_options_t opt;
  memset(&opt, 0xff, sizeof(opt));
  if (mode == "defaults") {
    graph_lm_options_default(&opt);
    printf("%d %d %a %a %a\n", opt.max_iterations, opt.max_pcg_iterations, opt.pcg_tolerance, opt.gradient_tolerance, opt.cost_tolerance);
    return graph_lm_options_refusal(&opt) ? 1 : 0;
  }
  if (mode == "cap") {
    const int max_pcg = next_int(), n_free = next_int();
    printf("%d\n", graph_pcg_cap(max_pcg, n_free));
    return 0;
  }
  if (mode != "refusal" && mode != "run") return 2;
  opt.max_iterations = next_int(); opt.max_pcg_iterations = next_int();
  opt.pcg_tolerance = next_double(); opt.gradient_tolerance = next_double(); opt.cost_tolerance = next_double();
  const bool refused = graph_lm_options_refusal(&opt) != nullptr;
  if (mode == "refusal" || refused) { puts(refused ? "refused" : "ok"); return 0; }
  const double initial = next_double();
  const int n_free = next_int(), n_active = next_int();
  return run(opt, initial, n_free, n_active);
}
