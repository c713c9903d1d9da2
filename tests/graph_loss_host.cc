// graph_loss of liodom_amd/csrc/liodom_math.h compiled for the host, in a program of its own (tests/test_graph_loss_host.py builds
// it with -ffp-contract=off under ASan + UBSan and runs it).  Reads lines "loss c s" from the standard input — loss a number, c and
// s hexadecimal floating point, so that no digit is lost —, and prints "rho w" for each, hexadecimal too.
#include <stdio.h>
#include <stdlib.h>

#include "../liodom_amd/csrc/liodom_math.h"

int main() {
  char line[256];
  int n = 0;
  while (fgets(line, sizeof(line), stdin)) {
    char *p = line, *q = nullptr;
    const long loss = strtol(p, &q, 10);
    if (q == p) continue;
    p = q;
    const double c = strtod(p, &q);
    if (q == p) { fprintf(stderr, "line %d: no scale\n", n + 1); return 2; }
    p = q;
    const double s = strtod(p, &q);
    if (q == p) { fprintf(stderr, "line %d: no s\n", n + 1); return 2; }
    double rho = -1.0, w = -1.0;
    liodom_dev::graph_loss((int)loss, c, s, &rho, &w);
    printf("%a %a\n", rho, w);
    n++;
  }
  return n > 0 ? 0 : 2;
}
