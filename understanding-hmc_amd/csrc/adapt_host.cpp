// adapt_host.cpp — prints the step-size adaptation rule of hmc_adapt.hpp (the code the ADAPT
// kernels compile) for a CPU test: no HIP, nothing linked.
//
//   adapt_host DELTA S0 ADAPT_END ALPHA...
//
// Starts from adapt_initial(S0) and ends one iteration per ALPHA, iteration i = 1, 2, ... adapting
// while i < ADAPT_END (gamma = 0.05, t0 = 10, kappa = 0.75).  One line per iteration: the eight state
// slots after it and the multiplier the next iteration runs at, as %.17g.
#include <stdio.h>
#include <stdlib.h>

#include "hmc_adapt.hpp"

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s DELTA S0 ADAPT_END ALPHA...\n", argv[0]);
    return 2;
  }
  const hmc::AdaptParams p{atof(argv[1]), 0.05, 10.0, 0.75};
  const double s0 = atof(argv[2]);
  const int adapt_end = atoi(argv[3]);
  if (!(p.delta > 0.0 && p.delta < 1.0) || !(s0 > 0.0)) {
    fprintf(stderr, "need 0 < DELTA < 1 and S0 > 0\n");
    return 2;
  }
  hmc::AdaptState a = hmc::adapt_initial(s0);
  double row[HMC_ADAPT_STRIDE];
  for (int i = 1; i + 3 < argc; ++i) {
    hmc::adapt_iteration(a, p, i < adapt_end, atof(argv[i + 3]));
    hmc::adapt_store(row, a);
    for (int k = 0; k < HMC_ADAPT_STRIDE; ++k) printf("%.17g ", row[k]);
    printf("%.17g\n", hmc::adapt_scale(a, i + 1 < adapt_end));
  }
  return 0;
}
