// pred_host.cpp — merges posterior-predictive partial records with pred_merge of hmc_pred.hpp (the
// code hmc_pred.hip compiles) for a CPU test: no HIP, nothing linked.
//
//   pred_host < records
//
// Reads records of HMC_PRED_STRIDE numbers each from stdin (white space between numbers; inf, -inf
// and nan as strtod reads them), merges them in the order given, starting from the first, and
// prints the merged record on one line as %.17g.  No record at all prints the n = 0 record.
#include <stdio.h>
#include <stdlib.h>

#define HMC_PRED_HOST_ONLY
#include "hmc_pred.hpp"

int main() {
  hmc::PredRecord acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double v[HMC_PRED_STRIDE];
  char tok[128];
  int k = 0;
  while (scanf("%127s", tok) == 1) {
    char* end = nullptr;
    v[k] = strtod(tok, &end);
    if (end == tok || *end != '\0') {
      fprintf(stderr, "pred_host: not a number: %s\n", tok);
      return 2;
    }
    if (++k == HMC_PRED_STRIDE) {
      hmc::pred_merge(acc, hmc::PredRecord{v[0], v[1], v[2], v[3], v[4], v[5], v[6], 0.0});
      k = 0;
    }
  }
  if (k != 0) {
    fprintf(stderr, "pred_host: %d numbers after the last whole record of %d\n", k, (int)HMC_PRED_STRIDE);
    return 2;
  }
  printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", acc.n, acc.mu_mean, acc.mu_M2, acc.ll_mean, acc.ll_M2,
         acc.ll_max, acc.ll_sumexp, 0.0);
  return 0;
}
