// nuts_tree_host.cpp — prints the integer tree bookkeeping of hmc_nuts_tree.hpp (the code the NUTS
// kernels compile) for a CPU test: no HIP, nothing linked.
//
//   nuts_tree_host D_MAX DEPTH
//
// One line per point m = 1 .. 2^DEPTH of a sub-tree:
//   odd m:   "m s SLOT"                   the save slot of point m
//   even m:  "m c L:SLOT L:SLOT ..."      check_points(m) in order, each with its save slot
#include <stdio.h>
#include <stdlib.h>

#include "hmc_nuts_tree.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s D_MAX DEPTH\n", argv[0]);
    return 2;
  }
  const int d_max = atoi(argv[1]), depth = atoi(argv[2]);
  if (d_max < 1 || d_max > 30 || depth < 0 || depth > 30) {
    fprintf(stderr, "need 1 <= D_MAX <= 30 and 0 <= DEPTH <= 30\n");
    return 2;
  }
  for (int m = 1; m <= (1 << depth); ++m) {
    if (m & 1) {
      printf("%d s %d\n", m, hmc::save_slot(m, d_max));
      continue;
    }
    printf("%d c", m);
    hmc::CheckPoints cp(m);
    int n = 0;
    do {
      printf(" %d:%d", cp.pt, hmc::save_slot(cp.pt, d_max));
      ++n;
    } while (cp.next());
    if (n != hmc::CheckPoints(m).count() || n != hmc::cp_count(m) || hmc::CheckPoints(m).half != hmc::cp_r(m)) {
      fprintf(stderr, "m = %d: iterated %d, count() %d, cp_count %d, half %d, cp_r %d\n", m, n,
              hmc::CheckPoints(m).count(), hmc::cp_count(m), hmc::CheckPoints(m).half, hmc::cp_r(m));
      return 1;
    }
    printf("\n");
  }
  return 0;
}
