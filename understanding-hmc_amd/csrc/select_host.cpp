// select_host.cpp — the key map, its inverse and the pick rule of hmc_select.hpp (the code
// hmc_select.hip compiles) behind a host-only program for a CPU test: no HIP, nothing linked.
//
//   select_host key  < bit patterns     one double per token, as 16 hexadecimal digits of its bits
//   select_host pick < histograms       per histogram: nbins, the rank, then nbins counts (decimal)
//
// key prints, per double, its key and the bits that the inverse map gives back, both as 16
// hexadecimal digits.  pick prints, per histogram, the chosen digit and the remaining rank.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#define HMC_SELECT_HOST_ONLY
#include "hmc_select.hpp"

static int run_key() {
  char tok[64];
  while (scanf("%63s", tok) == 1) {
    char* end = nullptr;
    const uint64_t bits = strtoull(tok, &end, 16);
    if (end == tok || *end != '\0' || strlen(tok) != 16) {
      fprintf(stderr, "select_host: not 16 hexadecimal digits: %s\n", tok);
      return 2;
    }
    const uint64_t key = hmc::select_key(__builtin_bit_cast(double, bits));
    const uint64_t back = __builtin_bit_cast(uint64_t, hmc::select_unkey(key));
    printf("%016" PRIx64 " %016" PRIx64 "\n", key, back);
  }
  return 0;
}

static int run_pick() {
  long long nbins, rank;
  while (scanf("%lld", &nbins) == 1) {
    if (nbins < 1 || nbins > (1 << 20) || scanf("%lld", &rank) != 1) {
      fprintf(stderr, "select_host: bad histogram header\n");
      return 2;
    }
    std::vector<int64_t> c((size_t)nbins);
    for (long long i = 0; i < nbins; ++i) {
      long long v;
      if (scanf("%lld", &v) != 1) {
        fprintf(stderr, "select_host: %lld counts expected, %lld read\n", nbins, i);
        return 2;
      }
      c[(size_t)i] = v;
    }
    int64_t rem = 0;
    const int digit = hmc::select_pick(c.data(), (int)nbins, rank, &rem);
    printf("%d %lld\n", digit, (long long)rem);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "key") == 0) return run_key();
  if (argc == 2 && strcmp(argv[1], "pick") == 0) return run_pick();
  fprintf(stderr, "usage: select_host key|pick < input\n");
  return 2;
}
