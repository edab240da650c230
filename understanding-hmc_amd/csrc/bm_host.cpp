// bm_host.cpp — host-only program (no HIP) behind hmc_bm_radius.hpp for tests/test_bm_split_host.py:
// reads numbers j (decimal or 0x..., 1 <= j <= 2^52) from stdin and prints, for u1 = j 2^-52, one
// line of four hexadecimal words:
//   the mantissa and the exponent (as a double) of bm_split (std::frexp here);
//   bm_neg2_log(u1), the radius function the kernels compile;
//   -2 log(u1) in the form that function replaced: frexp, the series in r = m / c_j - 1 with its
//     unscaled coefficients over the unscaled table (1 / c_j, log c_j), the result times -2.
// Both tables come from the same (1 / c_j, log c_j), here from libm: the identity between the two
// forms holds for any table contents.  Built with -ffp-contract=off: every fused operation is a
// std::fma, as on the device.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmc_bm_radius.hpp"

namespace {

uint64_t bits_of(double x) { return __builtin_bit_cast(uint64_t, x); }

// The form before the factor -2 moved into the table and the constants (what hmc_device.hpp's table_log was,
// followed by the multiply by -2).
double neg2_log_unscaled(double u, const double* logt) {
  int k;
  const double m = std::frexp(u, &k);
  const uint32_t mhi = (uint32_t)(bits_of(m) >> 32);
  const uint32_t j16 = (mhi >> (hmc::kLogShift - 4)) & ((hmc::kLogN - 1) << 4);
  const double* e = reinterpret_cast<const double*>(reinterpret_cast<const char*>(logt) + j16);
  const double r = std::fma(m, e[0], -1.0);
#ifdef HMC_SMALL_TABLES
  double pl = std::fma(r, 1.0 / 7.0, -1.0 / 6.0);
  pl = std::fma(r, pl, 1.0 / 5.0);
  pl = std::fma(r, pl, -1.0 / 4.0);
#else
  double pl = std::fma(r, 1.0 / 5.0, -1.0 / 4.0);
#endif
  pl = std::fma(r, pl, 1.0 / 3.0);
  pl = std::fma(r, pl, -0.5);
  const double l1p = std::fma(r * r, pl, r);
  const double dk = (double)k;
  const double lg = std::fma(dk, 6.93147180369123816490e-01, e[1] + std::fma(dk, 1.90821492927058770002e-10, l1p));
  return -2.0 * lg;
}

}  // namespace

int main() {
  std::vector<double> unscaled(2 * hmc::kLogN), scaled(2 * hmc::kLogN);
  for (int j = 0; j < hmc::kLogN; ++j) {
    const bool last = j == hmc::kLogN - 1;
    const double c = last ? 1.0 : 0.5 + ((double)j + 0.5) * (0.5 / hmc::kLogN);
    const double ic = last ? 1.0 : 1.0 / c;
    const double lc = last ? 0.0 : -std::log(ic);
    unscaled[2 * j] = ic;
    unscaled[2 * j + 1] = lc;
    const hmc::bm_entry e = hmc::bm_log_entry(ic, lc);
    scaled[2 * j] = e.x;
    scaled[2 * j + 1] = e.y;
  }
  char s[64];
  while (std::scanf("%63s", s) == 1) {
    const uint64_t j = std::strtoull(s, nullptr, 0);
    const double u = std::ldexp((double)j, -52);   // exact: j <= 2^52
    double m, dk;
    hmc::bm_split(u, m, dk);
    std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(m), bits_of(dk),
                bits_of(hmc::bm_neg2_log(u, scaled.data())), bits_of(neg2_log_unscaled(u, unscaled.data())));
  }
  return 0;
}
