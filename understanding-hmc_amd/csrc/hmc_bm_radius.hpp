// hmc_bm_radius.hpp — the squared radius of the table-driven Box–Muller, t = -2 log(u1), for
// u1 = j 2^-52, 1 <= j <= 2^52 (a normal number in [2^-52, 1]).
//
// u1 = 2^k m with m in [0.5, 1); bucket j = the top mantissa bits of m (kLogN buckets); with c_j the bucket's
// centre, log m = log c_j + log1p(r), r = m / c_j - 1, |r| <= 2^-11 (series to r^5; r^6/6 < 2^-68).
// Everything is formed already scaled by -2, so no multiply follows the logarithm:
//   * the table entry of bucket j is (-2 / c_j, 2 log(1 / c_j));
//   * r2 = fma(m, -2 / c_j, 2) = -2 r, and the series runs in r2 with its coefficients rescaled by
//     exact powers of two;
//   * the two parts of ln 2 are scaled by -2.
// Each input is the unscaled one times an exact power of two (and a sign), so every intermediate is
// exactly -2 times (or that power of two times) what log(u1) formed by frexp, the unscaled series
// and a final multiply by -2 passes through, and the rounded result is the same bit for bit
// (bm_host.cpp keeps that form beside this one; tests/test_bm_split_host.py compares them).
// The one exception is the sign of an exact zero (u1 = 1 when the table's rounding cancels): x - x
// is +0 here and -2 (+0) = -0 there; bm_sqrt takes the maximum of either with its floor.
//
// Compiles for the device (through hmc_device.hpp, which defines fmac_k before it includes this
// file) and for a host-only program (bm_host.cpp: std::fma and bit casts, -ffp-contract=off).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HMC_BM_FN __device__ __forceinline__
#else
#include <cmath>
#define HMC_BM_FN inline
#endif

namespace hmc {

#ifdef HMC_SMALL_TABLES
constexpr int kLogN = 128, kLogShift = 13;
#else
constexpr int kLogN = 1024, kLogShift = 10;
#endif

#ifdef __HIPCC__
typedef double2 bm_entry;
HMC_BM_FN double bm_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }
HMC_BM_FN double bm_fma_k(double x, double y, double c) { return fmac_k(x, y, c); }   // c: an SGPR-pair operand
#else
struct bm_entry {
  double x, y;
};
inline double bm_fma(double x, double y, double z) { return std::fma(x, y, z); }
inline double bm_fma_k(double x, double y, double c) { return std::fma(x, y, c); }
#endif

// The table entry from the unscaled one, (ic, lc) = (1 / c_j, log c_j): both times -2, exactly.
// (The last bucket has c = 1: the unscaled entry (1, 0), this one (-2, -0).)
HMC_BM_FN bm_entry bm_log_entry(double ic, double lc) {
  bm_entry e;
  e.x = -2.0 * ic;
  e.y = -2.0 * lc;
  return e;
}

// (m, k as a double) of u = 2^k m, m in [0.5, 1): v_frexp_mant_f64, v_frexp_exp_i32_f64 and
// v_cvt_f64_i32 on the device (each priced like a v_fma_f64 at four waves per SIMD,
// profiles/rr_instr_prices.txt: an integer split of the high word has nothing to win), std::frexp
// on the host.
HMC_BM_FN void bm_split(double u, double& m, double& dk) {
#ifdef __HIPCC__
  m = __builtin_amdgcn_frexp_mant(u);
  dk = (double)__builtin_amdgcn_frexp_exp(u);
#else
  int k;
  m = std::frexp(u, &k);
  dk = (double)k;
#endif
}

// -2 log(u1) from the table at `logt` (kLogN entries of bm_log_entry).
HMC_BM_FN double bm_neg2_log(double u1, const double* logt) {
  const uint32_t hi = (uint32_t)(__builtin_bit_cast(uint64_t, u1) >> 32);
  // byte offset 16 j of bucket j = (hi >> kLogShift) & (kLogN - 1): one shift, one and (the mantissa
  // bits of u1's high word are those of m's)
  const uint32_t j16 = (hi >> (kLogShift - 4)) & ((kLogN - 1) << 4);
  double m, dk;
  bm_split(u1, m, dk);
  const bm_entry e = *reinterpret_cast<const bm_entry*>(reinterpret_cast<const char*>(logt) + j16);
  const double r2 = bm_fma(m, e.x, 2.0);                                  // -2 r
  // log1p(r) = r + r^2 (-1/2 + r (1/3 + r (-1/4 + r / 5 ...))).  In r2 = -2 r the Horner step that
  // forms s p has the coefficient of the unscaled step times s, and s doubles with the sign swapped
  // from one step to the next so that r2 (s p) = (-2 s) (r p); the last step has s = -1/2, so that
  // (r2 r2) (s p) + r2 = -2 (r^2 p + r).
#ifdef HMC_SMALL_TABLES
  double pl = bm_fma_k(r2, (1.0 / 7.0) / 64.0, (1.0 / 6.0) / 32.0);     // s = -1/32: -2 s / 2 = 1/64 on r's coefficient
  pl = bm_fma_k(r2, pl, (1.0 / 5.0) / 16.0);                              // s = 1/16
  pl = bm_fma_k(r2, pl, (1.0 / 4.0) / 8.0);                               // s = -1/8
#else
  double pl = bm_fma_k(r2, (1.0 / 5.0) / 16.0, (1.0 / 4.0) / 8.0);      // s = -1/8: (r / 5 - 1/4) (-1/8)
#endif
  pl = bm_fma_k(r2, pl, (1.0 / 3.0) / 4.0);                               // s = 1/4
  pl = bm_fma_k(r2, pl, 0.25);                                            // s = -1/2: (-0.5) (-1/2)
  const double l1p = bm_fma(r2 * r2, pl, r2);                             // -2 log1p(r)
  return bm_fma(dk, -2.0 * 6.93147180369123816490e-01, e.y + bm_fma(dk, -2.0 * 1.90821492927058770002e-10, l1p));
}

}  // namespace hmc
