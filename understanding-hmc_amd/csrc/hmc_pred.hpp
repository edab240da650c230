// hmc_pred.hpp — posterior-predictive partial records of the GLM targets (hmc_pred.hip,
// hmc_glm_predictive): what the host and the device share.  One record per evaluation row holds
// mergeable moments of mu and ll over a set of samples (include/hmc.h: HMC_PRED_STRIDE slots):
//   0 n   1 mu_mean   2 mu_M2   3 ll_mean   4 ll_M2   5 ll_max   6 ll_sumexp   7 reserved (0)
// pred_merge below is the one merge rule: the kernel's lanes, its sample blocks, pred_host.cpp
// (which prints it for tests/test_predictive_host.py) and, restated in NumPy,
// hmc_amd.predictive.merge_partials.  The launch geometry (sample blocks, workspace) is stated here
// once, as a function of the shapes alone.
//
// pred_host.cpp defines HMC_PRED_HOST_ONLY: no HIP header, no launcher.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hmc.h"

#ifndef HMC_PRED_HOST_ONLY
#include <hip/hip_runtime.h>
#endif
#if defined(__HIPCC__) && !defined(HMC_PRED_HOST_ONLY)
#define HMC_PRED_FN __host__ __device__ __forceinline__
#else
#define HMC_PRED_FN inline
#endif

namespace hmc {

struct PredRecord {
  double n, mu_mean, mu_M2, ll_mean, ll_M2, ll_max, ll_sumexp, reserved;
};
static_assert(sizeof(PredRecord) == HMC_PRED_STRIDE * sizeof(double), "PredRecord is one row of out");

HMC_PRED_FN bool pred_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }
HMC_PRED_FN double pred_nan() { return __builtin_nan(""); }

// Chan's pairwise update of (mean, M2) for na, nb > 0 samples.  A difference of the means that is
// not finite (an infinite or NaN mean on either side) follows NumPy's two-pass result on the
// concatenated data: the mean is the sum of the means (inf + x = inf, inf - inf = NaN), M2 is NaN.
HMC_PRED_FN void pred_merge_moments(double na, double& mean_a, double& M2_a, double nb, double mean_b,
                                    double M2_b) {
  const double n = na + nb;
  const double delta = mean_b - mean_a;
  if (pred_finite(delta)) {
    mean_a = mean_a + delta * (nb / n);
    M2_a = (M2_a + M2_b) + (delta * delta) * (na * nb / n);
  } else {
    mean_a = mean_a + mean_b;
    M2_a = pred_nan();
  }
}

// The log-sum-exp pair (max, sum exp(ll - max)).  A side that holds the maximum keeps its sum as
// it is (also when both maxima are -inf: every ll was -inf, the sums are 0); the other side is
// rescaled, and a side with max = -inf adds 0 * exp(-inf) = 0.  NaN on either side: both NaN
// (fmax would drop it).
HMC_PRED_FN void pred_merge_lse(double& max_a, double& sum_a, double max_b, double sum_b) {
  if (max_a != max_a || max_b != max_b || sum_a != sum_a || sum_b != sum_b) {
    max_a = sum_a = pred_nan();
    return;
  }
  const double m = max_a > max_b ? max_a : max_b;
  const double ta = max_a == m ? sum_a : sum_a * exp(max_a - m);
  const double tb = max_b == m ? sum_b : sum_b * exp(max_b - m);
  max_a = m;
  sum_a = ta + tb;
}

// a <- a merged with b.  A record with n == 0 is the identity.
HMC_PRED_FN void pred_merge(PredRecord& a, const PredRecord& b) {
  if (b.n == 0.0) return;
  if (a.n == 0.0) {
    a = b;
    return;
  }
  pred_merge_moments(a.n, a.mu_mean, a.mu_M2, b.n, b.mu_mean, b.mu_M2);
  pred_merge_moments(a.n, a.ll_mean, a.ll_M2, b.n, b.ll_mean, b.ll_M2);
  pred_merge_lse(a.ll_max, a.ll_sumexp, b.ll_max, b.ll_sumexp);
  a.n += b.n;
  a.reserved = 0.0;
}

// ---- launch geometry: a function of (D, n_eval, S) alone, never of the device
constexpr int kPredWaves = 4;           // row tiles (16 evaluation rows each) per block
constexpr int kPredMinTiles = 8;        // a sample block streams at least 8 tiles of 16 samples ...
constexpr int64_t kPredBlocks = 2048;   // ... and the launch aims at this many blocks
constexpr int64_t kPredMaxSampleBlocks = 65535;   // gridDim.y

inline int64_t pred_row_groups(int64_t n_eval) { return (n_eval + 16 * kPredWaves - 1) / (16 * kPredWaves); }

// 16-sample tiles per sample block; the sample blocks of the launch follow from it
inline int64_t pred_tiles_per_block(int64_t n_eval, int64_t n_samples) {
  const int64_t tiles = (n_samples + 15) / 16;
  const int64_t groups = pred_row_groups(n_eval);
  int64_t want = (kPredBlocks + groups - 1) / groups;                 // sample blocks that fill the launch
  want = want > kPredMaxSampleBlocks ? kPredMaxSampleBlocks : want;
  int64_t per = (tiles + want - 1) / want;
  per = per < kPredMinTiles ? kPredMinTiles : per;
  const int64_t least = (tiles + kPredMaxSampleBlocks - 1) / kPredMaxSampleBlocks;
  return per < least ? least : per;
}

inline int64_t pred_sample_blocks(int D, int64_t n_eval, int64_t n_samples) {
  if (D < 1 || D > HMC_LOGIT_MAX_D || n_eval < 1 || n_eval > HMC_LOGIT_MAX_N || n_samples < 1) return 0;
  const int64_t tiles = (n_samples + 15) / 16;
  const int64_t per = pred_tiles_per_block(n_eval, n_samples);
  return (tiles + per - 1) / per;
}

#if !defined(HMC_PRED_HOST_ONLY)
// Records of every sample block into ws ([blocks][n_eval] records), then their merge, in block
// order, into out ([n_eval] records).  rows = samples per chain, n_samples = chains x rows.
hipError_t launch_pred(const hmc_glm& eval, const hmc_samples& s, int64_t rows, int64_t n_samples, double* out,
                       double* ws, hipStream_t stream);
#endif

}  // namespace hmc

#undef HMC_PRED_FN
