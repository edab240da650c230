// hmc_diag.hpp — what the diagnostics kernel families share (utils.py:77-179; samplers.py:213, :246).
//
// The reference's convergence_stats splits every chain into two halves
// (utils.py:88-104), then needs, per dimension:
//   * per split chain j: mean_j and std_j (ddof=1)             -> k_split_moments (hmc_diag_sums.hip)
//   * sums over j of std_j, mean_j, (mean_j - mean_all)^2        -> k_rowsum_partial + k_colsum (two-stage,
//                                                                   deterministic; hmc_diag_sums.hip)
//   * variogram sums  sum_j sum_s (x_j[s+t] - x_j[s])^2, t = lags -> k_conv_series (hmc_diag_lags.hip), k_conv_mfma
//     (hmc_diag_mfma.hip); over a circular window, q_chain never stored whole: hmc_diag_stream.hip
// Everything is additive over chains, so on several GPUs each rank reduces its own
// chains and one small all-reduce combines the per-dimension sums.
// Chains are read in place through strides: element (chain m, sample s, dim d) sits at
//   x[base + m*chain_stride + s*sample_stride + d]
// which covers q_chain[:, 1:, :], warm-up offsets and thinning without copies.
#pragma once
#include <type_traits>
#include <utility>

#include "hmc_device.hpp"
#include "hmc_internal.hpp"

namespace hmc {

constexpr int kDimTile = 64;           // dims per block (lane = dim: coalesced row reads)
constexpr int kLagOOB = 0x40000000;    // buffer bound: lanes past the last series read zeros
#ifndef HMC_MFMA_MIN_N
#define HMC_MFMA_MIN_N 96
#endif
constexpr int kMfmaMinN = HMC_MFMA_MIN_N;   // the matrix-core pass's shortest split chain

struct Src {
  const double* x;
  int64_t chain_stride, sample_stride, base;
  int64_t n_chains;
  int n, D;
  // series per chain: 2 = the split chains j = 2m + h of convergence_stats (half h starts h*n
  // samples in); 1 = one series per chain (a completed half of a streaming window: series j =
  // chain j, its sample s in window row (slot0 + s) % wrap, wrap 0 = row s)
  int halves = 2;
  int wrap = 0, slot0 = 0;
};

__host__ __device__ __forceinline__ int64_t n_series(const Src& s) { return s.halves * s.n_chains; }

__device__ __forceinline__ const double* split_ptr(const Src& s, int64_t j, int smp) {
  if (s.halves == 1) return s.x + s.base + j * s.chain_stride + (int64_t)smp * s.sample_stride;
  const int64_t m = j >> 1;
  const int h = (int)(j & 1);
  return s.x + s.base + m * s.chain_stride + (int64_t)(h * s.n + smp) * s.sample_stride;
}

__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ int64_t uni(int64_t x) {
  return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)x >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)x));
}
template <class T>
__device__ __forceinline__ T* uni(T* p) {
  return reinterpret_cast<T*>(uni((int64_t)(uintptr_t)p));
}

// f(std::integral_constant<int, r>) for the runtime r in [0, N): a uniform branch to one of N
// statically indexed bodies
template <class F, int... I>
__device__ __forceinline__ void static_dispatch_(int r, F& f, std::integer_sequence<int, I...>) {
  ((r == I ? f(std::integral_constant<int, I>{}) : void()), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_dispatch(int r, F& f) {
  static_dispatch_(r, f, std::make_integer_sequence<int, N>{});
}
// f(std::integral_constant<int, i>) for i = 0 .. N-1 in order: a source-level unroll (bodies too
// large for the loop unroller's pragma threshold)
template <class F, int... I>
__device__ __forceinline__ void static_for_(F& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F& f) {
  static_for_(f, std::make_integer_sequence<int, N>{});
}

// A block of 4 row lanes x 64 dims (thread = rl * 64 + dl) adds its four values of dim lane dl
// through LDS: the sum in the fixed order ((r0 + r1) + r2) + r3, read by row lane 0 only.  The
// caller barriers before red is written again.
__device__ __forceinline__ double block_sum4(double (&red)[4][kDimTile], int rl, int dl, double v) {
  red[rl][dl] = v;
  __syncthreads();
  return ((red[0][dl] + red[1][dl]) + red[2][dl]) + red[3][dl];
}

// The matrix-core pass (hmc_diag_mfma.hip) as the entry points of hmc_diag_lags.hip choose it.
bool mfma_ok(const Src& s, int T);
int64_t mfma_work_bound(int64_t n_chains, int D);
hipError_t launch_conv_mfma(const Src& s, int nlag, double* work, double* out, hipStream_t st);
// out[c] = (accumulate: out[c] +) sum_k partial[k][c] for c < ncols (hmc_diag_sums.hip)
hipError_t launch_colsum(const double* partial, int64_t nchunks, int64_t ncols, double* out, bool accumulate,
                         hipStream_t st);

}  // namespace hmc
