// hmc_lane_group.hpp — the lane-group layout of one chain inside a wave64, shared by the kernels that
// hold a chain's coordinates that way (hmc_random.hip, hmc_mix.hip): a chain's D coordinates live in
// lpc consecutive lanes, lane s owning the pairs k = s + lpc*j (j < K, dims 2k and 2k+1); cpw chains
// share a wave.  Which lane is whose, the lane's slots, row loads and stores, the momentum draw and
// the launch grid.
#pragma once
#include "hmc_device.hpp"
#include "hmc_internal.hpp"

namespace hmc {

struct Lane {
  int lane, g, s, base;
  int64_t c;       // local chain (or row) index
  bool active;     // lane belongs to a live chain
  bool leader;     // first lane of a live chain's group
};

__device__ __forceinline__ Lane lane_info(const RandArgs& a) {
  Lane L;
  L.lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  L.g = L.lane / a.lpc;
  L.s = L.lane - L.g * a.lpc;
  L.base = L.g * a.lpc;
  L.c = wave * a.cpw + L.g;
  L.active = (L.g < a.cpw) && (L.c < a.n);
  L.leader = L.active && (L.s == 0);
  return L;
}

// the lane's pair slots kk[j] and whether each holds coordinates of a live chain
template <int K>
__device__ __forceinline__ void lane_slots(const RandArgs& a, const Lane& ln, int (&kk)[K], bool (&pv)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    kk[j] = ln.s + a.lpc * j;
    pv[j] = ln.active && kk[j] < a.npairs;
  }
}

// the lane's coordinates of a [D] row; slots past D (and lanes without a chain) read as zero
template <int K>
__device__ __forceinline__ void load_row(const double* row, const RandArgs& a, const int (&kk)[K], const bool (&pv)[K],
                                         double (&x)[2 * K]) {
  const bool even = (a.D & 1) == 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    x[2 * j] = x[2 * j + 1] = 0.0;
    if (pv[j]) load_pair(row, kk[j], even, 2 * kk[j] + 1 < a.D, x[2 * j], x[2 * j + 1]);
  }
}

template <int K>
__device__ __forceinline__ void store_row(double* row, const RandArgs& a, const int (&kk)[K], const bool (&pv)[K],
                                          const double (&x)[2 * K]) {
  const bool even = (a.D & 1) == 0;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (pv[j]) store_pair(row, kk[j], even, 2 * kk[j] + 1 < a.D, x[2 * j], x[2 * j + 1]);
}

// p ~ N(0, cov_p) of iteration `it` (0: the chain start's p0): the replay stream's row, or Philox
// block (k, it, chain) through Box-Muller for pair k, times p_scale where the mass is not the
// identity (GEN)
template <int K, bool GEN, bool REPLAY>
__device__ __forceinline__ void draw_momentum(const RandArgs& a, const Lane& ln, int it, const int (&kk)[K],
                                              const bool (&pv)[K], double (&p)[2 * K]) {
  const bool even = (a.D & 1) == 0;
  const uint64_t gc = (uint64_t)(a.chain_offset + ln.c);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    p[2 * j] = 0.0;
    p[2 * j + 1] = 0.0;
    if (pv[j]) {
      const int d = 2 * kk[j];
      if constexpr (REPLAY) {
        const double* row = (it == 0) ? a.rp0 + ln.c * (int64_t)a.D
                                      : a.rp + (ln.c * (int64_t)a.niter + (it - 1)) * a.D;
        load_pair(row, kk[j], even, d + 1 < a.D, p[2 * j], p[2 * j + 1]);
      } else {
        normal_pair(draw_block((uint32_t)kk[j], (uint32_t)it, gc, a.k0, a.k1), p[2 * j], p[2 * j + 1]);
        if (GEN && a.pscale) {
          p[2 * j] *= a.pscale[d];
          if (d + 1 < a.D) p[2 * j + 1] *= a.pscale[d + 1];
        }
      }
      if (d + 1 >= a.D) p[2 * j + 1] = 0.0;
    }
  }
}

// four waves per block of 256 threads, cpw chains per wave
inline dim3 grid_for(const RandArgs& a) {
  const int64_t waves = (a.n + a.cpw - 1) / a.cpw;
  return dim3((unsigned)((waves + 3) / 4));
}

}  // namespace hmc
