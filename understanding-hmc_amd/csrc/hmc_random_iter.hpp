// hmc_random_iter.hpp — the per-iteration bookkeeping of HMC_sampler.gen_sample_random
// (samplers.py:413-420, :428-475), written once for the Random-trajectory kernels: which iteration
// stores a row and which, the (L, log u) draw, the Metropolis tally with its end-of-launch flush, and
// the init epilogue.  hmc_random.hip, hmc_mix.hip, hmc_logit.hip, hmc_dense.hip and hmc_big.hip use
// it (the NUTS kernels take the row rule through hmc_nuts_tree.hpp); what a kernel emits differently
// (non-temporal or null-checked E rows, debug hooks, how it reduces L over a wave) stays in the kernel.
// hmc_wave.hip and hmc_rows.hip keep their own scalar-ALU forms of the same rules.
#pragma once
#include "hmc_device.hpp"
#include "hmc_internal.hpp"

namespace hmc {

// whether iteration `it` stores a row of q_chain / E_chain / dE_chain (samplers.py:436-438, :466,
// :471; NUTS :571-573, :786-791): after warm-up, every thin-th iteration and the last one
__device__ __forceinline__ bool stores_row(const RandArgs& a, int it) {
  return it >= a.wu && ((it == a.niter) || ((it - a.wu + 1) % a.thin == 0));
}

// ... and which: (it - warm_up) // thin (the last write of a thinned row wins, as in Python); 0
// during warm-up, when no row is stored
__device__ __forceinline__ int64_t row_of(const RandArgs& a, int it) {
  return it >= a.wu ? (int64_t)((it - a.wu) / a.thin) : 0;
}

// Trajectory length (samplers.py:441, Q1) and log u of the Metropolis test (:461) of iteration `it`
// of global chain gc: Philox block kDrawSlot, L = L_low + x mod (L_high - L_low), u = u53(z, w).
struct TrajDraw {
  int L;
  double lnu;
};
__device__ __forceinline__ TrajDraw draw_traj(const RandArgs& a, int it, uint64_t gc) {
  const uint4 r = draw_block(kDrawSlot, (uint32_t)it, gc, a.k0, a.k1);
  const double u = u53(r.z, r.w);
  return TrajDraw{uniform_int(r.x, a.L_low, a.L_high), u > 0.0 ? fast_log(u) : -__builtin_inf()};   // log(random())
}

// The five tallies of one lane over a launch (samplers.py:462-472, :450), counted by the lane that
// owns a chain and flushed once per wave.
struct RandomTally {
  unsigned long long n_acc = 0, n_acc_wu = 0, n_lf = 0, n_lf2 = 0, n_oob = 0;

  // one finished iteration of one chain; post: it >= warm_up
  __device__ __forceinline__ void count(const RandArgs& a, int it, bool post, bool accept, int L) {
    if (accept) {
      if (post) ++n_acc; else ++n_acc_wu;
    } else if (it < a.i_oob) {
      ++n_oob;                                           // reference would raise IndexError (Q5)
    }
    const unsigned long long Lp = L > 0 ? (unsigned long long)L : 0ull;  // xrange(1, L+1) is empty for L <= 0
    n_lf += Lp;
    n_lf2 += Lp * Lp;
  }

  // end of launch, every lane of the wave: per-wave sums into row `slot` of the HMC_COUNTER_SLOTS rows
  __device__ __forceinline__ void flush(const RandArgs& a, int lane, int64_t slot) {
    n_acc = wave_sum_u64(n_acc);
    n_acc_wu = wave_sum_u64(n_acc_wu);
    n_lf = wave_sum_u64(n_lf);
    n_lf2 = wave_sum_u64(n_lf2);
    n_oob = wave_sum_u64(n_oob);
    if (lane == 0 && a.cnt) {
      unsigned long long* cs = a.cnt + (slot & (HMC_COUNTER_SLOTS - 1)) * HMC_NCOUNTERS;
      if (n_acc) atomicAdd(cs + HMC_CNT_ACCEPT, n_acc);
      if (n_acc_wu) atomicAdd(cs + HMC_CNT_ACCEPT_WU, n_acc_wu);
      if (n_lf) atomicAdd(cs + HMC_CNT_LEAPFROG, n_lf);
      if (n_lf2) atomicAdd(cs + HMC_CNT_LEAPFROG_SQ, n_lf2);
      if (n_oob) atomicAdd(cs + HMC_CNT_OOB_REJECT, n_oob);
    }
  }
};

// Chain initialisation's last step (samplers.py:417-420): E(q_start, p0) is the energy the first
// iteration's dE refers to and row 0 of E_chain; dE_chain[:, 0] = 0.
__device__ __forceinline__ void store_init_energy(const RandArgs& a, int64_t c, double E0) {
  a.Eprev[c] = E0;
  if (a.Ec) a.Ec[c * (int64_t)a.Lc] = E0;
  if (a.dEc) a.dEc[c * (int64_t)a.Lc] = 0.0;
}

}  // namespace hmc
