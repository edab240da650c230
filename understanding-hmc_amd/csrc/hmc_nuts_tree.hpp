// hmc_nuts_tree.hpp — the per-chain scalar bookkeeping of the reference's NUTS tree
// (samplers.py:595-791, utils.py:222-385), written once for the three NUTS kernels: hmc_nuts.hip
// (D <= 128, 16 chains per wave), hmc_nuts_lock.hip (128 < D <= 320, lockstep blocks) and
// hmc_nuts_big.hip (beyond, one wave per chain).  Those differ in how a chain's vectors are held and
// how its gradient is computed; everything here is independent of that and works on per-lane values
// (in hmc_nuts.hip they are per lane, not wave-uniform).
//
// The integer part (save_slot, CheckPoints) also compiles for the host: nuts_tree_host.cpp prints it
// and tests/test_oracle.py compares the printout with check_points of hmc_amd/utils.py.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include "hmc_device.hpp"
#include "hmc_internal.hpp"
#include "hmc_random_iter.hpp"   // stores_row: the row rule shared with the Random kernels
#define HMC_TREE_FN __host__ __device__ __forceinline__
#else
#define HMC_TREE_FN inline
#endif

namespace hmc {

// Save slot of odd point l of a sub-tree.  The reference keeps the saved odd points in a table
// (utils.py:222-385: next free entry, lookup by value, release) and looks them up by value.
// A saved point l is only ever checked as the first point of an aligned block of size s | (l - 1)
// ending at an even point m <= l + lowbit(l - 1) - 1, so two points with the same level
// ctz(l - 1) are never needed at the same time: slot = ctz(l - 1) (point 1, the start of every
// block, gets slot d_max) holds exactly the points the table would hold when they are checked,
// with no search and no releases.  Slots 0 .. d_max: d_max + 1 (q, p) pairs per chain.
HMC_TREE_FN int save_slot(int l, int d_max) { return l == 1 ? d_max : __builtin_ctz(l - 1); }

// check_points(m) of utils.py:246-283 for even m >= 2: the first point of every aligned
// power-of-two block (size >= 2) that ends at m, smallest start first.  The largest such block has
// the size of m's lowest set bit (the reference strips m's leading bits until a power of two is
// left), the others halve it down to 2, so the last point is always m - 1.
//   for (CheckPoints cp(m);;) { use(cp.pt); if (!cp.next()) break; }
struct CheckPoints {
  int pt, half;   // the current check point; the size of its block
  HMC_TREE_FN explicit CheckPoints(int m) : pt(m - (m & -m) + 1), half(m & -m) {}
  HMC_TREE_FN int count() const { return 31 - __builtin_clz(half); }   // points from pt on: log2(half)
  HMC_TREE_FN bool next() {                                            // advance; false when done
    if (half <= 2) return false;
    half >>= 1;
    pt += half;
    return true;
  }
};

// The same two quantities as the reference computes them (strip m's leading bits until a power of
// two or 2 is left; halve down to 2), for hmc_nuts.hip alone: its converged check loop keeps the
// incremental pt / half scalars it had, and with the closed forms above six of its 64 instances,
// all of them already spilling, gained scratch.  nuts_tree_host.cpp checks the two spellings
// against each other for every even m it prints.
HMC_TREE_FN int cp_r(int m) {          // CheckPoints(m).half
  int r = m;
  while ((r & (r - 1)) != 0 && r > 2) r -= 1 << (31 - __builtin_clz(r));
  return r;
}
HMC_TREE_FN int cp_count(int m) {      // CheckPoints(m).count()
  const int r = cp_r(m);
  int cnt = 1, half = r;
  while (half > 2) {
    half >>= 1;
    ++cnt;
  }
  return cnt;
}

#ifdef __HIPCC__

// The tree's loop-carried scalars stay plain variables of each kernel, declared where they were,
// and the helpers below hold no state: the weights go in by value and come back in a small
// result, the draw counters go in by reference.  Members of a struct object are promoted to
// registers ahead of a kernel's other scalars, which reorders the loop header and costs the
// kernels at their register cap scratch (lockstep kernel, D > 192: 8 bytes per lane for a
// TreeWeights object, more SGPR spills for a NutsDraws object).

// Progressive multinomial sampling inside the new sub-tree (:743-751) and the biased sub-tree
// acceptance (:766-771, Q11) on the kernel's four weights, each relative to a running energy
// maximum: E_max_now, pi_new of the new sub-tree (its first point sets E_max_now = E, pi_new = 1,
// :618-619) and E_max_old, pi_old of the tree so far (E_initial and 1 at an iteration's start,
// :586-587).
struct TreeWeights {
  // a later point of the sub-tree with energy E_tmp: the ratio r it replaces the live point with.
  // The reference takes exp(-(E_tmp - E_max_now)) and exp(E_max_now - E_max_prev): one argument is
  // exactly 0 (E_max_now is one of E_tmp, E_max_prev), so ONE_EXP takes one exp and exp(0) = 1,
  // 1 * x = x: bit-equal to the reference's two (NaN energies give the same NaN r as the two exps).
  // hmc_nuts.hip, whose energies are per lane, takes that form.  ONE_EXP = false writes the two
  // out, for the two kernels whose energies are wave-uniform: the one-exp form holds about 18
  // VGPRs more there.  The lockstep kernel, at its 128-register cap, gains 44 to 80 bytes of
  // scratch per lane in 14 of its 16 instances with it (all but the replay instances of D <= 192
  // with a diagonal cov_p), which costs more than the exp saves; the per-chain kernel needs 94 to
  // 124 VGPRs with it and 74 to 106 without (one more wave per SIMD in replay mode).
  struct Added { double E_max_now, pi_new, r; };
  template <bool ONE_EXP = true>
  static __device__ __forceinline__ Added add_point(double E_max_prev, double pi_new, double E_tmp) {
    const double E_max_now = fmax(E_max_prev, E_tmp);
    double num, w_old;   // weights of the new point and of the points so far, relative to E_max_now
    if constexpr (ONE_EXP) {
      const bool up = E_max_now != E_max_prev;
      const double e = exp(up ? E_max_now - E_max_prev : -(E_tmp - E_max_now));
      num = up ? 1.0 : e;
      w_old = up ? e : 1.0;
    } else {
      num = exp(-(E_tmp - E_max_now));
      w_old = exp(E_max_now - E_max_prev);
    }
    pi_new = num + w_old * pi_new;
    return {E_max_now, pi_new, num / pi_new};
  }
  // sub-tree end: min(1, r) of the new sub-tree against the old tree; the old tree absorbs it.
  // (operation order as the reference's: replay parity compares energies to 1e-10)
  struct Merged { double E_max_old, pi_old, A; };
  static __device__ __forceinline__ Merged merge(double E_max_now, double pi_new, double E_max_old_prev, double pi_old) {
    const double r = exp(-(E_max_now - E_max_old_prev)) * pi_old / pi_new;   // :766
    const double E_max_old = fmax(E_max_old_prev, E_max_now);
    pi_old = exp(-(E_max_now - E_max_old)) * pi_new + exp(-(E_max_old_prev - E_max_old)) * pi_old;   // :771
    return {E_max_old, pi_old, fmin(1.0, r)};
  }
};

// The tree's random numbers in the reference's order of consumption: directions (:608) and
// uniforms (:750, :773).  A kernel's draw(direction) calls tape() in replay mode and philox()
// otherwise, each on the kernel's own counters, and names nothing the other mode uses.
struct NutsDraws {
  // replay: the chain's tape as is, cursor tpos (persists across launches); an exhausted tape gives
  // 0.0 for a direction and 2.0 for a uniform and is counted in n_tape (the host raises)
  static __device__ __forceinline__ double tape(int64_t& tpos, const RandArgs& a, unsigned long long& n_tape, int64_t c,
                                                bool direction) {
    if (tpos >= a.tape_stride) {
      ++n_tape;
      return direction ? 0.0 : 2.0;
    }
    return a.tape[c * a.tape_stride + (tpos++)];
  }
  // Philox: draw ndraw (reset at an iteration's start) of iteration it of global chain gc is block
  // kDrawSlot + ndraw, direction = bit 0 of .x, uniform = u53(.z, .w)
  template <typename N>
  static __device__ __forceinline__ double philox(N& ndraw, int it, uint64_t gc, const RandArgs& a, bool direction) {
    const uint4 r = draw_block(kDrawSlot + (uint32_t)(ndraw++), (uint32_t)it, gc, a.k0, a.k1);
    return direction ? (double)(r.x & 1u) : u53(r.z, r.w);
  }
};

// row of the counter block that a kernel's slot index (wave, chain) adds to
__device__ __forceinline__ unsigned long long* nuts_counter_row(unsigned long long* cnt, int64_t slot_index) {
  return cnt + (slot_index & (HMC_COUNTER_SLOTS - 1)) * HMC_NCOUNTERS;
}

// End-of-kernel counter flush of one lane: leapfrogs (also the energy evaluations), unstable
// sub-trees, iterations stopped at d_max, draws past the replay tape (HMC_CNT_OOB_REJECT) and
// n_steps into HMC_CNT_LEAPFROG_SQ; zero tallies are skipped.  The caller picks the counter row and
// what a step is:
//   hmc_nuts.hip       row of the wave,         n_steps = wave steps (16 chain slots each; with the
//                                               leapfrogs: lane utilisation)
//   hmc_nuts_lock.hip  row of the (block, wave), n_steps = block steps (16 chain slots each), counted
//                                               by wave 0
//   hmc_nuts_big.hip   row of the chain,        n_steps = the chain's leapfrogs (one chain per wave)
__device__ __forceinline__ void nuts_flush_counters(unsigned long long* cnt, int64_t slot_index,
                                                    unsigned long long n_lf, unsigned long long n_unst,
                                                    unsigned long long n_dmax, unsigned long long n_tape,
                                                    unsigned long long n_steps) {
  if (!cnt) return;
  unsigned long long* cs = nuts_counter_row(cnt, slot_index);
  if (n_lf) {
    atomicAdd(cs + HMC_CNT_LEAPFROG, n_lf);
    atomicAdd(cs + HMC_CNT_ENERGY_EVALS, n_lf);
  }
  if (n_unst) atomicAdd(cs + HMC_CNT_UNSTABLE, n_unst);
  if (n_dmax) atomicAdd(cs + HMC_CNT_DMAX, n_dmax);
  if (n_tape) atomicAdd(cs + HMC_CNT_OOB_REJECT, n_tape);
  if (n_steps) atomicAdd(cs + HMC_CNT_LEAPFROG_SQ, n_steps);
}

#endif  // __HIPCC__

}  // namespace hmc

#undef HMC_TREE_FN
