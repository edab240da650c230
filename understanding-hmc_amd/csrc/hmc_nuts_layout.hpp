// hmc_nuts_layout.hpp — where things live inside a NUTS workspace, stated once per kernel.
//
// Each NUTS kernel carves the caller's buffer `ws` into regions.  Only the slot vectors go through a
// bounded buffer descriptor; the cursors, queue words and momenta are plain pointers past them, so a
// size query, a launcher and a kernel that disagreed about an offset would write out of bounds
// silently.  All three take every region from the kernel's layout object: offsets in doubles from
// `ws`, and the total that the size queries return.  Plain integer arithmetic for host and device.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HMC_LAYOUT_FN __host__ __device__ inline
#else
#define HMC_LAYOUT_FN inline
#endif

namespace hmc {

// Philox momenta are drawn ahead of the tree kernel (k_nuts_momenta) for up to kNutsMomIters
// iterations per launch: a tree start then costs a 16-byte load per lane pair, issued with the
// chain's state loads, instead of ~23k clocks of Philox + Box-Muller that the whole wave waited
// for at every tree end (profiles/r03_c5_nuts_phases.json), and the tree kernel needs no
// Box-Muller tables in LDS.  Longer ranges run as several launches.
constexpr int kNutsMomIters = 32;

// hmc_nuts.hip, MT 16-dim tiles per chain:
//   slots    per wave (16 chain slots) nvec vectors of 16 MT doubles per slot, slot-contiguous
//   cursors  16 replay-tape cursors (int64) per wave, zeroed before a run's first launch
//   queue    zeroed before every launch: the unit counter (u64), a spare word, then from `done` the
//            per-chain iterations done (u32), padded to a multiple of 16 bytes
//   momenta  one 16 MT-double vector per (chain, iteration of the launch), chain-major, for
//            min(kNutsMomIters, mom_iters) iterations (mom_iters 0: replay or a full cov_p)
struct NutsTreeLayout {
  static constexpr int kFixedVecs = 10;          // live points and both ends, before the save slots
  static constexpr int kQueueHead = 2;           // u64 words of the queue block before `done`
  int64_t n;
  int MT, d_max, mom_iters;                      // computed on use, so a kernel pays for what it takes
  HMC_LAYOUT_FN int nvec() const { return kFixedVecs + 2 * (d_max + 1); }               // vectors per chain slot
  HMC_LAYOUT_FN int64_t wave_doubles() const { return (int64_t)nvec() * (4 * MT) * 64; }   // one wave's slot block
  HMC_LAYOUT_FN int64_t n_waves() const { return (n + 15) / 16; }                       // slot blocks
  // a region's size where another follows it (cursors in int64 words, the queue block in bytes), its offset
  HMC_LAYOUT_FN int64_t n_cursors() const { return n_waves() * 16; }
  HMC_LAYOUT_FN uint64_t queue_bytes() const { return (uint64_t)((16 + 4 * n + 15) / 16 * 16); }
  HMC_LAYOUT_FN int64_t slots(int64_t wave) const { return wave * wave_doubles(); }
  HMC_LAYOUT_FN int64_t cursors() const { return n_waves() * wave_doubles(); }
  HMC_LAYOUT_FN int64_t queue() const { return cursors() + n_cursors(); }
  HMC_LAYOUT_FN int64_t momenta() const { return queue() + (int64_t)(queue_bytes() / 8); }
  HMC_LAYOUT_FN int64_t total() const {
    return momenta() + n * (mom_iters < kNutsMomIters ? mom_iters : kNutsMomIters) * (16 * MT); }
  // vector of iteration i (0-based) of a launch of K iterations, from the start of `momenta`
  static HMC_LAYOUT_FN int64_t mom_vec(int64_t c, int K, int64_t i, int MT) { return (c * K + i) * (16 * MT); }
};

// hmc_nuts_lock.hip:
//   slots       blocks x 16 chain slots of nvec vectors of 64 kLockJ doubles (an instance with fewer
//               coordinates per lane, J, packs its slots closer: nvec vectors of 64 J doubles)
//   pf, mf, cf  fragments of the precision, and with a full cov_p of inv_cov_p and chol(cov_p)
//   queue       next chain of the launch (u64, zeroed per launch), a spare word
//   cursors     one replay-tape cursor (int64) per chain
// mass: the size query passes true wherever the call may bring a full cov_p (the larger fragment
// count); a launch passes what its arguments say.
constexpr int kLockW = 16;        // chain slots (waves) per block
constexpr int kLockJ = 5;         // coordinates per lane: D <= 64 * kLockJ
struct NutsLockLayout {
  static constexpr int kFixedVecs = 8;           // both ends and the live points, before the save slots
  int NT, KS, F;                                 // output tiles (16 rows), k-steps (4), fragments NT * KS
  int64_t blocks;                                // slot blocks the workspace holds
  int64_t pf, mf, cf, queue, cursors, total;
  static HMC_LAYOUT_FN int nvec(int d_max) { return kFixedVecs + 2 * (d_max + 1); }
  // a slot per chain, in whole blocks: at least one, at most 1024
  static HMC_LAYOUT_FN int64_t slot_blocks(int64_t b) { return b < 1 ? 1 : b < 1024 ? b : 1024; }
  HMC_LAYOUT_FN NutsLockLayout(int64_t n, int D, int d_max, bool mass)
      : NT((D + 15) / 16), KS((D + 3) / 4), F(NT * KS), blocks(slot_blocks((n + kLockW - 1) / kLockW)),
        pf(blocks * kLockW * nvec(d_max) * 64 * kLockJ), mf(pf + (int64_t)F * 64), cf(mf + (int64_t)F * 64),
        queue(pf + (int64_t)F * 64 * (mass ? 3 : 1)), cursors(queue + 2), total(cursors + n) {}
};

// hmc_nuts_big.hip: per chain nvec vectors of Dp doubles (D padded to 64), the last two the full-cov_p
// scratch; then one tape cursor (int64) per chain.  The kernel rebuilds the object from nvec and Dp.
struct NutsChainLayout {
  static constexpr int kFixedVecs = 11;          // three (q, p, g) triples and the live points
  int64_t n;
  int nvec, Dp;
  static HMC_LAYOUT_FN NutsChainLayout of(int64_t n, int D, int d_max) { return {n, kFixedVecs + 2 * (d_max + 1) + 2, (D + 63) / 64 * 64}; }
  HMC_LAYOUT_FN int scratch() const { return nvec - 2; }
  HMC_LAYOUT_FN int64_t chain(int64_t c) const { return c * (int64_t)nvec * Dp; }
  HMC_LAYOUT_FN int64_t cursors() const { return chain(n); }
  HMC_LAYOUT_FN int64_t total() const { return cursors() + n; }
};

// hmc_glm_nuts.hip, MT 16-dim tiles per chain: per 16-chain tile nvec vectors of 16 MT x 16
// doubles, tile-interleaved; then 16 replay-tape cursors (int64) per tile.
struct GlmNutsLayout {
  static constexpr int kFixedVecs = 8;           // live points and both ends, before the save slots
  int nvec;
  int64_t tiles, tile_doubles, cursors, total;
  HMC_LAYOUT_FN GlmNutsLayout(int64_t n, int MT, int d_max)
      : nvec(kFixedVecs + 2 * (d_max + 1)), tiles((n + 15) / 16), tile_doubles((int64_t)nvec * (4 * MT) * 64),
        cursors(tiles * tile_doubles), total(cursors + tiles * 16) {}
  HMC_LAYOUT_FN int64_t slots(int64_t tile) const { return tile * tile_doubles; }
};

}  // namespace hmc

#undef HMC_LAYOUT_FN
