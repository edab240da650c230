// hmc_debug.hpp — the profiling hooks of the debug build (make debug -> lib/libhmc_debug.so,
// -DHMC_DEBUG_HOOKS), stated once.  The debug library reads HMC_DEBUG_ABLATE,
// HMC_DEBUG_L, HMC_DEBUG_STAMPS, HMC_FORCE_K and HMC_KERNEL; in the release libhmc.so, which the
// product and bench.py load, everything here is a constant or an empty inline and the kernels
// compile none of it.  Apart from RandArgs' debug members this is the only file that tests
// HMC_DEBUG_HOOKS.
#pragma once
#include "hmc_internal.hpp"

namespace hmc {

constexpr int kStampWords = 16;   // phase-timer words per wave (HMC_DEBUG_STAMPS)

// HMC_DEBUG_ABLATE bits: each takes one part out of the Random iteration kernels (timing only, the
// samples are then wrong).  1..16 act in the lane-group kernel (hmc_random.hip), 32..256 and
// HMC_DEBUG_L in the FULL instances of the wave kernel (hmc_wave.hip).
enum Ablate : int {
  kAblateMomentum = 1,      // constant momentum instead of the draw
  kAblateEnergy = 2,        // no energies
  kAblateZeroL = 4,         // L = 0
  kAblateRowStores = 8,     // no row stores (lane-group kernel)
  kAblateL12 = 16,          // L = 12
  kAblateCapture = 32,      // no chain-0 capture
  kAblateQStore = 64,       // no q row store (wave kernel)
  kAblateRestore = 128,     // no restore on rejection
  kAblateNextDraw = 256,    // no next-momentum draw
};

#ifdef HMC_DEBUG_HOOKS

__device__ __forceinline__ bool ablate(const RandArgs& a, Ablate bit) { return (a.dbg & bit) != 0; }
__host__ __device__ __forceinline__ int forced_L(const RandArgs& a) { return a.dbgL; }   // HMC_DEBUG_L, or -1
__device__ __forceinline__ unsigned long long* stamps(const RandArgs& a) { return a.stamps; }

bool instrumented();   // HMC_DEBUG_ABLATE or HMC_DEBUG_L set: the launch takes the FULL instances
void apply_env(RandArgs& a, const Layout& lay, int64_t n_chains);   // the HMC_DEBUG_* variables into a
int force_K();        // HMC_FORCE_K: the pairs-per-lane template to force (0: none)
bool force_group();   // HMC_KERNEL=group: the lane-group kernel where the wave kernel would run

#else

__device__ __forceinline__ constexpr bool ablate(const RandArgs&, Ablate) { return false; }
__host__ __device__ __forceinline__ constexpr int forced_L(const RandArgs&) { return -1; }
__device__ __forceinline__ constexpr unsigned long long* stamps(const RandArgs&) { return nullptr; }

constexpr bool instrumented() { return false; }
inline void apply_env(RandArgs&, const Layout&, int64_t) {}
constexpr int force_K() { return 0; }
constexpr bool force_group() { return false; }

#endif

// Phase timers: N accumulators of wave-uniform s_memtime deltas, fed by CLOCKS independent clocks,
// and written by store() to the wave's row of the stamp buffer (kStampWords words, vector stores).
// start(k) restarts clock k, lap(i, k) adds the time since clock k's last start or lap to slot i,
// count(i) uses slot i as a plain counter.  Off (no reads, zeros) unless HMC_DEBUG_STAMPS is set.
//
// Stamp row of hmc_random.hip's k_random_iters (PhaseTimer<6>), summed over the launch's iterations:
//   0 momentum draw, 1 E0, 2 row bookkeeping + L/u draw, 3 leapfrog loop, 4 E1, 5 MH + stores
//   (low 16 bits; bits 16..31 XCC_ID, high word HW_ID: stamp_hw_id), 6 t_start, 7 t_end.
// Stamp row of hmc_nuts.hip's k_nuts_iters (PhaseTimer<14, 2>), per part of a wave step summed over
// the launch.  Clock 0, the parts of a step: 0 transitions, 1 half kick + drift, 2 gradient (MFMA),
// 3 half kick + energies, 4 new-point bookkeeping / saves, 5 loaded U-turn checks, 6 progressive
// sampling, 7 sub-tree end.  Clock 1, inside part 0: 8 tree end (live point, row), 9 write-back +
// drain + publish, 10 queue reservation, 11 poll + state loads, 12 momentum + tree start.  13 counts
// the wave steps with a tree end.
template <int N, int CLOCKS = 1>
struct PhaseTimer {
  static_assert(N <= kStampWords, "a stamp row holds kStampWords words");
#ifdef HMC_DEBUG_HOOKS
  unsigned long long* const out;
  unsigned long long ph[N] = {}, t[CLOCKS] = {};
  __device__ __forceinline__ explicit PhaseTimer(const RandArgs& a) : out(stamps(a)) {}
  __device__ __forceinline__ bool on() const { return out != nullptr; }
  __device__ __forceinline__ unsigned long long now() const { return out ? __builtin_amdgcn_s_memtime() : 0ull; }
  __device__ __forceinline__ void start(int k = 0) { t[k] = now(); }
  __device__ __forceinline__ void lap(int i, int k = 0) {
    const unsigned long long t_ = now();
    ph[i] += t_ - t[k];
    t[k] = t_;
  }
  __device__ __forceinline__ void count(int i) { ++ph[i]; }
  __device__ __forceinline__ unsigned long long* store(int64_t wave) const {   // call with on()
    unsigned long long* row = out + wave * kStampWords;
#pragma unroll
    for (int i = 0; i < N; ++i) row[i] = ph[i];
    return row;
  }
#else
  __device__ __forceinline__ explicit PhaseTimer(const RandArgs&) {}
  __device__ __forceinline__ static constexpr bool on() { return false; }
  __device__ __forceinline__ static constexpr unsigned long long now() { return 0ull; }
  __device__ __forceinline__ void start(int = 0) {}
  __device__ __forceinline__ void lap(int, int = 0) {}
  __device__ __forceinline__ void count(int) {}
  __device__ __forceinline__ unsigned long long* store(int64_t) const { return nullptr; }
#endif
};

// Where the wave ran: HW_ID (wave / simd / cu / sh / se) into the high word of *w and XCC_ID into
// bits 16..31; the low 16 bits of *w stay.
__device__ __forceinline__ void stamp_hw_id(unsigned long long* w) {
#ifdef HMC_DEBUG_HOOKS
  const unsigned hwid = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  *w = ((unsigned long long)hwid << 32) | ((unsigned long long)(xcc & 0xffff) << 16) | (*w & 0xffffull);
#endif
}

}  // namespace hmc
