// hmc_select.hpp — exact order statistics by radix select (hmc_select.hip, hmc_select_* and
// hmc_order_stats): what the host and the device share.  Three rules are stated here once:
//   select_key      the order-preserving map of a double to uint64: every bit of a negative value
//                   flipped, only the sign bit of a non-negative one; every NaN (either sign, any
//                   payload) becomes the largest key, so NaNs sort last as np.sort puts them
//   select_unkey    its inverse (the largest key gives the canonical quiet NaN)
//   select_pick     one pass's choice: the digit whose bin holds the remaining rank, and the rank
//                   that remains inside that bin
// The kernels, select_host.cpp (which prints them for tests/test_select_host.py) and nothing else
// compile them.  The launch geometry is stated here once too, as a function of the shapes alone.
//
// State: one record of HMC_SELECT_STATE_STRIDE int64 words per (dimension, rank), [D][T]:
//   0 prefix     the key's top 8 * pass bits fixed so far, right-aligned (the key after the last pass)
//   1 remaining  the rank that remains among the elements whose key starts with the prefix
//   2 owner      the lowest rank index of this dimension with the same prefix: the count step adds
//                into the owner's bins only and the pick step reads them for every rank that shares
//   3 padding, written 0 by init: a record is 32 bytes, so that none straddles a 64-byte line and
//     record i starts at state + 32 i
//
// select_host.cpp defines HMC_SELECT_HOST_ONLY: no HIP header, no launcher.
#pragma once
#include <stdint.h>

#include "hmc.h"

#ifndef HMC_SELECT_HOST_ONLY
#include <hip/hip_runtime.h>
#endif
#if defined(__HIPCC__) && !defined(HMC_SELECT_HOST_ONLY)
#define HMC_SEL_FN __host__ __device__ __forceinline__
#else
#define HMC_SEL_FN inline
#endif

namespace hmc {

constexpr int kSelBits = HMC_SELECT_BITS;
constexpr int kSelBins = 1 << kSelBits;
constexpr int kSelPasses = 64 / kSelBits;
static_assert(kSelBits * kSelPasses == 64, "HMC_SELECT_BITS must divide 64");

constexpr uint64_t kSelSign = 0x8000000000000000ull;
constexpr uint64_t kSelNanKey = 0xFFFFFFFFFFFFFFFFull;

HMC_SEL_FN uint64_t select_key_bits(uint64_t b) {
  if ((b & ~kSelSign) > 0x7FF0000000000000ull) return kSelNanKey;   // NaN of either sign
  return (b & kSelSign) ? ~b : (b ^ kSelSign);
}

HMC_SEL_FN uint64_t select_unkey_bits(uint64_t k) {
  if (k == kSelNanKey) return 0x7FF8000000000000ull;
  return (k & kSelSign) ? (k ^ kSelSign) : ~k;
}

HMC_SEL_FN uint64_t select_key(double x) { return select_key_bits(__builtin_bit_cast(uint64_t, x)); }
HMC_SEL_FN double select_unkey(uint64_t k) { return __builtin_bit_cast(double, select_unkey_bits(k)); }

// The digit d with c[0] + .. + c[d-1] <= r < c[0] + .. + c[d] and, in *r_out, r - (c[0] + .. + c[d-1]).
// Empty bins are never chosen.  r at or past the total (no caller passes one) gives the last bin.
HMC_SEL_FN int select_pick(const int64_t* c, int nbins, int64_t r, int64_t* r_out) {
  int64_t below = 0;
  int d = 0;
  for (; d < nbins - 1; ++d) {
    const int64_t next = below + c[d];
    if (r < next) break;
    below = next;
  }
  *r_out = r - below;
  return d;
}

// ---- launch geometry: a function of (D, n_samples) alone, never of the device
constexpr int kSelTile = 16;            // dimensions per block: one 128-byte line of a sample row
constexpr int kSelThreads = 1024;       // 16 waves; a wave reads 4 sample rows x 16 dimensions
constexpr int kSelRowsPerStep = kSelThreads / kSelTile;   // sample rows a block reads per step
constexpr int64_t kSelBlocks = 1024;    // the launch aims at this many blocks over all tiles ...
constexpr int64_t kSelMinPerBlock = 1024;   // ... of at least this many samples each
// A block's share of the samples never exceeds this, and a bin receives at most one increment per
// sample of its dimension: the 32-bit LDS counters cannot wrap.
constexpr int64_t kSelMaxPerBlock = (int64_t)1 << 31;
constexpr int64_t kSelMaxSamples = (int64_t)1 << 48;
constexpr int64_t kSelMaxTiles = 65535;                   // D <= 1,048,560
constexpr int64_t kSelMaxGrid = 0x7FFFFFFF;               // tiles x blocks per tile, one grid dimension

inline int64_t select_tiles(int64_t D) { return (D + kSelTile - 1) / kSelTile; }

// samples per block; the blocks per dimension tile follow from it
inline int64_t select_per_block(int64_t D, int64_t n_samples) {
  const int64_t tiles = select_tiles(D);
  const int64_t want = (kSelBlocks + tiles - 1) / tiles;
  int64_t per = (n_samples + want - 1) / want;
  per = per < kSelMinPerBlock ? kSelMinPerBlock : per;
  return per > kSelMaxPerBlock ? kSelMaxPerBlock : per;
}

inline int64_t select_blocks(int64_t D, int64_t n_samples) {
  if (D < 1 || select_tiles(D) > kSelMaxTiles || n_samples < 1 || n_samples > kSelMaxSamples) return 0;
  const int64_t per = select_per_block(D, n_samples);
  const int64_t blocks = (n_samples + per - 1) / per;
  return blocks * select_tiles(D) > kSelMaxGrid ? 0 : blocks;
}

inline int64_t select_state_words(int64_t D, int64_t T) { return D * T * HMC_SELECT_STATE_STRIDE; }
inline int64_t select_count_words(int64_t D, int64_t T) { return D * T * kSelBins; }

#if !defined(HMC_SELECT_HOST_ONLY)
struct SelectRanks {
  int64_t r[HMC_SELECT_MAX_RANKS];
};
hipError_t launch_select_init(int64_t* state, int D, int T, const SelectRanks& ranks, hipStream_t s);
// rows = samples per chain, n_samples = chains x rows (> 0); counts is zeroed first.
hipError_t launch_select_count(const hmc_samples& sm, int64_t rows, int64_t n_samples, int D, int T, int pass,
                               const int64_t* state, int64_t* counts, hipStream_t s);
hipError_t zero_select_counts(int64_t* counts, int D, int T, hipStream_t s);
hipError_t launch_select_pick(int D, int T, int64_t* state, const int64_t* counts, hipStream_t s);
hipError_t launch_select_values(int D, int T, const int64_t* state, double* out, hipStream_t s);
#endif

}  // namespace hmc

#undef HMC_SEL_FN
