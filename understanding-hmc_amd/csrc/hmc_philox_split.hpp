// hmc_philox_split.hpp — Philox4x32-10 of a momentum block with rounds 1–2 split by what they depend on.
//
// The counter of a momentum block is (pair k, iteration, chain lo, chain hi).  Of the four products
// of rounds 1 and 2,
//   round 1:  k * M0                                 depends on the pair only,
//             glo * M1                               on the chain only (loop-invariant per lane),
//   round 2:  (hi(k M0) ^ ghi ^ k1) * M1             on the pair, the seed and the chain's high word,
//             (hi(glo M1) ^ k0 ^ iter) * M0          the only one that needs the iteration.
// A table holds, per pair, the third product and round 2's other pair-only word; a lane keeps the
// two words of its chain; a block then costs one xor with the iteration, one product and two xors
// before rounds 3–10.  split_block(split_entry(k, ghi, k1), a, b, iter, k0, k1) with (a, b) from
// split_lane_words(glo, k0) is draw_block(k, iter, ghi:glo, k0, k1), word for word.
//
// Compiles for the device (hipcc: xor3 and philox_rounds of hmc_device.hpp) and for a host-only
// program (split_host.cpp: the same statements over plain C++ restatements of the two).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include "hmc_device.hpp"
#define HMC_SPLIT_FN __device__ __forceinline__
#else
#define HMC_SPLIT_FN inline
#endif

namespace hmc {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

#ifndef __HIPCC__
struct uint4 {
  uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline uint32_t xor3(uint32_t a, uint32_t b, uint32_t k) { return a ^ b ^ k; }
template <int ROUNDS>
inline uint4 philox_rounds(uint4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < ROUNDS; ++r) {
    const uint64_t p0 = (uint64_t)c.x * kPhiloxM0;
    const uint64_t p1 = (uint64_t)c.z * kPhiloxM1;
    c = make_uint4(xor3((uint32_t)(p1 >> 32), c.y, k0), (uint32_t)p1, xor3((uint32_t)(p0 >> 32), c.w, k1),
                   (uint32_t)p0);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}
#endif

// Table entry of pair k, three words padded to 16 B (one ds_read_b128):
//   x, y = hi, lo of (hi(k M0) ^ ghi ^ k1) * M1      round 2's product of round 1's word z
//   z    = lo(k M0) ^ (k1 + W1)                      round 1's word w with round 2's key
HMC_SPLIT_FN uint4 split_entry(uint32_t k, uint32_t ghi, uint32_t k1) {
  const uint64_t p0 = (uint64_t)k * kPhiloxM0;
  const uint64_t r1 = (uint64_t)((uint32_t)(p0 >> 32) ^ ghi ^ k1) * kPhiloxM1;
  return make_uint4((uint32_t)(r1 >> 32), (uint32_t)r1, (uint32_t)p0 ^ (k1 + kPhiloxW1), 0u);
}

// The lane's two loop-invariant words: a = hi(glo M1) ^ k0 (round 1's word x before the iteration),
// b = lo(glo M1) ^ (k0 + W0) (round 1's word y with round 2's key).
HMC_SPLIT_FN void split_lane_words(uint32_t glo, uint32_t k0, uint32_t& a, uint32_t& b) {
  const uint64_t p1 = (uint64_t)glo * kPhiloxM1;
  a = (uint32_t)(p1 >> 32) ^ k0;
  b = (uint32_t)p1 ^ (k0 + kPhiloxW0);
}

// The block of (pair, iter, chain) from the pair's entry and the chain's words: four instructions
// for rounds 1–2, then rounds 3–10 with the keys two steps on.
HMC_SPLIT_FN uint4 split_block(uint4 e, uint32_t a, uint32_t b, uint32_t iter, uint32_t k0, uint32_t k1) {
  const uint64_t r0 = (uint64_t)(a ^ iter) * kPhiloxM0;
  const uint4 c = make_uint4(e.x ^ b, e.y, (uint32_t)(r0 >> 32) ^ e.z, (uint32_t)r0);
  return philox_rounds<8>(c, k0 + 2u * kPhiloxW0, k1 + 2u * kPhiloxW1);
}

}  // namespace hmc
