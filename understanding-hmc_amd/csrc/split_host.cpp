// split_host.cpp — host-only program (no HIP) behind hmc_philox_split.hpp for
// tests/test_philox_split_host.py: reads lines "seed chain iteration pair" (decimal or 0x..., 64-bit
// seed and chain) from stdin and prints the four words of each block, formed the way the four-chain
// kernel forms them: the pair's table entry from (pair, chain hi, seed hi), the lane's two words from
// (chain lo, seed lo), then split_block.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "hmc_philox_split.hpp"

int main() {
  char s[4][64];
  while (std::scanf("%63s %63s %63s %63s", s[0], s[1], s[2], s[3]) == 4) {
    const uint64_t seed = std::strtoull(s[0], nullptr, 0), chain = std::strtoull(s[1], nullptr, 0);
    const uint32_t iter = (uint32_t)std::strtoull(s[2], nullptr, 0), pair = (uint32_t)std::strtoull(s[3], nullptr, 0);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t a, b;
    hmc::split_lane_words((uint32_t)chain, k0, a, b);
    const hmc::uint4 r = hmc::split_block(hmc::split_entry(pair, (uint32_t)(chain >> 32), k1), a, b, iter, k0, k1);
    std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", r.x, r.y, r.z, r.w);
  }
  return 0;
}
