// hmc_select.hip — exact order statistics of every dimension of a strided sample view by radix
// select (hmc_select_*, hmc_order_stats).  Most significant digit first, HMC_SELECT_BITS = 8 bits per
// pass, 8 passes over order-preserving uint64 keys (hmc_select.hpp).  Nothing is copied or sorted:
// a pass reads the view once and counts, for every (dimension, rank) target, the elements whose key
// starts with the target's prefix, by their next digit; a small kernel then picks each target's
// digit.  Counts are integers, so the result does not depend on the launch geometry, on the order
// of the atomics, or on how chains are split over shards (shards add their count tables).
//
// k_select_count: a block owns a tile of 16 dimensions (one 128-byte line of a sample row) and a
// contiguous range of samples.  Thread (dl = tid & 15, sub = tid >> 4) reads dimension dl of sample
// rows sub, sub + 64, ...: the 64 lanes of a wave read 4 rows x 16 dimensions, each row's line once,
// and lanes of different dimensions never meet in a histogram.  The block's histograms live in LDS
// as 32-bit counters, [rank][digit][dl]: the 16 dimensions of one (rank, digit) sit in 16
// consecutive banks, so that dimensions whose values share a digit (every N(0, 1) column in the
// first passes) do not collide.  The 4 lanes of a wave that hold the same dimension add to the same
// address when their digits agree; nothing is done about that.  An element matches
// the prefix of the targets that still share it; only their owner (the lowest such rank, recorded
// by pick) counts, so an element costs at most one LDS atomic.  At the end the block adds its
// non-zero counters to counts[D][T][256] (int64) with integer atomics.
#include <hip/hip_runtime.h>

#include "hmc_select.hpp"

namespace hmc {

namespace {

struct SelectArgs {
  const double* q;
  const int64_t* state;       // [D][T] records
  int64_t* counts;            // [D][T][256]
  int64_t chain_stride, row_stride, row_begin, row_step;
  int64_t rows;               // samples per chain
  int64_t n_samples;          // chains x rows
  int64_t per_block;          // samples per block (<= kSelMaxPerBlock: 32-bit counters cannot wrap)
  int D, T, pass, tiles;
};

constexpr uint64_t kNoPrefix = ~0ull;
constexpr int kUnroll = 8;   // sample rows a lane requests before it counts the first

template <int TCAP>
__global__ void __launch_bounds__(kSelThreads) k_select_count(const SelectArgs a) {
  __shared__ uint32_t hist[TCAP * kSelBins * kSelTile];
  const int tid = threadIdx.x;
  const int dl = tid & (kSelTile - 1), sub = tid >> 4;
  const int T = a.T;
  // tiles vary fastest over the launch: the blocks that share a range of samples run together, so
  // that a line of a row that straddles two tiles is fetched from memory once
  const uint32_t tiles = (uint32_t)a.tiles;
  const uint32_t sblock = blockIdx.x / tiles;
  const int d0 = (int)(blockIdx.x - sblock * tiles) * kSelTile;
  const int d = d0 + dl;
  const bool dim_ok = d < a.D;

  for (int i = tid; i < T * kSelBins * kSelTile; i += kSelThreads) hist[i] = 0u;

  // the lane's targets: the prefixes of the ranks that count (owners); every other slot holds a
  // value no prefix takes (a prefix has at most 56 bits)
  uint64_t prefix[TCAP];
#pragma unroll
  for (int t = 0; t < TCAP; ++t) {
    prefix[t] = kNoPrefix;
    if (t < T && dim_ok) {
      const int64_t* rec = a.state + ((int64_t)d * T + t) * HMC_SELECT_STATE_STRIDE;
      prefix[t] = rec[2] == t ? (uint64_t)rec[0] : kNoPrefix;
    }
  }
  __syncthreads();

  const int pass = a.pass;
  const int sh_digit = 64 - kSelBits * (pass + 1);   // 56, 48, .. 0
  const int sh_pre = (sh_digit + kSelBits) & 63;      // pass 0: no prefix yet (shift 0, masked below)
  const uint64_t pre_mask = pass == 0 ? 0ull : ~0ull;

  auto add = [&](double x) {
    const uint64_t key = select_key(x);
    const uint64_t pre = (key >> sh_pre) & pre_mask;
    const uint32_t digit = (uint32_t)(key >> sh_digit) & (kSelBins - 1);
    int hit = -1;
#pragma unroll
    for (int t = 0; t < TCAP; ++t)
      hit = pre == prefix[t] ? t : hit;                             // owners' prefixes are distinct
    if (hit >= 0) atomicAdd(&hist[(((uint32_t)hit << kSelBits) + digit) * kSelTile + dl], 1u);
  };

  // ---- the block's samples [s0, s1); the thread takes s0 + sub, s0 + sub + 64, ...; r = the
  // row of its sample within its chain, advanced by 64 samples without a division
  const int64_t rows = a.rows;
  const int64_t s0 = (int64_t)sblock * a.per_block;
  const int64_t s1 = min(s0 + a.per_block, a.n_samples);
  const int64_t mine = s0 + sub;
  int64_t n_it = (dim_ok && mine < s1) ? (s1 - mine + kSelRowsPerStep - 1) / kSelRowsPerStep : 0;
  const int64_t q64 = kSelRowsPerStep / rows, rem64 = kSelRowsPerStep - q64 * rows;
  // off = the element's offset from q; 64 samples on is d64 further, and one chain on and `rows`
  // rows back when the row wraps
  const int64_t row_pitch = a.row_step * a.row_stride;
  const int64_t d64 = q64 * a.chain_stride + rem64 * row_pitch;
  const int64_t dwrap = a.chain_stride - rows * row_pitch;
  int64_t r = 0, off = 0;
  if (n_it > 0) {
    const int64_t c = mine / rows;
    r = mine - c * rows;
    off = c * a.chain_stride + a.row_begin * a.row_stride + r * row_pitch + d;
  }
  auto addr = [&]() { return a.q + off; };
  auto step = [&]() {
    r += rem64;
    off += d64;
    const bool w = r >= rows;
    r = w ? r - rows : r;
    off = w ? off + dwrap : off;
  };
#pragma unroll 1
  for (; n_it >= kUnroll; n_it -= kUnroll) {     // kUnroll loads in flight per lane
    double x[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      x[k] = __builtin_nontemporal_load(addr());
      step();
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) add(x[k]);
  }
#pragma unroll 1
  for (; n_it > 0; --n_it) {
    add(*addr());
    step();
  }
  __syncthreads();

  // ---- the block's non-zero counters into the table (a non-zero counter is a dimension < D)
  for (int i = tid; i < T * kSelBins * kSelTile; i += kSelThreads) {
    const uint32_t v = hist[i];
    if (v != 0u) {
      const int l = i & (kSelTile - 1), bin = i >> 4;               // bin = t * 256 + digit
      const int t = bin >> kSelBits, digit = bin & (kSelBins - 1);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + ((int64_t)(d0 + l) * T + t) * kSelBins + digit,
                (unsigned long long)v);
    }
  }
}

__global__ void __launch_bounds__(256) k_select_init(int64_t* state, int D, int T, const SelectRanks ranks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * T) return;
  int64_t* rec = state + (int64_t)i * HMC_SELECT_STATE_STRIDE;
  rec[0] = 0;
  rec[1] = ranks.r[i % T];
  rec[2] = 0;                // every rank shares the empty prefix
  rec[3] = 0;
}

// One thread per (dimension, rank): the owner's bins, the pick, then the new owners of the dimension.
constexpr int kPickDims = 256 / HMC_SELECT_MAX_RANKS;

__global__ void __launch_bounds__(256) k_select_pick(int D, int T, int64_t* state, const int64_t* counts) {
  __shared__ uint64_t pre[256];
  const int dl = threadIdx.x / T, t = threadIdx.x - dl * T;
  const int d = blockIdx.x * kPickDims + dl;
  const bool live = dl < kPickDims && d < D;
  int64_t* rec = state + ((int64_t)d * T + t) * HMC_SELECT_STATE_STRIDE;
  uint64_t np = 0ull;
  if (live) {
    const int owner = (int)rec[2];
    int64_t rem;
    const int digit = select_pick(counts + ((int64_t)d * T + owner) * kSelBins, kSelBins, rec[1], &rem);
    np = ((uint64_t)rec[0] << kSelBits) | (uint64_t)digit;
    rec[0] = (int64_t)np;
    rec[1] = rem;
    pre[threadIdx.x] = np;
  }
  __syncthreads();
  if (live) {
    int owner = t;
    for (int u = t - 1; u >= 0; --u) owner = pre[dl * T + u] == np ? u : owner;
    rec[2] = owner;
  }
}

__global__ void __launch_bounds__(256) k_select_values(int D, int T, const int64_t* state, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // i = d * T + t
  if (i >= D * T) return;
  const int d = i / T, t = i - d * T;
  out[(int64_t)t * D + d] = select_unkey((uint64_t)state[(int64_t)i * HMC_SELECT_STATE_STRIDE]);
}

}  // namespace

hipError_t launch_select_init(int64_t* state, int D, int T, const SelectRanks& ranks, hipStream_t s) {
  hipLaunchKernelGGL(k_select_init, dim3((unsigned)(((int64_t)D * T + 255) / 256)), dim3(256), 0, s, state, D, T,
                     ranks);
  return hipGetLastError();
}

hipError_t zero_select_counts(int64_t* counts, int D, int T, hipStream_t s) {
  return hipMemsetAsync(counts, 0, (size_t)select_count_words(D, T) * sizeof(int64_t), s);
}

hipError_t launch_select_count(const hmc_samples& sm, int64_t rows, int64_t n_samples, int D, int T, int pass,
                               const int64_t* state, int64_t* counts, hipStream_t s) {
  hipError_t e = zero_select_counts(counts, D, T, s);
  if (e != hipSuccess) return e;
  SelectArgs a{};
  a.q = sm.q;
  a.state = state;
  a.counts = counts;
  a.chain_stride = sm.chain_stride;
  a.row_stride = sm.row_stride;
  a.row_begin = sm.row_begin;
  a.row_step = sm.row_step;
  a.rows = rows;
  a.n_samples = n_samples;
  a.per_block = select_per_block(D, n_samples);
  a.D = D;
  a.T = T;
  a.pass = pass;
  a.tiles = (int)select_tiles(D);
  const dim3 grid((unsigned)(select_blocks(D, n_samples) * select_tiles(D)));
  const dim3 block(kSelThreads);
  if (T <= 1) hipLaunchKernelGGL((k_select_count<1>), grid, block, 0, s, a);
  else if (T <= 2) hipLaunchKernelGGL((k_select_count<2>), grid, block, 0, s, a);
  else if (T <= 4) hipLaunchKernelGGL((k_select_count<4>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_select_count<8>), grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_select_pick(int D, int T, int64_t* state, const int64_t* counts, hipStream_t s) {
  hipLaunchKernelGGL(k_select_pick, dim3((unsigned)((D + kPickDims - 1) / kPickDims)), dim3(256), 0, s, D, T, state,
                     counts);
  return hipGetLastError();
}

hipError_t launch_select_values(int D, int T, const int64_t* state, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_select_values, dim3((unsigned)(((int64_t)D * T + 255) / 256)), dim3(256), 0, s, D, T, state,
                     out);
  return hipGetLastError();
}

}  // namespace hmc
