// hmc_diag_stream.hip — streaming (windowed) split-chain statistics: q_chain never has to be
// stored whole (k_stream_prod, k_stream_diff, behind hmc_stream_accumulate).
//
// Sample position p (0-based over q_chain[:, 1:, :]) lies in split half h = p / n at offset
// s = p - h*n (positions >= 2n are not part of any split chain, utils.py:102-104).  A call
// consumes `rows` new samples (positions pos0 ...) from a circular window of `wrap` rows per
// chain: the k-th sample from position pos0 - carry sits in window row (slot0 + k) % wrap.
// carry >= min(T, pos0) keeps every lag t <= T exact.
#include "hmc_diag.hpp"

namespace hmc {

namespace {

struct StreamArgs {
  const double* x;
  int64_t n_chains, chain_stride, sample_stride;
  int D, wrap, slot0, carry, rows, n;
  int64_t pos0;
  double* shift;  // [n_chains][2][D] first sample of each half (variance shift)
  double* s1;     // [n_chains][2][D] sum (x - shift)
  double* s2;     // [n_chains][2][D] sum (x - shift)^2
  double* vpart;  // [groups][T][D] partial variogram sums over this block's chains
  int groups;
};

constexpr int kStreamChunk = 8;   // window rows loaded together (memory-level parallelism)
#ifndef HMC_STREAM_PF
#define HMC_STREAM_PF 8              // rows in flight per wave in k_stream_prod (rolling prefetch)
#endif

// Block = 4 chain lanes x 64 dims (lane = dim: coalesced rows).  Each thread walks its chains'
// new rows once, with the last T samples in a register ring.  Two forms of the lag sums:
//  * product form (halves of n >= T samples, k_stream_prod below): the product form of
//    k_conv_series, ONE FMA per lag and row, V_t = 2 S2 - H_t - T_t - 2 C_t over shifted samples
//    y = x - shift.  The ring is zeroed when a half starts (so no product crosses halves) and the
//    other terms are three per-half events, all at static register indices: at position T-1 the
//    ring holds y[T-1..0] (H_t), at n-1 it holds the half's last T samples (T_t), and 2 S2 is added
//    once the half is complete.  vsum thus holds the sums of every completed half.
//  * difference form (short halves, this kernel): per lag and row (x - x_{-t})^2 under a
//    same-half mask.
// T <= 16 capped at 168 registers: three waves per SIMD keep enough rows in flight.
template <int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(T <= 16 ? 3 : 1))) void k_stream_diff(StreamArgs a) {
  __shared__ double red[4][kDimTile];
  const int dl = threadIdx.x & (kDimTile - 1);
  const int rl = threadIdx.x / kDimTile;
  const int d = blockIdx.y * kDimTile + dl;
  const int64_t left = 2 * (int64_t)a.n - a.pos0;
  const int rows = (int)(left < a.rows ? (left > 0 ? left : 0) : a.rows);
  double v[T];
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = 0.0;
  if (d < a.D) {
    for (int64_t c = (int64_t)blockIdx.x * 4 + rl; c < a.n_chains; c += (int64_t)a.groups * 4) {
      const double* xc = a.x + c * a.chain_stride + d;
      auto at = [&](int k) {             // k-th window sample (k < carry + rows)
        int sl = a.slot0 + k;
        sl = sl >= a.wrap ? sl - a.wrap : sl;
        return xc[(int64_t)sl * a.sample_stride];
      };
      const int64_t o = c * 2 * a.D + d;
      double sh[2] = {a.shift[o], a.shift[o + a.D]};
      double m1[2] = {a.s1[o], a.s1[o + a.D]};
      double m2[2] = {a.s2[o], a.s2[o + a.D]};
      // the carry rows enter the ring as they are (the same-half mask below drops the lags that
      // would reach into the other half), older ones are zero
      double ring[T];
#pragma unroll
      for (int k = 0; k < T; ++k) ring[k] = (k < a.carry) ? at(a.carry - 1 - k) : 0.0;
      for (int i0 = 0; i0 < rows; i0 += kStreamChunk) {
        double xs[kStreamChunk];
#pragma unroll
        for (int j = 0; j < kStreamChunk; ++j) xs[j] = (i0 + j < rows) ? at(a.carry + i0 + j) : 0.0;
        // Whole chunk inside one split half with every lag <= T available (uniform over the
        // block): no same-half selects.  Same operations as the general path.
        const int64_t p0 = a.pos0 + i0;
        const int h0 = p0 >= a.n ? 1 : 0;
        const int64_t s0 = p0 - (int64_t)h0 * a.n;
        if (i0 + kStreamChunk <= rows && s0 >= T && s0 + kStreamChunk <= a.n) {
#pragma unroll
          for (int j = 0; j < kStreamChunk; ++j) {
            const double x = xs[j];
            const double e = x - sh[h0];
            m1[h0] += e;
            m2[h0] = __builtin_fma(e, e, m2[h0]);
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const double df = x - ring[t];
              v[t] = __builtin_fma(df, df, v[t]);
            }
#pragma unroll
            for (int k = T - 1; k > 0; --k) ring[k] = ring[k - 1];
            ring[0] = x;
          }
          continue;
        }
#pragma unroll
        for (int j = 0; j < kStreamChunk; ++j) {
          if (i0 + j >= rows) break;
          const double x = xs[j];
          const int64_t p = a.pos0 + i0 + j;
          const int h = p >= a.n ? 1 : 0;
          const int sidx = (int)(p - (int64_t)h * a.n);
          if (sidx == 0) sh[h] = x;
          const double e = x - sh[h];
          m1[h] += e;
          m2[h] = __builtin_fma(e, e, m2[h]);
#pragma unroll
          for (int t = 0; t < T; ++t) {
            const double df = x - ring[t];
            v[t] = (t < sidx) ? __builtin_fma(df, df, v[t]) : v[t];   // lag t+1 inside the same half
          }
#pragma unroll
          for (int k = T - 1; k > 0; --k) ring[k] = ring[k - 1];
          ring[0] = x;
        }
      }
      a.shift[o] = sh[0];
      a.shift[o + a.D] = sh[1];
      a.s1[o] = m1[0];
      a.s1[o + a.D] = m1[1];
      a.s2[o] = m2[0];
      a.s2[o + a.D] = m2[1];
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const double sum = block_sum4(red, rl, dl, v[t]);
    if (rl == 0 && d < a.D) a.vpart[((int64_t)blockIdx.x * T + t) * a.D + d] = sum;
    __syncthreads();
  }
}

// The product form (halves of n >= T samples) as its own kernel, T rows per unrolled chunk so that
// every ring slot is a static register: position p lives in slot p mod T (chunks start at
// multiples of T), so the lag products, the ring update and both per-half events (H_t at half
// position T-1, T_t at n-1) index the ring statically -- no ring shifts (T moves per row before).
// Rows arrive by a rolling prefetch (slot p mod PF; the load of row p + PF is issued as row p is
// consumed), so PF rows per wave are always in flight instead of one chunk at a time; a wave's rows
// are one chain's (buffer descriptor on the chain, row offsets in the scalar offset).  Same sums
// in the same order as the shifting-ring product path this kernel replaced: bit-identical results.
template <int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(T <= 16 ? 3 : 1))) void k_stream_prod(StreamArgs a) {
  constexpr int PF = T < HMC_STREAM_PF ? T : HMC_STREAM_PF;
  static_assert(T % PF == 0, "prefetch slots repeat per chunk");
  __shared__ double red[4][kDimTile];
  const int dl = threadIdx.x & (kDimTile - 1);
  const int rl = __builtin_amdgcn_readfirstlane(threadIdx.x / kDimTile);   // wave-uniform: one chain per wave
  const int d = blockIdx.y * kDimTile + dl;
  const int dd = d < a.D ? d : a.D - 1;            // lanes past D load a valid element, write nothing
  const int64_t left = 2 * (int64_t)a.n - a.pos0;
  const int rows = (int)(left < a.rows ? (left > 0 ? left : 0) : a.rows);
  const int64_t pos0 = a.pos0, pend = a.pos0 + rows;
  double v[T];
#pragma unroll
  for (int t = 0; t < T; ++t) v[t] = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * 4 + rl; c < a.n_chains; c += (int64_t)a.groups * 4) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(a.x + c * a.chain_stride), 0, -1, 0x00020000);
    auto at = [&](int k) -> double {                // k-th window sample (k < carry + rows)
      int sl = a.slot0 + k;
      sl = sl >= a.wrap ? sl - a.wrap : sl;
      return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                            rs, dd * 8, (int)(sl * a.sample_stride * 8), 0));
    };
    auto kpos = [&](int64_t p) { return (int)(a.carry + (p - pos0)); };
    const int64_t o = c * 2 * a.D + dd;
    const int hc = pos0 >= a.n ? 1 : 0;
    // the current half's shift and sums; the other half's as stored
    double csh = a.shift[o + hc * a.D], cm1 = a.s1[o + hc * a.D], cm2 = a.s2[o + hc * a.D];
    double sh0 = a.shift[o], m10 = a.s1[o], m20 = a.s2[o];
    const double sh1s = a.shift[o + a.D], m11s = a.s1[o + a.D], m21s = a.s2[o + a.D];
    const int sidx0 = (int)(pos0 - (int64_t)hc * a.n);
    // ring: carry samples of the same half, slot = position mod T
    const int lim = a.carry < sidx0 ? a.carry : sidx0;
    double ring[T];
#pragma unroll
    for (int sl = 0; sl < T; ++sl) {
      const int k = (int)(((pos0 - 1 - sl) % T + T) % T);   // pos0 - 1 - k = position in slot sl
      const int kk = a.carry - 1 - k;
      ring[sl] = at(kk > 0 ? kk : 0);               // unconditional, all issued before any use
    }
    __builtin_amdgcn_sched_barrier(0);              // (the scheduler serialised load -> use pairs)
#pragma unroll
    for (int sl = 0; sl < T; ++sl) {
      const int k = (int)(((pos0 - 1 - sl) % T + T) % T);
      ring[sl] = k < lim ? ring[sl] - csh : 0.0;
    }
    double xs[PF];
#pragma unroll
    for (int sl = 0; sl < PF; ++sl) {
      const int64_t p = pos0 + (((sl - pos0) % PF) + PF) % PF;   // the first row with p = sl mod PF
      xs[sl] = at(kpos(p < pend ? p : pos0));       // (unconditional: rows past the end are unused)
    }
    int nsl = (a.slot0 + kpos(pos0 + PF)) % a.wrap;   // window slot of the next row to prefetch
    const int64_t P0 = pos0 - ((pos0 % T) + T) % T;
    for (int64_t pc = P0; pc < pend; pc += T) {
      auto row = [&](auto j_c) {
        constexpr int j = decltype(j_c)::value;
        const int64_t p = pc + j;
        if (p >= pos0 && p < pend) {                  // uniform
          const double x = xs[j % PF];
          if (p + PF < pend) {                        // row p + PF: a running window slot (scalar;
            int sl = nsl;                             // precomputed per unrolled row they spilled)
            asm volatile("" : "+s"(sl));
            xs[j % PF] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                       rs, dd * 8, (int)(sl * a.sample_stride * 8), 0));
            nsl = sl + 1 == a.wrap ? 0 : sl + 1;
          }
          if (p == a.n) {                            // the call crosses into half 1
            sh0 = csh;
            m10 = cm1;
            m20 = cm2;
            csh = sh1s;
            cm1 = m11s;
            cm2 = m21s;
          }
          const int sidx = (int)(p < a.n ? p : p - a.n);
          if (sidx == 0) {                           // a half starts: its shift, an empty ring
            csh = x;
#pragma unroll
            for (int k = 0; k < T; ++k) ring[k] = 0.0;
          }
          const double y = x - csh;
          cm1 += y;
          cm2 = __builtin_fma(y, y, cm2);
          const double ym2 = -2.0 * y;
#pragma unroll
          for (int t = 0; t < T; ++t) v[t] = __builtin_fma(ym2, ring[(j - 1 - t + 2 * T) % T], v[t]);   // -2 C_t
          ring[j] = y;
          if (sidx == T - 1) {                       // the half's first T samples: H_t = sum_{s<t} y^2
            double q = 0.0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const double r = ring[(j - (T - 1) + t + T) % T];
              q = __builtin_fma(r, r, q);
              v[t] -= q;
            }
          }
          if (sidx == a.n - 1) {                     // its last T samples: T_t; then + 2 S2
            double q = 0.0;
            const double s2x2 = 2.0 * cm2;
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const double r = ring[(j - t + T) % T];
              q = __builtin_fma(r, r, q);
              v[t] += s2x2 - q;
            }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      static_for<T>(row);
    }
    if (d < a.D) {
      const bool crossed = pos0 < a.n && pend > a.n;
      if (hc == 1 || crossed) {
        a.shift[o + a.D] = csh;
        a.s1[o + a.D] = cm1;
        a.s2[o + a.D] = cm2;
      }
      if (hc == 0) {
        a.shift[o] = crossed ? sh0 : csh;
        a.s1[o] = crossed ? m10 : cm1;
        a.s2[o] = crossed ? m20 : cm2;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const double sum = block_sum4(red, rl, dl, v[t]);
    if (rl == 0 && d < a.D) a.vpart[((int64_t)blockIdx.x * T + t) * a.D + d] = sum;
    __syncthreads();
  }
}

}  // namespace

int64_t diag_stream_groups(int64_t n_chains) {
  const int64_t g = (n_chains + 3) / 4;
  return g < 1024 ? (g < 1 ? 1 : g) : 1024;
}

hipError_t launch_stream_accum(const double* x, int64_t n_chains, int64_t cs, int64_t ss, int D, int wrap, int slot0,
                               int carry, int rows, int64_t pos0, int n, double* shift, double* s1, double* s2, int T,
                               double* vpart, double* vsum, hipStream_t st) {
  if ((int64_t)wrap * ss * 8 >= 0x7FFFFFFF) return hipErrorInvalidValue;   // row offsets: 32-bit scalar offsets
  const int64_t groups = diag_stream_groups(n_chains);
  StreamArgs a{x, n_chains, cs, ss, D, wrap, slot0, carry, rows, n, pos0, shift, s1, s2, vpart, (int)groups};
  dim3 grid((unsigned)groups, (unsigned)((D + kDimTile - 1) / kDimTile));
  // the product form needs every half to reach position T-1 (its H_t event); both forms give the
  // same sums of every completed half, and a run keeps one form (n and T are fixed per run)
  const bool prod = n >= T;
  auto go = [&](auto t_c) {
    constexpr int TT = decltype(t_c)::value;
    if (prod) k_stream_prod<TT><<<grid, 256, 0, st>>>(a);
    else k_stream_diff<TT><<<grid, 256, 0, st>>>(a);
  };
  switch (T) {
    case 8: go(std::integral_constant<int, 8>{}); break;
    case 16: go(std::integral_constant<int, 16>{}); break;
    case 32: go(std::integral_constant<int, 32>{}); break;
    case 64: go(std::integral_constant<int, 64>{}); break;
    default: return hipErrorInvalidValue;
  }
  if (hipError_t e = hipGetLastError()) return e;
  return launch_colsum(vpart, groups, (int64_t)T * D, vsum, true, st);   // vsum[t][d] += sum over groups
}

}  // namespace hmc
