// hmc_pred.hip — posterior-predictive and WAIC reductions of the GLM targets (hmc_glm_predictive).
//
// Z[j][s] = x_j . q_s for every evaluation row j and every stored sample s is never stored: a wave
// owns a tile of 16 evaluation rows, keeps their X fragments in registers as the A operand of
// v_mfma_f64_16x16x4 (4 MT doubles per lane, MT = 1, 2, 4, 8 tiles of 16 dims covering D) and
// streams tiles of 16 samples as the B operand.  Lane l = (c16 = l & 15, h = l >> 4) supplies
// X[row c16][dim h + 4k] and q[sample c16][dim h + 4k] to k-step k and receives z of rows h + 4r,
// r < 4, against sample c16.  Each lane keeps the running partials of its 4 rows x its sample
// column in registers; at the end the 16 sample columns merge with shuffles (pred_merge,
// hmc_pred.hpp) and the wave writes one record per row to the workspace.  The 4 waves of a block
// own 4 row tiles and stream the same samples at the same time (they meet in the CU's cache);
// blockIdx.x runs over the groups of 64 rows, so that blocks launched together share samples in L2.
// blockIdx.y is the sample block; k_pred_merge then merges the sample blocks' records in block
// order.  No atomics: bit-reproducible, and independent of the device (hmc_pred.hpp: geometry).
//
// One-pass moments: sums of d = x - pivot and d^2 about a per-lane pivot, the lane's first value of
// that row (0 if it is not finite).  The pivot is a draw from the very sample the moments describe,
// so |pivot - mean| is of the order of the spread and sum d^2 - (sum d)^2 / n loses
// log2(1 + (pivot - mean)^2 / var) bits, not the log2(mean^2 / var) of the unshifted form.
// ll_max / ll_sumexp: a running maximum with one exp per value: a new maximum rescales the sum
// (sum * e + 1), anything else adds e, e = exp(-|ll - max|).
#include <hip/hip_runtime.h>

#include "hmc_device.hpp"
#include "hmc_pred.hpp"

namespace hmc {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));   // the MFMA's accumulator

constexpr double kLowest = -1.79769313486231570815e308;   // running maximum before any finite ll
constexpr double kNegInf = -__builtin_huge_val();

struct PredArgs {
  const double* X;            // [n][ldx]
  const double* y;            // [n] or NULL
  const double* q;            // samples (strided view)
  double* ws;                 // [blocks][n] records
  int64_t ldx, chain_stride, row_stride, row_begin, row_step;
  int64_t rows;               // samples per chain
  int64_t n_samples;          // chains x rows
  int64_t tiles_per_block;    // 16-sample tiles per sample block
  int n, D;
};

// mu and ll of one (row, sample) entry from z: the overflow-free forms of logit_entry /
// poisson_entry (hmc_glm_ops.hpp), with mu and ll themselves instead of r = mu - y and v = -ll.
// mu comes in two parts, mu = base + part with base 0 or 1.  Bernoulli at z >= 0: mu = 1 - t / (1 + t);
// as one double a mu near 1 keeps 2^-53 of 1, as (1, -t / (1 + t)) it keeps 2^-53 of its distance
// from 1, which is what the spread of a saturated row's mu is made of (moments_add takes the
// difference from the pivot part by part).  Everywhere else base = 0 and part = mu.
template <int FAMILY, bool HASY>
__device__ __forceinline__ void pred_entry(double z, double y, double& base, double& part, double& ll) {
  static_assert(FAMILY == HMC_GLM_BERNOULLI || FAMILY == HMC_GLM_POISSON, "unknown GLM family");
  if constexpr (FAMILY == HMC_GLM_POISSON) {
    base = 0.0;
    part = fast_exp(z);                                 // +inf from z ~ 709.78 on; NaN stays NaN
    if constexpr (HASY) ll = y * z - part;
  } else {
    const double t = fast_exp(-__builtin_fabs(z));      // in [0, 1]
    const double s = 1.0 + t;
    const double inv = rcp_nr(s);
    const double c = t * inv;                           // sigma(-|z|); NaN for a NaN z
    base = z >= 0.0 ? 1.0 : 0.0;
    part = z >= 0.0 ? -c : c;
    // ll = y z - max(z, 0) - log1p(t).  Where the row is decided (|z| large, y on its side) the first
    // difference is 0 and ll is log1p(t) ~ t alone: s = 1 + t has rounded t to 2^-53, so log(s) gets
    // the rounded-off part back to first order, (t - (s - 1)) / s.
    if constexpr (HASY) ll = (y * z - (z > 0.0 ? z : 0.0)) - (fast_log(s) + (t - (s - 1.0)) * inv);
  }
}

// Running sums of one row's values x = base + part in one lane, about the pivot pbase + pivot.
struct Moments {
  double pbase, pivot, s1, s2;
};

template <bool FIRST, bool MASK>
__device__ __forceinline__ void moments_add(Moments& m, double base, double part, bool live) {
  if constexpr (FIRST) {
    const bool ok = live && pred_finite(part);
    m.pbase = ok ? base : 0.0;
    m.pivot = ok ? part : 0.0;
  }
  double d = (base - m.pbase) + (part - m.pivot);       // (base - pbase is 0 or +-1, exactly)
  if constexpr (MASK) d = live ? d : 0.0;
  m.s1 += d;
  m.s2 = __builtin_fma(d, d, m.s2);
}

// (mean, M2) of n > 0 values from the sums about the pivot.  A sum that is not finite gives the
// NumPy answers by itself: mean = pivot + (+-inf) = +-inf, M2 = inf - inf = NaN; NaN stays NaN.
__device__ __forceinline__ void moments_finish(const Moments& m, double n, double& mean, double& M2) {
  const double a = m.s1 / n;
  mean = m.pbase + (m.pivot + a);
  const double v = __builtin_fma(-m.s1, a, m.s2);
  M2 = v < 0.0 ? 0.0 : v;                               // (a comparison: NaN stays)
}

struct Lse {
  double mx, se;
};

template <bool MASK>
__device__ __forceinline__ void lse_add(Lse& l, double ll, bool live) {
  if constexpr (MASK) ll = live ? ll : kNegInf;
  const bool hi = ll > l.mx;                            // false for NaN and for -inf
  // ll = -inf: -inf - mx = -inf (mx is finite or +inf), e = 0: the term is ignored
  const double e = fast_exp(hi ? l.mx - ll : ll - l.mx);
  l.se = hi ? __builtin_fma(l.se, e, 1.0) : l.se + e;
  l.mx = hi ? ll : l.mx;
}

// One tile of 16 samples against the wave's 16 rows: the products, then the 4 entries of the lane.
template <int FAMILY, int MT, bool HASY, bool FIRST, bool MASK>
__device__ __forceinline__ void pred_tile(const double (&xa)[4 * MT], const double (&qb)[4 * MT],
                                          const double (&yv)[4], bool live, Moments (&mm)[4], Moments (&ml)[4],
                                          Lse (&ls)[4]) {
  d4 z = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int ks = 0; ks < 4 * MT; ++ks) z = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[ks], qb[ks], z, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double base, part, ll = 0.0;
    pred_entry<FAMILY, HASY>(z[r], yv[r], base, part, ll);
    moments_add<FIRST, MASK>(mm[r], base, part, live);
    if constexpr (HASY) {
      moments_add<FIRST, MASK>(ml[r], 0.0, ll, live);
      lse_add<MASK>(ls[r], ll, live);
    }
  }
}

__device__ __forceinline__ double shfl_xor_d(double v, int mask) { return __shfl_xor(v, mask, kWave); }

template <int FAMILY, int MT, bool HASY>
__global__ void __launch_bounds__(kPredWaves* kWave) k_pred(const PredArgs a) {
  constexpr int KS = 4 * MT;
  const int lane = threadIdx.x & (kWave - 1), c16 = lane & 15, h = lane >> 4;
  const int D = a.D, n = a.n;
  const int64_t tile = (int64_t)blockIdx.x * kPredWaves + (threadIdx.x / kWave);
  const int j0 = (int)(tile * 16);
  if (j0 >= n) return;                                   // wave-uniform; no barrier follows
  const int mfull = uniform_i(D >> 2), mrem = D & 3;
  const int ks_last = uniform_i((D - 1) >> 2);
  const int hl = min(h, (D - 1) & 3);
  auto dim_ok = [&](int ks) { return ks < mfull || (ks == mfull && h < mrem); };

  // ---- A operand: the row tile's X fragments, for the whole launch.  Rows past n re-read row
  // n - 1 (their records are not written), dims past D hold 0 and are read through the clamped
  // second pointer, so nothing outside [n][ldx] is touched.
  double xa[KS];
  {
    const double* xrow = a.X + (int64_t)min(j0 + c16, n - 1) * a.ldx;
    const double* xh = xrow + h;
    const double* xl = xrow + hl;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const double v = (ks >= ks_last ? xl : xh)[4 * min(ks, ks_last)];
      xa[ks] = dim_ok(ks) ? v : 0.0;
    }
  }
  double yv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) yv[r] = HASY ? a.y[min(j0 + h + 4 * r, n - 1)] : 0.0;

  // ---- the sample block: tiles [t0, t1) of 16 samples; (c0, r0) = (chain, row) of the tile's
  // first sample, advanced by 16 samples per tile without a division
  const int64_t rows = a.rows;
  const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_block;
  const int64_t tiles = (a.n_samples + 15) >> 4;
  const int64_t t1 = min(t0 + a.tiles_per_block, tiles);
  const int64_t s_first = t0 * 16;
  int64_t c0 = s_first / rows, r0 = s_first - c0 * rows;
  const int64_t q16 = 16 / rows, rem16 = 16 - q16 * rows;              // 16 samples on: chains, rows
  const int64_t lq = (int64_t)c16 / rows, lr = (int64_t)c16 - lq * rows;   // the lane's own offset
  const double* q_first = a.q + c0 * a.chain_stride + (a.row_begin + r0 * a.row_step) * a.row_stride;

  // B operand of tile t: dims h + 4 ks of sample 16 t + c16.  A lane past the last sample re-reads
  // the block's first sample and is masked; dims past D are read through the clamped pointer (a
  // real element of the same sample row) and replaced by 0.
  auto load_tile = [&](int64_t t, double (&qb)[KS]) -> bool {
    int64_t c = c0 + lq, r = r0 + lr;
    const bool wrap = r >= rows;
    r = wrap ? r - rows : r;
    c = wrap ? c + 1 : c;
    const bool live = t * 16 + c16 < a.n_samples;
    const double* qs = live ? a.q + c * a.chain_stride + (a.row_begin + r * a.row_step) * a.row_stride : q_first;
    const double* qh = qs + h;
    const double* ql = qs + hl;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const double v = (ks >= ks_last ? ql : qh)[4 * min(ks, ks_last)];
      qb[ks] = dim_ok(ks) ? v : 0.0;
    }
    // 16 samples on
    c0 += q16;
    r0 += rem16;
    const bool w0 = r0 >= rows;
    r0 = w0 ? r0 - rows : r0;
    c0 = w0 ? c0 + 1 : c0;
    return live;
  };

  Moments mm[4], ml[4];
  Lse ls[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mm[r] = Moments{0.0, 0.0, 0.0, 0.0};
    ml[r] = Moments{0.0, 0.0, 0.0, 0.0};
    ls[r] = Lse{kLowest, 0.0};
  }
  double cnt = 0.0;

  // first tile (sets the pivots; masked, as it may be the only one), full tiles, then the last
  // tile masked; the next tile's fragments are requested before the current tile's entries
  double qb[KS], qn[KS];
  bool live = load_tile(t0, qb), live_n = false;
  if (t0 + 1 < t1) live_n = load_tile(t0 + 1, qn);
  pred_tile<FAMILY, MT, HASY, true, true>(xa, qb, yv, live, mm, ml, ls);
  cnt += live ? 1.0 : 0.0;
#pragma unroll 1
  for (int64_t t = t0 + 1; t < t1; ++t) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qb[ks] = qn[ks];
    live = live_n;
    if (t + 1 < t1) live_n = load_tile(t + 1, qn);
    if (t + 1 < t1) {                                    // uniform: a full tile
      pred_tile<FAMILY, MT, HASY, false, false>(xa, qb, yv, true, mm, ml, ls);
      cnt += 1.0;
    } else {
      pred_tile<FAMILY, MT, HASY, false, true>(xa, qb, yv, live, mm, ml, ls);
      cnt += live ? 1.0 : 0.0;
    }
  }

  // ---- the lane's records, then the 16 sample columns into one (lanes c16 = 0 keep the result)
  PredRecord rec[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    PredRecord& p = rec[r];
    p.n = cnt;
    p.reserved = 0.0;
    p.mu_mean = p.mu_M2 = 0.0;
    p.ll_mean = p.ll_M2 = p.ll_max = p.ll_sumexp = pred_nan();
    if (cnt > 0.0) {
      moments_finish(mm[r], cnt, p.mu_mean, p.mu_M2);
      if constexpr (HASY) {
        moments_finish(ml[r], cnt, p.ll_mean, p.ll_M2);
        const double se = ls[r].se;
        // no term but -inf ones: max = -inf; a NaN term: both NaN (the comparisons dropped it)
        p.ll_max = se != se ? se : (se == 0.0 ? kNegInf : ls[r].mx);
        p.ll_sumexp = se;
      }
    }
  }
#pragma unroll
  for (int mask = 1; mask < 16; mask <<= 1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      PredRecord o;
      o.n = shfl_xor_d(rec[r].n, mask);
      o.mu_mean = shfl_xor_d(rec[r].mu_mean, mask);
      o.mu_M2 = shfl_xor_d(rec[r].mu_M2, mask);
      o.ll_mean = shfl_xor_d(rec[r].ll_mean, mask);
      o.ll_M2 = shfl_xor_d(rec[r].ll_M2, mask);
      o.ll_max = shfl_xor_d(rec[r].ll_max, mask);
      o.ll_sumexp = shfl_xor_d(rec[r].ll_sumexp, mask);
      o.reserved = 0.0;
      // the lower lane of a pair merges (own, other), the upper (other, own): both hold the same bits
      PredRecord lo = (c16 & mask) ? o : rec[r];
      const PredRecord hi = (c16 & mask) ? rec[r] : o;
      pred_merge(lo, hi);
      rec[r] = lo;
    }
  }
  if (c16 == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + h + 4 * r;
      if (j < n) {
        double* o = a.ws + ((int64_t)blockIdx.y * n + j) * HMC_PRED_STRIDE;
        o[0] = rec[r].n;
        o[1] = rec[r].mu_mean;
        o[2] = rec[r].mu_M2;
        o[3] = rec[r].ll_mean;
        o[4] = rec[r].ll_M2;
        o[5] = rec[r].ll_max;
        o[6] = rec[r].ll_sumexp;
        o[7] = 0.0;
      }
    }
  }
}

// out[j] = the records ws[0][j], ws[1][j], ... merged in that order; one thread per row.
__global__ void __launch_bounds__(256) k_pred_merge(const double* ws, int n, int blocks, double* out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  auto load = [&](int b) {
    const double* p = ws + ((int64_t)b * n + j) * HMC_PRED_STRIDE;
    return PredRecord{p[0], p[1], p[2], p[3], p[4], p[5], p[6], 0.0};
  };
  PredRecord acc = load(0);
  for (int b = 1; b < blocks; ++b) pred_merge(acc, load(b));
  double* o = out + (int64_t)j * HMC_PRED_STRIDE;
  o[0] = acc.n;
  o[1] = acc.mu_mean;
  o[2] = acc.mu_M2;
  o[3] = acc.ll_mean;
  o[4] = acc.ll_M2;
  o[5] = acc.ll_max;
  o[6] = acc.ll_sumexp;
  o[7] = 0.0;
}

template <int FAMILY, int MT>
void launch_pred_y(const PredArgs& a, dim3 grid, hipStream_t s) {
  if (a.y) hipLaunchKernelGGL((k_pred<FAMILY, MT, true>), grid, dim3(kPredWaves * kWave), 0, s, a);
  else hipLaunchKernelGGL((k_pred<FAMILY, MT, false>), grid, dim3(kPredWaves * kWave), 0, s, a);
}

template <int FAMILY>
void launch_pred_mt(const PredArgs& a, dim3 grid, hipStream_t s) {
  if (a.D <= 16) launch_pred_y<FAMILY, 1>(a, grid, s);
  else if (a.D <= 32) launch_pred_y<FAMILY, 2>(a, grid, s);
  else if (a.D <= 64) launch_pred_y<FAMILY, 4>(a, grid, s);
  else launch_pred_y<FAMILY, 8>(a, grid, s);
}

}  // namespace

hipError_t launch_pred(const hmc_glm& eval, const hmc_samples& sm, int64_t rows, int64_t n_samples, double* out,
                       double* ws, hipStream_t s) {
  PredArgs a{};
  a.X = eval.X;
  a.y = eval.y;
  a.q = sm.q;
  a.ws = ws;
  a.ldx = eval.ldx;
  a.chain_stride = sm.chain_stride;
  a.row_stride = sm.row_stride;
  a.row_begin = sm.row_begin;
  a.row_step = sm.row_step;
  a.rows = rows;
  a.n_samples = n_samples;
  a.tiles_per_block = pred_tiles_per_block(eval.n, n_samples);
  a.n = eval.n;
  a.D = eval.D;
  const int64_t blocks = pred_sample_blocks(eval.D, eval.n, n_samples);
  const dim3 grid((unsigned)pred_row_groups(eval.n), (unsigned)blocks);
  if (eval.family == HMC_GLM_POISSON) launch_pred_mt<HMC_GLM_POISSON>(a, grid, s);
  else launch_pred_mt<HMC_GLM_BERNOULLI>(a, grid, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pred_merge, dim3((unsigned)((eval.n + 255) / 256)), dim3(256), 0, s, ws, eval.n, (int)blocks,
                     out);
  return hipGetLastError();
}

}  // namespace hmc
