// hmc_glm_ops.hpp — the 16-chain tile of the generalized-linear-model targets, shared by the
// Random-trajectory kernels (hmc_logit.hip) and the NUTS kernel (hmc_glm_nuts.hip): the lane layout,
// the per-dimension tables in LDS, the f64-MFMA gradient with its family-specific entry, the two
// half kicks, the kinetic energy, the row loads / stores and the momentum draw.
// Lane l = (chain c = l & 15, h = l >> 4) owns dims d = h + 4m, m < 4*MT, of chain c.
#pragma once
#include "hmc_adapt.hpp"
#include "hmc_device.hpp"
#include "hmc_dense_ops.hpp"
#include "hmc_logit.hpp"

namespace hmc {

namespace {

constexpr int kLogitWaves = 4;   // waves (16-chain tiles) per block
constexpr int kLogitPad = HMC_LOGIT_MAX_D;
// Waves per SIMD the iteration kernel is compiled for: two (256 registers) up to 32 dims, so that
// one wave's exp / log / reciprocal VALU work overlaps the other's MFMAs and loads; above, one wave
// with the whole 512-register file (capped at 256 registers the 64-dim instance spills).
template <int MT>
constexpr int kItersWaves = MT <= 2 ? 2 : 1;
// The gradient holds a whole row tile's X fragments (8 MT doubles) in registers up to 64 dims; at
// 128 dims q, p and g leave no room for them.
constexpr int kPreloadMaxMT = 4;

// Per-dimension constants of the launch, staged once per block and zero padded to kLogitPad, so
// that lane (c, h) reads dim h + 4m at a fixed offset from one LDS address and a padding dim needs
// no test: it has a zero prior precision, step and kick.
enum : int { kPrec = 0, kDt = 1, kHalfKick = 2, kMinv = 3, kPscale = 4, kDimRows = 5 };
typedef double DimTable[kDimRows][kLogitPad];

// Every thread of the block calls this (it ends with the block barrier).
__device__ __forceinline__ void stage_dims(const LogitArgs& x, DimTable& sd) {
  const RandArgs& a = x.a;
  for (int d = threadIdx.x; d < kLogitPad; d += blockDim.x) {
    const bool ok = d < a.D;
    const double dt = !ok ? 0.0 : (a.dtv ? a.dtv[d] : a.dt);
    const double mi = !ok ? 0.0 : (a.minv ? a.minv[d] : 1.0);
    sd[kPrec][d] = ok ? x.pprec[d] : 0.0;
    sd[kDt][d] = dt;
    sd[kHalfKick][d] = (0.5 * dt) * mi;      // dt_d minv_d / 2
    sd[kMinv][d] = mi;
    sd[kPscale][d] = !ok ? 0.0 : (a.pscale ? a.pscale[d] : 1.0);
  }
  __syncthreads();
}

// The lane's row offset h for reads of a DimTable, made opaque where a pass over the dims starts:
// the tables never change during a launch, and reads the optimiser can prove loop-invariant are
// hoisted out of the iteration loop into up to 5 x 32 register pairs.
__device__ __forceinline__ int table_lane(int h) { return (int)opaque_u32((uint32_t)h); }

struct TileLane {
  int lane, c16, h;
  int mfull, mrem;   // dim h + 4m < D  <=>  m < mfull, or m == mfull and h < mrem
  int64_t tile, c;   // the wave's tile; the lane's chain (or row), clamped to 0 when not live
  bool live;
};

__device__ __forceinline__ TileLane tile_lane(int64_t n, int D) {
  TileLane t;
  t.lane = threadIdx.x & (kWave - 1);
  t.c16 = t.lane & 15;
  t.h = t.lane >> 4;
  t.mfull = uniform_i(D >> 2);
  t.mrem = D & 3;
  t.tile = (int64_t)blockIdx.x * kLogitWaves + (threadIdx.x / kWave);
  const int64_t slot = t.tile * 16 + t.c16;
  t.live = slot < n;
  t.c = t.live ? slot : 0;
  return t;
}

__device__ __forceinline__ bool dim_ok(const TileLane& t, int m) {
  return m < t.mfull || (m == t.mfull && t.h < t.mrem);
}

// One (row, chain) entry: r = sigma(z) - y and v = softplus(z) - y z.  t = exp(-|z|) is in [0, 1]
// (0 once |z| > 746), so 1 + t is in [1, 2] and nothing overflows; a NaN z gives NaN r and v.
__device__ __forceinline__ void logit_entry(double z, double y, double& r, double& v) {
  const double t = fast_exp(-__builtin_fabs(z));
  const double s = 1.0 + t;
  const double inv = rcp_nr(s);
  r = (z >= 0.0 ? inv : t * inv) - y;
  v = ((z > 0.0 ? z : 0.0) + fast_log(s)) - y * z;
}

// Poisson regression with a log link: r = exp(z) - y and v = exp(z) - y z (log y! is constant in
// q).  fast_exp saturates by itself: +inf from z ~ 709.78 on (its argument clamp at 710 overflows
// in the final ldexp), 0 below -746, so an overflowing chain gets V = +inf and a NaN z stays NaN.
__device__ __forceinline__ void poisson_entry(double z, double y, double& r, double& v) {
  const double e = fast_exp(z);
  r = e - y;
  v = e - y * z;
}

// The family-specific part of the gradient: one (row, chain) entry of R and of V.
template <int FAMILY>
__device__ __forceinline__ void glm_entry(double z, double y, double& r, double& v) {
  static_assert(FAMILY == HMC_GLM_BERNOULLI || FAMILY == HMC_GLM_POISSON, "unknown GLM family");
  if constexpr (FAMILY == HMC_GLM_POISSON) poisson_entry(z, y, r, v);
  else logit_entry(z, y, r, v);
}

// g = dV/dq(q) in the lane's dims (padding dims hold values that the callers drop) and the lane's
// share of V(q): chain_sum4 of the return value is V.  Called by every lane of the wave together.
// No branch sits between the MFMAs: a uniform branch around one ends a basic block, and the
// accumulators then travel between the two register files at every block edge while each MFMA is
// waited out (measured: the guarded form was 2-3x slower).  So all 4 MT k-steps and all MT output
// tiles always run.  A k-step (output tile) past the last real one re-reads the last real one's
// columns: against q = 0 it adds exact zeros to Z, and the gradient entries it produces belong to
// padding dims, which the callers drop.  Only the last real k-step (output tile) can reach past
// column D - 1; there the lane offset is clamped (a second pointer), so a padding lane re-reads a
// real column of the same row and nothing outside [n][ldx] is touched.
template <int FAMILY, int MT>
__device__ __forceinline__ double logit_grad(const LogitArgs& x, const TileLane& t, const DimTable& sd,
                                             const double (&q)[4 * MT], d4 (&g)[MT]) {
  constexpr int KS = 4 * MT;
  constexpr bool PRE = MT <= kPreloadMaxMT;   // a tile's 8 MT fragments in registers at once
  const int D = x.a.D, n = x.nrows;
  const int ks_last = uniform_i((D - 1) >> 2), nt_last = uniform_i((D - 1) >> 4);
  const int hl = min(t.h, (D - 1) & 3), cl = min(t.c16, (D - 1) & 15);
  // prior: g = prec q, V = sum prec q^2 / 2 (padding dims: prec = 0, q = 0)
  double vp = 0.0;
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < KS; ++m) {
    const double pq = sd[kPrec][ho + 4 * m] * q[m];
    g[m >> 2][m & 3] = pq;
    vp = __builtin_fma(pq, q[m], vp);
  }
  vp *= 0.5;
#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += 16) {
    const double* xrow = x.X + (int64_t)min(j0 + t.c16, n - 1) * x.ldx;
    const double* xzh = xrow + t.h;
    const double* xzl = xrow + hl;
    // fragment of k-step ks of the first product, of (k-step r, output tile nt) of the second
    auto frag_z = [&](int ks) { return (ks >= ks_last ? xzl : xzh)[4 * min(ks, ks_last)]; };
    auto frag_g = [&](int r, int nt) {
      const double* grow = x.X + (int64_t)min(j0 + 4 * r + t.h, n - 1) * x.ldx;
      return (nt >= nt_last ? grow + cl : grow + t.c16)[16 * min(nt, nt_last)];
    };
    // PRE: every fragment of the tile is requested before the first MFMA, so one wave per SIMD
    // waits out the cache latency once per tile; otherwise the loads sit next to their MFMAs
    double xa[PRE ? KS : 1], xb[PRE ? 4 * MT : 1];
    if constexpr (PRE) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xa[ks] = frag_z(ks);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int nt = 0; nt < MT; ++nt) xb[r * MT + nt] = frag_g(r, nt);
      }
    }
    // ---- Z^T = X_tile . Q^T
    d4 z = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const double a = PRE ? xa[PRE ? ks : 0] : frag_z(ks);
      z = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[ks], z, 0, 0, 0);
    }
    // ---- R = sigma(Z) - y and the tile's share of V; rows j >= n contribute nothing
    double R[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + t.h + 4 * r;
      double v;
      glm_entry<FAMILY>(z[r], x.y[min(j, n - 1)], R[r], v);
      R[r] = j < n ? R[r] : 0.0;
      vp += j < n ? v : 0.0;
    }
    // ---- G^T += X_tile^T . R
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int nt = 0; nt < MT; ++nt) {
        const double a = PRE ? xb[PRE ? r * MT + nt : 0] : frag_g(r, nt);
        g[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, R[r], g[nt], 0, 0, 0);
      }
    }
  }
  return vp;
}

// A table entry that scales with the step (kDt, kHalfKick) under the lane's step multiplier s
// (hmc_adapt.hpp): one multiply per table read in the ADAPT form, the entry itself otherwise.
template <bool ADAPT>
__device__ __forceinline__ double step_entry(double entry, double s) {
  if constexpr (ADAPT) return s * entry;
  else return entry;
}

// First half of samplers.py:831-839: p_half (left in p) and q_new.  Padding dims stay 0.
// ADAPT: the step is s dt_d, with s the multiplier of the lane's chain.
template <int MT, bool ADAPT = false>
__device__ __forceinline__ void kick_drift(const TileLane& t, const DimTable& sd, const d4 (&g)[MT],
                                           double (&p)[4 * MT], double (&q)[4 * MT], double s = 1.0) {
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) {
    const double gm = dim_ok(t, m) ? gval<MT>(g, m) : 0.0;
    p[m] = __builtin_fma(-step_entry<ADAPT>(sd[kHalfKick][ho + 4 * m], s), gm, p[m]);
    q[m] = __builtin_fma(step_entry<ADAPT>(sd[kDt][ho + 4 * m], s), p[m], q[m]);
    if ((m & 7) == 7) __builtin_amdgcn_sched_barrier(0);     // bound the table reads in flight
  }
}

// Second half: p_new = p_half - dt (minv g(q_new)) / 2.
template <int MT, bool ADAPT = false>
__device__ __forceinline__ void kick(const TileLane& t, const DimTable& sd, const d4 (&g)[MT], double (&p)[4 * MT],
                                     double s = 1.0) {
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) {
    const double gm = dim_ok(t, m) ? gval<MT>(g, m) : 0.0;
    p[m] = __builtin_fma(-step_entry<ADAPT>(sd[kHalfKick][ho + 4 * m], s), gm, p[m]);
  }
}

// The lane's share of K(p) = sum p_d minv_d p_d / 2 (samplers.py:817 with a diagonal inv(cov_p)).
template <int MT>
__device__ __forceinline__ double kinetic_part(const TileLane& t, const DimTable& sd, const double (&p)[4 * MT]) {
  double kin = 0.0;
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) kin = __builtin_fma(p[m], sd[kMinv][ho + 4 * m] * p[m], kin);
  return 0.5 * kin;
}

template <int MT>
__device__ __forceinline__ void load_dims(const double* row, const TileLane& t, double (&v)[4 * MT]) {
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) v[m] = (t.live && dim_ok(t, m)) ? row[t.h + 4 * m] : 0.0;
}

template <int MT>
__device__ __forceinline__ void store_dims(double* row, const TileLane& t, const double (&v)[4 * MT]) {
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m)
    if (t.live && dim_ok(t, m)) row[t.h + 4 * m] = v[m];
}

// Momentum of (chain, iteration it): the dense Random kernel's streams.  Replay: the tape's row.
// Philox: dims h + 4m, pairs (m, m+1) for even m from block (h + 4m, it, chain); iteration 0 (TAB
// false) is the plain Box-Muller, later iterations the table transform; scaled by p_scale.
template <int MT, bool REPLAY, bool TAB>
__device__ __forceinline__ void draw_momentum(const RandArgs& a, const TileLane& t, const DimTable& sd, int it,
                                              uint64_t gc, const double* s_ntab, double (&p)[4 * MT]) {
  if constexpr (REPLAY) {
    const double* row = (it == 0) ? a.rp0 + t.c * (int64_t)a.D : a.rp + (t.c * (int64_t)a.niter + (it - 1)) * a.D;
    load_dims<MT>(row, t, p);
  } else {
    const int ho = table_lane(t.h);
#pragma unroll
    for (int m = 0; m < 4 * MT; m += 2) {
      double z0 = 0.0, z1 = 0.0;
      if (m < t.mfull || (m == t.mfull && t.mrem > 0)) {   // uniform: pairs wholly in the padding are not drawn
        const uint4 r = draw_block(opaque_u32((uint32_t)(t.h + 4 * m)), (uint32_t)it, gc, a.k0, a.k1);
        if constexpr (TAB) normal_pair_tab(r, s_ntab, z0, z1);
        else normal_pair(r, z0, z1);
        z0 *= sd[kPscale][ho + 4 * m];
        z1 *= sd[kPscale][ho + 4 * m + 4];
      }
      p[m] = (t.live && dim_ok(t, m)) ? z0 : 0.0;
      p[m + 1] = (t.live && dim_ok(t, m + 1)) ? z1 : 0.0;
      if ((m & 6) == 6) __builtin_amdgcn_sched_barrier(0);   // bound the RNG chains in flight (registers)
    }
  }
}

}  // namespace

}  // namespace hmc
