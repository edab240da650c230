// hmc_logit.hip — fused Random-trajectory HMC iterations for a Bayesian logistic-regression
// posterior: the first target defined by data (a design matrix X [n][D] and labels y [n]).
//
// Replaces HMC_sampler.gen_sample_random (samplers.py:387-491) and leap_frog / E (:811-839) for
//     V(q)  = sum_j [ softplus(z_j) - y_j z_j ] + 0.5 sum_d prec_d q_d^2,      z = X q
//     dV/dq = X^T (sigma(z) - y) + prec q
// with softplus(z) = max(z, 0) + log(1 + exp(-|z|)) and sigma(z) = 1/(1+t) (z >= 0), t/(1+t)
// (z < 0), t = exp(-|z|): the forms that never overflow.
//
// One wave integrates a tile of 16 chains, as the dense-precision kernel (hmc_dense.hip): lane
// l = (chain c = l & 15, h = l >> 4) owns dims d = h + 4m (m < 4 MT) of chain c; q, p and the
// gradient stay in registers across the fused iterations.  One gradient walks X in tiles of 16
// rows, two products on v_mfma_f64_16x16x4_f64 per tile (A: lane l holds A[l&15][l>>4]; B: lane l
// holds B[l>>4][l&15]; C/D register r of lane l holds C[(l>>4) + 4r][l&15]):
//     Z^T[16 rows x 16 chains]     = X_tile . Q^T       k-step ks: A = X[j0 + c][4ks + h], B = q[ks]
//     G^T[16 dims x 16 chains]    += X_tile^T . R       k-step r:  A = X[j0 + 4r + h][16nt + c], B = R[r]
// The accumulator of Z^T holds, in lane (c, h) register r, row j0 + h + 4r of chain c; after the
// elementwise R = sigma(Z) - y that register is the B operand of k-step r (rows 4r .. 4r+3) of the
// second product, whose accumulator nt register r holds dim 16nt + h + 4r = h + 4(4nt + r): the
// layout q and p live in.  Nothing moves between lanes except the per-chain sums of V and K
// (chain_sum4), and an MFMA output column reads only its own B column, so a chain's arithmetic
// does not depend on its tile column, on its neighbours, on the launch split or on chain_offset.
// X is read from global memory in both lane layouts (every wave reads the same rows: they stay
// in L2 / the CU's cache).  Indices are clamped, never masked: a row j >= n gets R = 0 and adds
// nothing to V, a column d >= D meets q_d = 0 in the first product and gives a gradient entry
// that is dropped where it is consumed (padding dims keep p = q = 0).  The per-dimension
// constants (prior precision, dt, dt minv / 2, minv, p_scale) sit zero padded in LDS.
//
// V falls out of the gradient pass: the per-(row, chain) terms are summed per lane and reduced
// over a chain's four lanes only where an energy is needed (E0 with the gradient of the first
// half kick, E1 with the last step's gradient).  Leapfrog with the reference's Q3 semantics
// (samplers.py:831-839): p_half = p - dt_d (minv_d g_d) / 2;  q += dt_d p_half;  g = grad(q);
// p = p_half - dt_d (minv_d g_d) / 2.  accept iff (dE < 0) || (log u < -dE): a NaN or infinite
// energy rejects.  A tile steps to its longest trajectory; chains that have done their L steps
// stand still under the EXEC mask (no arithmetic on them, so a non-finite chain stays put).
//
// One arithmetic for both fp_mode values (fast_exp / fast_log of hmc_device.hpp are ~1 ulp fp64,
// not bit-identical to NumPy's).  Built with -ffp-contract=off; the FMAs are explicit.
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
template <int MT>
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
      logit_entry(z[r], x.y[min(j, n - 1)], R[r], v);
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

// First half of samplers.py:831-839: p_half (left in p) and q_new.  Padding dims stay 0.
template <int MT>
__device__ __forceinline__ void kick_drift(const TileLane& t, const DimTable& sd, const d4 (&g)[MT],
                                           double (&p)[4 * MT], double (&q)[4 * MT]) {
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) {
    const double gm = dim_ok(t, m) ? gval<MT>(g, m) : 0.0;
    p[m] = __builtin_fma(-sd[kHalfKick][ho + 4 * m], gm, p[m]);
    q[m] = __builtin_fma(sd[kDt][ho + 4 * m], p[m], q[m]);
    if ((m & 7) == 7) __builtin_amdgcn_sched_barrier(0);     // bound the table reads in flight
  }
}

// Second half: p_new = p_half - dt (minv g(q_new)) / 2.
template <int MT>
__device__ __forceinline__ void kick(const TileLane& t, const DimTable& sd, const d4 (&g)[MT], double (&p)[4 * MT]) {
  const int ho = table_lane(t.h);
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) {
    const double gm = dim_ok(t, m) ? gval<MT>(g, m) : 0.0;
    p[m] = __builtin_fma(-sd[kHalfKick][ho + 4 * m], gm, p[m]);
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

// ------------------------------------------------------------------------------------------
// Chain initialisation (samplers.py:413-420): q_chain[:,0] = q_start, E_chain[:,0] = E(q, p0).
template <int MT, bool REPLAY>
__global__ __launch_bounds__(64 * kLogitWaves) void k_logit_init(LogitArgs x) {
  constexpr int M = 4 * MT;
  const RandArgs& a = x.a;
  __shared__ DimTable sd;
  stage_dims(x, sd);
  const TileLane t = tile_lane(a.n, a.D);
  if (t.tile >= a.ntiles) return;            // wave-uniform; no block barrier follows
  const uint64_t gc = (uint64_t)(a.chain_offset + t.c);
  double q[M], p[M];
  d4 g[MT];
  load_dims<MT>(a.qstart + t.c * (int64_t)a.D, t, q);
  draw_momentum<MT, REPLAY, false>(a, t, sd, 0, gc, nullptr, p);
  const double vp = logit_grad<MT>(x, t, sd, q, g);
  const double E0 = chain_sum4(vp + kinetic_part<MT>(t, sd, p));
  store_dims<MT>(a.q + t.c * (int64_t)a.D, t, q);
  if (a.qc && a.q_row0 == 0) store_dims<MT>(a.qc + t.c * (int64_t)a.Lq * a.D, t, q);
  if (t.live && t.h == 0) {
    a.Eprev[t.c] = E0;
    if (a.Ec) a.Ec[t.c * (int64_t)a.Lc] = E0;
    if (a.dEc) a.dEc[t.c * (int64_t)a.Lc] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// Iterations [it0, it1) (samplers.py:428-475).
template <int MT, bool REPLAY>
__global__ __launch_bounds__(64 * kLogitWaves) __attribute__((amdgpu_waves_per_eu(kItersWaves<MT>, kItersWaves<MT>)))
void k_logit_iters(LogitArgs x) {
  constexpr int M = 4 * MT;
  const RandArgs& a = x.a;
  __shared__ DimTable sd;
  __shared__ double s_ntab[REPLAY ? 2 : kNormalTableDoubles];   // Box-Muller tables (Philox momentum)
  if constexpr (!REPLAY) init_normal_tables(s_ntab);             // synchronised by stage_dims
  stage_dims(x, sd);
  const TileLane t = tile_lane(a.n, a.D);
  if (t.tile >= a.ntiles) return;            // wave-uniform; no block barrier follows
  const uint64_t gc = (uint64_t)(a.chain_offset + t.c);
  // a.q keeps the chain's state at the start of the current iteration (written back on every
  // acceptance), so a rejection reloads it instead of holding a copy in registers
  double q[M], p[M];
  d4 g[MT];
  double* const qrow = a.q + t.c * (int64_t)a.D;
  load_dims<MT>(qrow, t, q);
  double Eprev = t.live ? a.Eprev[t.c] : 0.0;
  double* const qcb = a.qc ? a.qc + t.c * (int64_t)a.Lq * a.D : nullptr;
  unsigned long long n_acc = 0, n_acc_wu = 0, n_lf = 0, n_lf2 = 0, n_oob = 0;
  // chain-0 trajectory capture (samplers.py:442-452): the wave holding global chain 0 (lane 0)
  const bool cap_wave = a.traj_q && uniform_i((int)(__builtin_amdgcn_readfirstlane((int)(gc & 0xffffffff)) == 0 &&
                                                    __builtin_amdgcn_readfirstlane((int)(gc >> 32)) == 0));

  for (int it = a.it0; it < a.it1; ++it) {
    draw_momentum<MT, REPLAY, true>(a, t, sd, it, gc, s_ntab, p);          // samplers.py:431
    const bool post = it >= a.wu;
    const bool write_row = post && ((it == a.niter) || ((it - a.wu + 1) % a.thin == 0));
    const int64_t row = post ? (int64_t)((it - a.wu) / a.thin) : 0;
    // ---- trajectory length (:441) and log-uniform for the MH test (:461), per chain
    int L;
    double lnu;
    if constexpr (REPLAY) {
      L = t.live ? a.rL[t.c * (int64_t)a.niter + (it - 1)] : 0;
      lnu = t.live ? a.rlnu[t.c * (int64_t)a.niter + (it - 1)] : 0.0;
    } else {
      const uint4 r = draw_block(kDrawSlot, (uint32_t)it, gc, a.k0, a.k1);
      L = t.live ? uniform_int(r.x, a.L_low, a.L_high) : 0;
      const double u = u53(r.z, r.w);
      lnu = u > 0.0 ? fast_log(u) : -__builtin_inf();      // log(random()), :461
    }
    const int Lmax = wave_max_i32(L);
    const bool cap = cap_wave && it <= a.n_save;
    double* capp = cap ? a.traj_q + (int64_t)(it - 1) * a.traj_stride * 2 : nullptr;
    if (cap) {   // dims 0 and 1 of chain 0 live in lanes 0 (h = 0) and 16 (h = 1)
      const double q1 = __shfl(q[0], 16, kWave);
      if (t.lane == 0) {
        capp[0] = q[0];
        capp[1] = a.D > 1 ? q1 : q[0];
      }
    }
    // ---- one gradient pass at the start point (l = -1: with it the initial energy, :434, and the
    // gradient the first half kick needs), then L leapfrog steps (:448-450 -> :831-839).  The tile
    // steps as long as its longest trajectory; the MFMAs run with all lanes, a chain that has done
    // its L steps stands still (the gradient of an unchanged q is the one it already holds).
    double vp = 0.0, E0 = 0.0;
    for (int l = -1; l < Lmax; ++l) {
      const bool act = l >= 0 && l < L;
      if (act) kick_drift<MT>(t, sd, g, p, q);
      const double vn = logit_grad<MT>(x, t, sd, q, g);
      if (l < 0) {                                           // uniform
        vp = vn;
        E0 = chain_sum4(vp + kinetic_part<MT>(t, sd, p));
        if (t.live && t.h == 0 && write_row) {               // :436-438 (Q14)
          if (a.Ec) a.Ec[t.c * (int64_t)a.Lc + row] = E0;
          if (a.dEc) a.dEc[t.c * (int64_t)a.Lc + row] = E0 - Eprev;
        }
        Eprev = E0;                                          // :460
        continue;
      }
      if (act) {
        kick<MT>(t, sd, g, p);
        vp = vn;
      }
      if (cap) {
        const double q1 = __shfl(q[0], 16, kWave);
        if (t.lane == 0 && act) {
          capp[2 * (l + 1)] = q[0];
          capp[2 * (l + 1) + 1] = a.D > 1 ? q1 : q[0];
        }
      }
    }
    // ---- final energy with the last step's gradient pass, Metropolis test (:455-472)
    const double E1 = chain_sum4(vp + kinetic_part<MT>(t, sd, p));
    const double dE = E1 - E0;
    const bool accept = (dE < 0.0) || (lnu < -dE);
    if (accept) store_dims<MT>(qrow, t, q);
    else load_dims<MT>(qrow, t, q);
    if (write_row && qcb && row >= a.q_row0) {
      double* rowp = qcb + (row % a.Lq) * a.D;
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (t.live && dim_ok(t, m)) __builtin_nontemporal_store(q[m], rowp + t.h + 4 * m);   // written once
    }
    if (cap && t.lane == 0) {
      a.traj_len[it - 1] = (L > 0 ? L : 0) + 1;
      a.decision[it - 1] = accept ? 1 : 0;
    }
    if (t.live && t.h == 0) {
      if (accept) {
        if (post) ++n_acc; else ++n_acc_wu;
      } else if (it < a.i_oob) {
        ++n_oob;                                           // reference would raise IndexError (Q5)
      }
      const unsigned long long Lp = L > 0 ? (unsigned long long)L : 0ull;   // xrange(1, L+1) is empty for L <= 0
      n_lf += Lp;
      n_lf2 += Lp * Lp;
    }
  }

  // ---- state write-back and counters (a.q already holds q)
  if (t.live && t.h == 0) a.Eprev[t.c] = Eprev;
  n_acc = wave_sum_u64(n_acc);
  n_acc_wu = wave_sum_u64(n_acc_wu);
  n_lf = wave_sum_u64(n_lf);
  n_lf2 = wave_sum_u64(n_lf2);
  n_oob = wave_sum_u64(n_oob);
  if (t.lane == 0 && a.cnt) {   // per-wave counts into one of HMC_COUNTER_SLOTS rows
    unsigned long long* cs = a.cnt + (t.tile & (HMC_COUNTER_SLOTS - 1)) * HMC_NCOUNTERS;
    if (n_acc) atomicAdd(cs + HMC_CNT_ACCEPT, n_acc);
    if (n_acc_wu) atomicAdd(cs + HMC_CNT_ACCEPT_WU, n_acc_wu);
    if (n_lf) atomicAdd(cs + HMC_CNT_LEAPFROG, n_lf);
    if (n_lf2) atomicAdd(cs + HMC_CNT_LEAPFROG_SQ, n_lf2);
    if (n_oob) atomicAdd(cs + HMC_CNT_OOB_REJECT, n_oob);
  }
}

// ------------------------------------------------------------------------------------------
// Row-wise forms on tiles of 16 rows: HMC_sampler.leap_frog (samplers.py:831-839) and E (:819-823).
template <int MT, bool LEAP>
__global__ __launch_bounds__(64 * kLogitWaves) void k_logit_rows(LogitArgs x) {
  constexpr int M = 4 * MT;
  const RandArgs& a = x.a;
  __shared__ DimTable sd;
  stage_dims(x, sd);
  const TileLane t = tile_lane(a.n, a.D);
  if (t.tile >= a.ntiles) return;            // wave-uniform; no block barrier follows
  double q[M], p[M];
  d4 g[MT];
  load_dims<MT>(x.row_q + t.c * (int64_t)a.D, t, q);
  load_dims<MT>(x.row_p + t.c * (int64_t)a.D, t, p);
  double vp = 0.0;
#pragma unroll 1
  for (int pass = 0; pass < (LEAP ? 2 : 1); ++pass) {   // one call site of the gradient
    if (pass) kick_drift<MT>(t, sd, g, p, q);
    vp = logit_grad<MT>(x, t, sd, q, g);
  }
  if constexpr (LEAP) {
    kick<MT>(t, sd, g, p);
    store_dims<MT>(x.row_po + t.c * (int64_t)a.D, t, p);
    store_dims<MT>(x.row_qo + t.c * (int64_t)a.D, t, q);
  } else {
    const double E = chain_sum4(vp + kinetic_part<MT>(t, sd, p));
    if (t.live && t.h == 0) x.row_E[t.c] = E;
  }
}

template <int MT>
hipError_t launch_mt(const LogitArgs& x, int what, bool flag, hipStream_t s) {
  const dim3 grid((unsigned)((x.a.ntiles + kLogitWaves - 1) / kLogitWaves)), block(64 * kLogitWaves);
  switch (what) {
    case 0:
      if (flag) k_logit_init<MT, true><<<grid, block, 0, s>>>(x);
      else k_logit_init<MT, false><<<grid, block, 0, s>>>(x);
      break;
    case 1:
      if (flag) k_logit_iters<MT, true><<<grid, block, 0, s>>>(x);
      else k_logit_iters<MT, false><<<grid, block, 0, s>>>(x);
      break;
    default:
      if (flag) k_logit_rows<MT, true><<<grid, block, 0, s>>>(x);
      else k_logit_rows<MT, false><<<grid, block, 0, s>>>(x);
      break;
  }
  return hipGetLastError();
}

// 16-dim output tiles per chain: 1, 2, 4 or 8 (D <= HMC_LOGIT_MAX_D = 128).  An instance runs all
// its k-steps and output tiles whatever D is (see logit_grad).
hipError_t launch(LogitArgs x, int what, bool flag, hipStream_t s) {
  if (x.a.n == 0) return hipSuccess;
  x.a.ntiles = (x.a.n + 15) / 16;
  const int mt = (x.a.D + 15) / 16;
  if (mt <= 1) return launch_mt<1>(x, what, flag, s);
  if (mt <= 2) return launch_mt<2>(x, what, flag, s);
  if (mt <= 4) return launch_mt<4>(x, what, flag, s);
  if (mt <= 8) return launch_mt<8>(x, what, flag, s);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_logit_init(const LogitArgs& x, bool replay, hipStream_t s) { return launch(x, 0, replay, s); }
hipError_t launch_logit_iters(const LogitArgs& x, bool replay, hipStream_t s) { return launch(x, 1, replay, s); }
hipError_t launch_logit_rows(const LogitArgs& x, bool leapfrog, hipStream_t s) { return launch(x, 2, leapfrog, s); }

}  // namespace hmc
