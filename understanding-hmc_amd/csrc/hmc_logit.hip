// hmc_logit.hip — fused Random-trajectory HMC iterations for a Bayesian logistic-regression
// posterior: the first target defined by data (a design matrix X [n][D] and labels y [n]).
// The kernels take the GLM family as a template parameter (hmc_glm_ops.hpp: glm_entry): what follows
// describes HMC_GLM_BERNOULLI, the instances the hmc_logit_* entries launch; HMC_GLM_POISSON differs
// in the per-(row, chain) entry alone, r = exp(z) - y and v = exp(z) - y z.  The tile, its gradient
// and the leapfrog pieces live in hmc_glm_ops.hpp, shared with the NUTS kernel (hmc_glm_nuts.hip).
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
#include "hmc_dispatch.hpp"
#include "hmc_glm_ops.hpp"
#include "hmc_random_iter.hpp"

namespace hmc {

namespace {

// ------------------------------------------------------------------------------------------
// Chain initialisation (samplers.py:413-420): q_chain[:,0] = q_start, E_chain[:,0] = E(q, p0).
template <int FAMILY, int MT, bool REPLAY>
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
  const double vp = logit_grad<FAMILY, MT>(x, t, sd, q, g);
  const double E0 = chain_sum4(vp + kinetic_part<MT>(t, sd, p));
  store_dims<MT>(a.q + t.c * (int64_t)a.D, t, q);
  if (a.qc && a.q_row0 == 0) store_dims<MT>(a.qc + t.c * (int64_t)a.Lq * a.D, t, q);
  if (t.live && t.h == 0) store_init_energy(a, t.c, E0);
}

// ------------------------------------------------------------------------------------------
// Iterations [it0, it1) (samplers.py:428-475).  ADAPT: every chain runs at its own multiple s of
// the step and adapts it during warm-up from min(1, exp(-dE)) of its Metropolis test
// (hmc_adapt.hpp); the lane holds its chain's state for the launch.  With ADAPT = false none of it
// is compiled and the kernel takes the plain argument block: those instances are the code they were
// before the ADAPT form.
template <bool ADAPT>
using ItersKernelArgs = std::conditional_t<ADAPT, LogitAdaptArgs, LogitArgs>;

template <int FAMILY, int MT, bool REPLAY, bool ADAPT>
__global__ __launch_bounds__(64 * kLogitWaves) __attribute__((amdgpu_waves_per_eu(kItersWaves<MT>, kItersWaves<MT>)))
void k_logit_iters(ItersKernelArgs<ADAPT> x) {
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
  RandomTally tally;
  // chain-0 trajectory capture (samplers.py:442-452): the wave holding global chain 0 (lane 0)
  const bool cap_wave = a.traj_q && uniform_i((int)(__builtin_amdgcn_readfirstlane((int)(gc & 0xffffffff)) == 0 &&
                                                    __builtin_amdgcn_readfirstlane((int)(gc >> 32)) == 0));
  hmc_adapt ax{};
  AdaptParams adp{};
  AdaptState ad{};
  double s = 1.0;   // ADAPT: the chain's step multiplier of the current iteration
  if constexpr (ADAPT) {
    ax = x.ad;
    adp = AdaptParams{ax.delta, ax.gamma, ax.t0, ax.kappa};
    ad = t.live ? adapt_load(ax.state + t.c * HMC_ADAPT_STRIDE) : adapt_initial(1.0);
    s = adapt_scale(ad, a.it0 < ax.adapt_end);
  }

  for (int it = a.it0; it < a.it1; ++it) {
    draw_momentum<MT, REPLAY, true>(a, t, sd, it, gc, s_ntab, p);          // samplers.py:431
    const bool post = it >= a.wu;
    const bool write_row = stores_row(a, it);
    const int64_t row = row_of(a, it);
    // ---- trajectory length (:441) and log-uniform for the MH test (:461), per chain
    int L;
    double lnu;
    if constexpr (REPLAY) {
      L = t.live ? a.rL[t.c * (int64_t)a.niter + (it - 1)] : 0;
      lnu = t.live ? a.rlnu[t.c * (int64_t)a.niter + (it - 1)] : 0.0;
    } else {
      const TrajDraw d = draw_traj(a, it, gc);
      L = t.live ? d.L : 0;
      lnu = d.lnu;
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
      if (act) kick_drift<MT, ADAPT>(t, sd, g, p, q, s);
      const double vn = logit_grad<FAMILY, MT>(x, t, sd, q, g);
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
        kick<MT, ADAPT>(t, sd, g, p, s);
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
    if constexpr (ADAPT) {
      adapt_iteration(ad, adp, it < ax.adapt_end, adapt_alpha(dE, E1));
      s = adapt_scale(ad, it + 1 < ax.adapt_end);
    }
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
    if (t.live && t.h == 0) tally.count(a, it, post, accept, L);
  }

  // ---- state write-back and counters (a.q already holds q)
  if (t.live && t.h == 0) {
    a.Eprev[t.c] = Eprev;
    if constexpr (ADAPT) adapt_store(ax.state + t.c * HMC_ADAPT_STRIDE, ad);
  }
  tally.flush(a, t.lane, t.tile);
}

// ------------------------------------------------------------------------------------------
// Row-wise forms on tiles of 16 rows: HMC_sampler.leap_frog (samplers.py:831-839) and E (:819-823).
template <int FAMILY, int MT, bool LEAP>
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
    vp = logit_grad<FAMILY, MT>(x, t, sd, q, g);
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

// what: 0 init, 1 iterations (ad: NULL the plain kernel, otherwise its ADAPT form), 2 rows;
// flag: REPLAY, or LEAP for the rows
template <int FAMILY, int MT>
hipError_t launch_mt(const LogitArgs& x, int what, bool flag, const hmc_adapt* ad, hipStream_t s) {
  const dim3 grid((unsigned)((x.a.ntiles + kLogitWaves - 1) / kLogitWaves)), block(64 * kLogitWaves);
  return with_bool(flag, [&](auto FLAG) {
    if (what == 0) k_logit_init<FAMILY, MT, FLAG()><<<grid, block, 0, s>>>(x);
    else if (what != 1) k_logit_rows<FAMILY, MT, FLAG()><<<grid, block, 0, s>>>(x);
    else if (ad) k_logit_iters<FAMILY, MT, FLAG(), true><<<grid, block, 0, s>>>(LogitAdaptArgs{x, *ad});
    else k_logit_iters<FAMILY, MT, FLAG(), false><<<grid, block, 0, s>>>(x);
    return hipGetLastError();
  });
}

// 16-dim output tiles per chain: 1, 2, 4 or 8 (D <= HMC_LOGIT_MAX_D = 128).  An instance runs all
// its k-steps and output tiles whatever D is (see logit_grad).
template <int FAMILY>
hipError_t launch_family(LogitArgs x, int what, bool flag, const hmc_adapt* ad, hipStream_t s) {
  if (x.a.n == 0) return hipSuccess;
  x.a.ntiles = (x.a.n + 15) / 16;
  const int mt = (x.a.D + 15) / 16;
  if (mt <= 1) return launch_mt<FAMILY, 1>(x, what, flag, ad, s);
  if (mt <= 2) return launch_mt<FAMILY, 2>(x, what, flag, ad, s);
  if (mt <= 4) return launch_mt<FAMILY, 4>(x, what, flag, ad, s);
  if (mt <= 8) return launch_mt<FAMILY, 8>(x, what, flag, ad, s);
  return hipErrorInvalidValue;
}

hipError_t launch(const LogitArgs& x, int family, int what, bool flag, hipStream_t s, const hmc_adapt* ad = nullptr) {
  switch (family) {
    case HMC_GLM_BERNOULLI: return launch_family<HMC_GLM_BERNOULLI>(x, what, flag, ad, s);
    case HMC_GLM_POISSON: return launch_family<HMC_GLM_POISSON>(x, what, flag, ad, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_logit_init(const LogitArgs& x, int family, bool replay, hipStream_t s) {
  return launch(x, family, 0, replay, s);
}
hipError_t launch_logit_iters(const LogitArgs& x, int family, bool replay, hipStream_t s, const hmc_adapt* ad) {
  return launch(x, family, 1, replay, s, ad);
}

// hmc_adapt_init: the initial adaptation state of n chains (hmc_adapt.hpp), s0 NULL: s = 1
__global__ void k_adapt_init(double* state, int64_t n, const double* s0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) adapt_store(state + i * HMC_ADAPT_STRIDE, adapt_initial(s0 ? s0[i] : 1.0));
}

hipError_t launch_adapt_init(double* state, int64_t n, const double* s0, hipStream_t s) {
  if (n == 0) return hipSuccess;
  k_adapt_init<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(state, n, s0);
  return hipGetLastError();
}
hipError_t launch_logit_rows(const LogitArgs& x, int family, bool leapfrog, hipStream_t s) {
  return launch(x, family, 2, leapfrog, s);
}

}  // namespace hmc
