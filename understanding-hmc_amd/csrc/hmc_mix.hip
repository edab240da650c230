// hmc_mix.hip — fused Random-trajectory HMC iterations for a mixture of Kc Gaussians with diagonal
// covariances: the first target that is not a multivariate normal.
//
// Replaces HMC_sampler.gen_sample_random (samplers.py:387-491) and leap_frog / E (:811-839) for
//     V(q) = -log sum_k w_k N(q; mu_k, diag var_k).
// The layout and the Philox keying (hmc_lane_group.hpp), the row bookkeeping (Q5, Q14, thinning) and
// the counters (hmc_random_iter.hpp) are those of the lane-group kernel (hmc_random.hip): a chain's D
// coordinates live in lpc consecutive lanes of a wave64, lane s owning pairs k = s + lpc*j (j < K);
// cpw chains share a wave; above 64 dims one wave holds one chain (lpc = 64).  The state stays in
// registers across the fused iterations.
//
// One gradient evaluation at q (every per-chain scalar is a lane-group shuffle reduction, no LDS):
//     m_k  = sum_d prec_kd (q_d - mu_kd)^2          two components' partial sums per shuffle tree
//     l_k  = logw_k - 0.5 (logdet_const_k + m_k)
//     M    = max_k l_k;  S = sum_k exp(l_k - M)      (the max-shift: S >= 1, no underflow to log 0)
//     V(q) = -(M + log S)                            falls out of the gradient pass
//     r_k  = exp(l_k - M) / S
//     g_d  = sum_k r_k prec_kd (q_d - mu_kd)
// mu and prec (2 Kc D doubles, at most 64 KB) are read through the vector cache in both passes:
// every wave of the launch reads the same lines, so they stay in L2 / the CU's cache.
//
// Leapfrog with the reference's Q3 semantics (samplers.py:831-839), as the diagonal kernels:
//     p_half = p - dt_d (minv_d g_d) / 2;  q += dt_d p_half;  g = grad(q);  p = p_half - dt_d (minv_d g_d) / 2
// with the gradient at q_new reused as the next step's q_old gradient.  E = V(q) + sum p_d minv_d p_d / 2;
// accept iff (dE < 0) || (log u < -dE): a NaN or infinite energy rejects.
//
// One arithmetic for both fp_mode values: exp and log are ~1 ulp fdlibm-style fp64 (fast_exp and
// fast_log of hmc_device.hpp), which cannot be bit-identical to NumPy's, so there is no EXACT
// instance.  Built with -ffp-contract=off; the FMAs are explicit.
#include "hmc_device.hpp"
#include "hmc_dispatch.hpp"
#include "hmc_lane_group.hpp"
#include "hmc_mix.hpp"
#include "hmc_random_iter.hpp"

namespace hmc {

namespace {

constexpr int kMixK = HMC_MIX_MAX_COMPONENTS;

// Byte offsets, inside a [D] row, of a lane's coordinates 2k and 2k+1: 32-bit, computed once per
// launch, so that every table load is a uniform row base plus a VGPR offset.  A padding slot (or a
// lane without a chain) gets a clamped, valid offset; valid says which of the two are real.
struct PairAt {
  uint32_t o0, o1;
  bool v0, v1;
};
__device__ __forceinline__ PairAt pair_at(int D, int k, bool pv) {
  return PairAt{(uint32_t)min(2 * k, D - 1) * 8u, (uint32_t)min(2 * k + 1, D - 1) * 8u, pv, pv && 2 * k + 1 < D};
}
__device__ __forceinline__ double at(const double* row, uint32_t off) {
  return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(row) + off);
}

// l[c] of a register-resident array for a wave-uniform index c, as a select chain: the component
// loops below are rolled, and a dynamically indexed array would live in scratch.  The empty asm
// keeps the optimiser from folding the chain back into such an indexed access.
__device__ __forceinline__ double pinned(double v) {
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double comp_get(const double (&l)[kMixK], int c) {
  double v = pinned(l[0]);
#pragma unroll
  for (int i = 1; i < kMixK; ++i) v = (c == i) ? pinned(l[i]) : v;
  return v;
}
__device__ __forceinline__ void comp_set(double (&l)[kMixK], int c, double v) {
#pragma unroll
  for (int i = 0; i < kMixK; ++i) l[i] = (c == i) ? v : pinned(l[i]);
}

// The lane's share of m_c = sum_d prec_cd (q_d - mu_cd)^2.  Padding coordinates get a zero
// precision: they add nothing here and get a zero gradient below.
template <int K>
__device__ __forceinline__ double maha_part(const MixArgs& m, int c, const PairAt (&at_)[K], const double (&q)[2 * K]) {
  const double* mu = m.mu + (int64_t)c * m.a.D;
  const double* pr = m.prec + (int64_t)c * m.a.D;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double r0 = at(pr, at_[j].o0), r1 = at(pr, at_[j].o1);     // unconditional loads, then a select
    const double pr0 = at_[j].v0 ? r0 : 0.0, pr1 = at_[j].v1 ? r1 : 0.0;
    const double x0 = q[2 * j] - at(mu, at_[j].o0), x1 = q[2 * j + 1] - at(mu, at_[j].o1);
    acc = __builtin_fma(pr0 * x0, x0, acc);
    acc = __builtin_fma(pr1 * x1, x1, acc);
  }
  return acc;
}

// g += r prec_c (q - mu_c) over the lane's coordinates.
template <int K>
__device__ __forceinline__ void grad_part(const MixArgs& m, int c, double r, const PairAt (&at_)[K],
                                          const double (&q)[2 * K], double (&g)[2 * K]) {
  const double* mu = m.mu + (int64_t)c * m.a.D;
  const double* pr = m.prec + (int64_t)c * m.a.D;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double r0 = at(pr, at_[j].o0), r1 = at(pr, at_[j].o1);     // unconditional loads, then a select
    const double pr0 = at_[j].v0 ? r0 : 0.0, pr1 = at_[j].v1 ? r1 : 0.0;
    g[2 * j] = __builtin_fma(r * pr0, q[2 * j] - at(mu, at_[j].o0), g[2 * j]);
    g[2 * j + 1] = __builtin_fma(r * pr1, q[2 * j + 1] - at(mu, at_[j].o1), g[2 * j + 1]);
  }
}

// V(q) and g = dV/dq(q) of the lane's coordinates.  Called by every lane of the wave together
// (the shuffles read the neighbours of the group).  The component loops are rolled: unrolled, the
// scheduler hoists the 2 Kc K pair loads of a pass and the K >= 8 instances spill.
template <int K>
__device__ __forceinline__ double mix_grad(const MixArgs& m, const Lane& ln, const PairAt (&at_)[K],
                                           const double (&q)[2 * K], double (&g)[2 * K]) {
  constexpr int kStep = K < 8 ? 2 : 1;   // 8 pairs per lane: one component per pass fits the registers
  const int lpc = m.a.lpc;
  double l[kMixK];
#pragma unroll
  for (int c = 0; c < kMixK; ++c) l[c] = 0.0;
  // ---- l_c, two components per pass: their partial sums walk one shuffle tree together
  double M = -__builtin_inf();
#pragma unroll 1
  for (int c = 0; c < m.Kc; c += kStep) {
    const bool two = kStep == 2 && c + 1 < m.Kc;
    double a0 = maha_part<K>(m, c, at_, q);
    double a1 = two ? maha_part<K>(m, c + 1, at_, q) : 0.0;
    double m0, m1;
    if (lpc == kWave) {       // one chain per wave: both sums in one DPP pass (lanes 31 and 63)
      const double v = wave_sum2_dpp(a0, a1);
      m0 = readlane_d(v, 31);
      m1 = readlane_d(v, 63);
    } else {
      for (int off = 1; off < lpc; off <<= 1) {
        const double o0 = __shfl_down(a0, off, kWave), o1 = __shfl_down(a1, off, kWave);
        if (ln.s + off < lpc) {
          a0 += o0;
          a1 += o1;
        }
      }
      m0 = __shfl(a0, ln.base, kWave);
      m1 = __shfl(a1, ln.base, kWave);
    }
    const double l0 = m.logw[c] - 0.5 * (m.ldc[c] + m0);
    M = l0 > M ? l0 : M;
    comp_set(l, c, l0);
    if (two) {
      const double l1 = m.logw[c + 1] - 0.5 * (m.ldc[c + 1] + m1);
      M = l1 > M ? l1 : M;
      comp_set(l, c + 1, l1);
    }
  }
  double S = 0.0;
#pragma unroll
  for (int c = 0; c < kMixK; ++c) {
    if (c < m.Kc) {
      l[c] = fast_exp(l[c] - M);
      S += l[c];
    }
  }
  // the largest term is exp(0) = 1, so 1 <= S <= Kc unless q is not finite (every m_k infinite or
  // NaN): V = +inf then, which the Metropolis test rejects
  const bool finite = S >= 1.0;
  const double rS = rcp_nr(S);
  const double V = finite ? -(M + fast_log(S)) : __builtin_inf();
#pragma unroll
  for (int e = 0; e < 2 * K; ++e) g[e] = 0.0;
#pragma unroll 1
  for (int c = 0; c < m.Kc; c += kStep) {   // two components per pass: twice the loads in flight
    grad_part<K>(m, c, comp_get(l, c) * rS, at_, q, g);
    if (kStep == 2 && c + 1 < m.Kc) grad_part<K>(m, c + 1, comp_get(l, c + 1) * rS, at_, q, g);
  }
  return V;
}

// Per-coordinate step dt_d and half kick factor dt_d minv_d / 2 of the lane's slots, read once per
// launch and kept in registers; a padding slot never touches the per-dimension arrays.
template <int K>
__device__ __forceinline__ void step_consts(const RandArgs& a, const int (&kk)[K], const bool (&pv)[K],
                                            double (&dtc)[2 * K], double (&hk)[2 * K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = 2 * kk[j] + h, e = 2 * j + h;
      dtc[e] = a.dt;
      hk[e] = a.h;
      if (pv[j] && d < a.D) {
        if (a.dtv) {
          dtc[e] = a.dtv[d];
          hk[e] = dtc[e] * 0.5;
        }
        if (a.minv) hk[e] *= a.minv[d];
      }
    }
  }
}

// K(p) = sum p_d minv_d p_d / 2 (samplers.py:817 with a diagonal inv(cov_p)); padding slots hold p = 0.
template <int K>
__device__ __forceinline__ double kinetic(const RandArgs& a, const Lane& ln, const int (&kk)[K],
                                          const double (&p)[2 * K]) {
  double kin = 0.0;
  if (a.minv) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      kin = __builtin_fma(p[2 * j], a.minv[min(2 * kk[j], a.D - 1)] * p[2 * j], kin);
      kin = __builtin_fma(p[2 * j + 1], a.minv[min(2 * kk[j] + 1, a.D - 1)] * p[2 * j + 1], kin);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 2 * K; ++e) kin = __builtin_fma(p[e], p[e], kin);
  }
  return 0.5 * group_sum(kin, ln.s, a.lpc, ln.base);
}

// First half of samplers.py:831-839: p_half (left in p) and q_new.
template <int K>
__device__ __forceinline__ void kick_drift(const double (&dtc)[2 * K], const double (&hk)[2 * K],
                                           const double (&g)[2 * K], double (&p)[2 * K], double (&q)[2 * K]) {
#pragma unroll
  for (int e = 0; e < 2 * K; ++e) {
    p[e] = __builtin_fma(-hk[e], g[e], p[e]);
    q[e] = __builtin_fma(dtc[e], p[e], q[e]);
  }
}

// Second half: p_new = p_half - dt (minv g(q_new)) / 2.
template <int K>
__device__ __forceinline__ void kick(const double (&hk)[2 * K], const double (&g)[2 * K], double (&p)[2 * K]) {
#pragma unroll
  for (int e = 0; e < 2 * K; ++e) p[e] = __builtin_fma(-hk[e], g[e], p[e]);
}

template <int K>
__device__ __forceinline__ void slots(const RandArgs& a, const Lane& ln, int (&kk)[K], bool (&pv)[K],
                                      PairAt (&at_)[K]) {
  lane_slots<K>(a, ln, kk, pv);
#pragma unroll
  for (int j = 0; j < K; ++j) at_[j] = pair_at(a.D, kk[j], pv[j]);
}

// ------------------------------------------------------------------------------------------
// Chain initialisation (samplers.py:413-420): q_chain[:,0] = q_start, E_chain[:,0] = E(q, p0).
template <int K, bool REPLAY>
__global__ __launch_bounds__(256) void k_mix_init(MixArgs m) {
  const RandArgs& a = m.a;
  const Lane ln = lane_info(a);
  int kk[K];
  bool pv[K];
  PairAt at_[K];
  double q[2 * K], p[2 * K], g[2 * K];
  slots<K>(a, ln, kk, pv, at_);
  load_row<K>(a.qstart + ln.c * (int64_t)a.D, a, kk, pv, q);
  draw_momentum<K, true, REPLAY>(a, ln, 0, kk, pv, p);
  const double E0 = mix_grad<K>(m, ln, at_, q, g) + kinetic<K>(a, ln, kk, p);
  store_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  if (a.qc && a.q_row0 == 0) store_row<K>(a.qc + ln.c * (int64_t)a.Lq * a.D, a, kk, pv, q);
  if (ln.leader) store_init_energy(a, ln.c, E0);
}

// ------------------------------------------------------------------------------------------
// Iterations [it0, it1) (samplers.py:428-475).
template <int K, bool REPLAY>
__global__ __launch_bounds__(256) void k_mix_iters(MixArgs m) {
  const RandArgs& a = m.a;
  const Lane ln = lane_info(a);
  const uint64_t gc = (uint64_t)(a.chain_offset + ln.c);
  int kk[K];
  bool pv[K];
  PairAt at_[K];
  double q[2 * K], p[2 * K], qi[2 * K], g[2 * K], dtc[2 * K], hk[2 * K];
  slots<K>(a, ln, kk, pv, at_);
  step_consts<K>(a, kk, pv, dtc, hk);
  load_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  double Eprev = ln.active ? a.Eprev[ln.c] : 0.0;
  RandomTally tally;
  int it_base = a.it0 - a.lpc, draw_L = 0;     // cached (L, log u) draws (Philox mode)
  double draw_lnu = 0.0;

  for (int it = a.it0; it < a.it1; ++it) {
    // ---- momentum resample (samplers.py:431) and initial energy (:434); the same pass gives the
    // gradient the first half kick needs
    draw_momentum<K, true, REPLAY>(a, ln, it, kk, pv, p);
    double V = mix_grad<K>(m, ln, at_, q, g);
    const double E0 = V + kinetic<K>(a, ln, kk, p);
    const bool post = it >= a.wu;
    const bool write_row = stores_row(a, it);
    const int64_t row = row_of(a, it);
    if (ln.leader && write_row) {                        // :436-438 (Q14)
      if (a.Ec) __builtin_nontemporal_store(E0, a.Ec + ln.c * (int64_t)a.Lc + row);
      if (a.dEc) __builtin_nontemporal_store(E0 - Eprev, a.dEc + ln.c * (int64_t)a.Lc + row);
    }
    Eprev = E0;                                          // :460

    // ---- trajectory length (:441) and log-uniform for the MH test (:461)
    int L;
    double lnu;
    if constexpr (REPLAY) {
      L = ln.active ? a.rL[ln.c * (int64_t)a.niter + (it - 1)] : 0;
      lnu = ln.active ? a.rlnu[ln.c * (int64_t)a.niter + (it - 1)] : 0.0;
    } else {
      // lane s of the group draws (L, u) of iteration it_base + s once per LPC iterations;
      // iteration it reads them from lane base + (it - it_base)
      if (it - it_base >= a.lpc) {
        it_base = it;
        const TrajDraw d = draw_traj(a, it + ln.s, gc);
        draw_L = d.L;
        draw_lnu = d.lnu;
      }
      L = __shfl(draw_L, ln.base + (it - it_base), kWave);
      lnu = __shfl(draw_lnu, ln.base + (it - it_base), kWave);
      if (!ln.active) L = 0;
    }

    // ---- chain-0 trajectory capture (samplers.py:442-452): lane holding dims 0,1 records q[:2]
    const bool cap = a.traj_q && (gc == 0) && (it <= a.n_save) && ln.leader;
    double* capp = cap ? a.traj_q + (int64_t)(it - 1) * a.traj_stride * 2 : nullptr;
    if (cap) {
      capp[0] = q[0];
      capp[1] = a.D > 1 ? q[1] : q[0];
    }

    // ---- L leapfrog steps (:448-450 -> :831-839).  The wave steps as long as its longest
    // trajectory; every lane takes part in each gradient (its shuffles), a chain that has done its
    // L steps stands still (the gradient of an unchanged q is the one it already holds).
#pragma unroll
    for (int e = 0; e < 2 * K; ++e) qi[e] = q[e];
    const int Lmax = wave_max_i32(L);
    for (int l = 0; l < Lmax; ++l) {
      const bool on = l < L;
      if (on) kick_drift<K>(dtc, hk, g, p, q);
      const double Vn = mix_grad<K>(m, ln, at_, q, g);
      if (on) {
        kick<K>(hk, g, p);
        V = Vn;
        if (cap) {
          capp[2 * (l + 1)] = q[0];
          capp[2 * (l + 1) + 1] = a.D > 1 ? q[1] : q[0];
        }
      }
    }

    // ---- final energy and Metropolis test (:455-472)
    const double E1 = V + kinetic<K>(a, ln, kk, p);
    const double dE = E1 - E0;
    const bool accept = (dE < 0.0) || (lnu < -dE);
    if (!accept) {
#pragma unroll
      for (int e = 0; e < 2 * K; ++e) q[e] = qi[e];
    }
    if (write_row && a.qc && row >= a.q_row0) store_row<K>(a.qc + (ln.c * (int64_t)a.Lq + row % a.Lq) * a.D, a, kk, pv, q);
    if (cap) {
      a.traj_len[it - 1] = (L > 0 ? L : 0) + 1;
      a.decision[it - 1] = accept ? 1 : 0;
    }
    if (ln.leader) tally.count(a, it, post, accept, L);
  }

  // ---- state write-back and counters
  store_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  if (ln.leader) a.Eprev[ln.c] = Eprev;
  tally.flush(a, ln.lane, (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave));
}

// ------------------------------------------------------------------------------------------
// Row-wise forms, one row per lane group: HMC_sampler.leap_frog (samplers.py:831-839) and E (:819-823).
template <int K, bool LEAP>
__global__ __launch_bounds__(256) void k_mix_rows(MixArgs m) {
  const RandArgs& a = m.a;
  const Lane ln = lane_info(a);
  int kk[K];
  bool pv[K];
  PairAt at_[K];
  double q[2 * K], p[2 * K], g[2 * K];
  slots<K>(a, ln, kk, pv, at_);
  load_row<K>(m.row_q + ln.c * (int64_t)a.D, a, kk, pv, q);
  load_row<K>(m.row_p + ln.c * (int64_t)a.D, a, kk, pv, p);
  const double V = mix_grad<K>(m, ln, at_, q, g);
  if constexpr (LEAP) {
    double dtc[2 * K], hk[2 * K];
    step_consts<K>(a, kk, pv, dtc, hk);
    kick_drift<K>(dtc, hk, g, p, q);
    mix_grad<K>(m, ln, at_, q, g);
    kick<K>(hk, g, p);
    store_row<K>(m.row_po + ln.c * (int64_t)a.D, a, kk, pv, p);
    store_row<K>(m.row_qo + ln.c * (int64_t)a.D, a, kk, pv, q);
  } else {
    const double E = V + kinetic<K>(a, ln, kk, p);
    if (ln.leader) m.row_E[ln.c] = E;
  }
}

template <int K>
hipError_t launch_k(const MixArgs& m, int what, bool flag, hipStream_t s) {
  const dim3 grid = grid_for(m.a);
  switch (what) {
    case 0:
      if (flag) k_mix_init<K, true><<<grid, 256, 0, s>>>(m);
      else k_mix_init<K, false><<<grid, 256, 0, s>>>(m);
      break;
    case 1:
      if (flag) k_mix_iters<K, true><<<grid, 256, 0, s>>>(m);
      else k_mix_iters<K, false><<<grid, 256, 0, s>>>(m);
      break;
    default:
      if (flag) k_mix_rows<K, true><<<grid, 256, 0, s>>>(m);
      else k_mix_rows<K, false><<<grid, 256, 0, s>>>(m);
      break;
  }
  return hipGetLastError();
}

hipError_t launch(const MixArgs& m, const Layout& lay, int what, bool flag, hipStream_t s) {
  if (m.a.n == 0) return hipSuccess;
  return with_value<1, 2, 4, 5, 8>(lay.K, [&](auto K) { return launch_k<K()>(m, what, flag, s); });
}

}  // namespace

hipError_t launch_mix_init(const MixArgs& m, const Layout& lay, bool replay, hipStream_t s) {
  return launch(m, lay, 0, replay, s);
}
hipError_t launch_mix_iters(const MixArgs& m, const Layout& lay, bool replay, hipStream_t s) {
  return launch(m, lay, 1, replay, s);
}
hipError_t launch_mix_rows(const MixArgs& m, const Layout& lay, bool leapfrog, hipStream_t s) {
  return launch(m, lay, 2, leapfrog, s);
}

}  // namespace hmc
