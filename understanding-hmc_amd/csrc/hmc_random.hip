// hmc_random.hip — fused Random-trajectory HMC iterations for diagonal-precision MVN targets.
//
// Replaces the hot triple loop of HMC_sampler.gen_sample_random (samplers.py:410 -> :428 -> :448)
// and its primitives K / E / p_sample / leap_frog (samplers.py:811-839) for targets whose
// precision inv(cov0) is diagonal (identity in BASELINE configs 1, 2, 4).
//
// One launch runs iterations [it0, it1) of every chain: state q stays in registers across
// iterations, each iteration does
//     p ~ N(0, cov_p)                      (replay stream or in-kernel Philox + Box–Muller)
//     E0 = V(q) + K(p)                     -> E_chain / dE_chain row            (Q14)
//     L  ~ U{L_low..L_high-1}              (Q1)
//     L x leap_frog with the gradient of q_new reused as the next step's q_old (bit-identical)
//     E1, dE = E1 - E0, accept iff dE < 0 or log u < -dE
//     store q_chain row (i - warm_up)//thin  (last write of a thinned row wins, as in Python)
// HBM traffic per chain-iteration: one q_chain row (8D B) + E + dE (16 B); q is read/written
// once per launch.  The arithmetic is fp64 VALU; EXACT mode keeps the reference's operation
// order with no FMA contraction (built with -ffp-contract=off), so for diagonal targets the
// sampled states are bit-identical to the NumPy reference on replayed streams.
#include "hmc_debug.hpp"
#include "hmc_device.hpp"
#include "hmc_dispatch.hpp"
#include "hmc_internal.hpp"
#include "hmc_lane_group.hpp"
#include "hmc_random_iter.hpp"
#include "hmc_route.hpp"
#include "hmc_target_ops.hpp"

namespace hmc {

namespace {

template <int K, bool GEN>
__device__ __forceinline__ double chain_energy(const RandArgs& a, const Lane& ln, const int (&kk)[K],
                                               const bool (&pv)[K], const double (&q)[2 * K],
                                               const double (&p)[2 * K]) {
  // E = V + K = 0.5*(logdet_const + (q-q0)^T P (q-q0)) + p^T Minv p / 2  (utils.py:218, samplers.py:817),
  // summed as one group reduction of the per-coordinate terms.
  double maha = 0.0, kin = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (pv[j]) {
      const int d = 2 * kk[j];
      energy_terms<GEN>(dim_const<GEN>(a, d), q[2 * j], p[2 * j], maha, kin);
      if (d + 1 < a.D) energy_terms<GEN>(dim_const<GEN>(a, d + 1), q[2 * j + 1], p[2 * j + 1], maha, kin);
    }
  }
  const double tot = group_sum(maha + kin, ln.s, a.lpc, ln.base);
  return 0.5 * (a.logc + tot);
}

// ------------------------------------------------------------------------------------------
// Chain initialisation (samplers.py:413-420): q_chain[:,0] = q_start, E_chain[:,0] = E(q, p0).
template <int K, bool GEN, bool REPLAY>
__global__ __launch_bounds__(256) void k_random_init(RandArgs a) {
  const Lane ln = lane_info(a);
  int kk[K];
  bool pv[K];
  double q[2 * K], p[2 * K];
  lane_slots<K>(a, ln, kk, pv);
  load_row<K>(a.qstart + ln.c * (int64_t)a.D, a, kk, pv, q);
  draw_momentum<K, GEN, REPLAY>(a, ln, 0, kk, pv, p);
  const double E0 = chain_energy<K, GEN>(a, ln, kk, pv, q, p);
  store_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  if (a.qc && a.q_row0 == 0) store_row<K>(a.qc + ln.c * (int64_t)a.Lq * a.D, a, kk, pv, q);
  if (ln.leader) store_init_energy(a, ln.c, E0);
}

// ------------------------------------------------------------------------------------------
// Iterations [it0, it1) (samplers.py:428-475).
template <int K, bool EXACT, bool GEN, bool REPLAY>
__global__ __launch_bounds__(256) void k_random_iters(RandArgs a) {
  PhaseTimer<6> tm(a);   // debug build's phase timers (hmc_debug.hpp has the legend)
  const unsigned long long t_start = tm.now();
  const Lane ln = lane_info(a);
  const uint64_t gc = (uint64_t)(a.chain_offset + ln.c);
  int kk[K];
  bool pv[K];
  double q[2 * K], p[2 * K], qi[2 * K], t[2 * K];
  lane_slots<K>(a, ln, kk, pv);
  load_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  double Eprev = ln.active ? a.Eprev[ln.c] : 0.0;
  RandomTally tally;
  int it_base = a.it0 - a.lpc, draw_L = 0;     // cached (L, log u) draws (Philox mode)
  double draw_lnu = 0.0;
  // Retire the state loads here: the wait-count pass otherwise sees them pending at the loop
  // header and emits vmcnt(0) inside the loop, which (loads and stores share one in-order
  // counter on gfx950) stalls every iteration on the previous iteration's sample stores.
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) only

  for (int it = a.it0; it < a.it1; ++it) {
    // ---- momentum resample (samplers.py:431) and initial energy (:434)
    tm.start();
    if (!ablate(a, kAblateMomentum)) {
      draw_momentum<K, GEN, REPLAY>(a, ln, it, kk, pv, p);
    } else {
#pragma unroll
      for (int e = 0; e < 2 * K; ++e) p[e] = 0.3;
    }
    tm.lap(0);
    const double E0 = ablate(a, kAblateEnergy) ? 0.0 : chain_energy<K, GEN>(a, ln, kk, pv, q, p);
    tm.lap(1);
    const bool post = it >= a.wu;
    const bool write_row = stores_row(a, it);
    const int64_t row = row_of(a, it);
    if (ln.leader && write_row && !ablate(a, kAblateRowStores)) {       // :436-438 (Q14)
      __builtin_nontemporal_store(E0, a.Ec + ln.c * (int64_t)a.Lc + row);
      __builtin_nontemporal_store(E0 - Eprev, a.dEc + ln.c * (int64_t)a.Lc + row);
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
      if (ablate(a, kAblateL12)) L = 12;
      if (ablate(a, kAblateZeroL)) L = 0;
      if (!ln.active) L = 0;
    }

    tm.lap(2);
    // ---- chain-0 trajectory capture (samplers.py:442-452): lane holding dims 0,1 records q[:2]
    const bool cap = a.traj_q && (gc == 0) && (it <= a.n_save) && ln.leader;
    double* capp = cap ? a.traj_q + (int64_t)(it - 1) * a.traj_stride * 2 : nullptr;
    if (cap) {
      capp[0] = q[0];
      capp[1] = a.D > 1 ? q[1] : q[0];
    }

    // ---- L leapfrog steps (:448-450 -> :831-839)
#pragma unroll
    for (int e = 0; e < 2 * K; ++e) qi[e] = q[e];
    if constexpr (EXACT) {
#pragma unroll
      for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) t[2 * j + h] = kick<GEN>(slot_const<GEN>(a, kk[j], h, pv[j]), q[2 * j + h]);
      }
      for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int e = 2 * j + h;
            const DimConst c = slot_const<GEN>(a, kk[j], h, pv[j]);
            const double ph = p[e] - t[e];              // p_half = p_old - dt*(M^-1 dVdq(q_old))/2
            q[e] = q[e] + c.dt * ph;                    // q_new  = q_old + dt*p_half
            t[e] = kick<GEN>(c, q[e]);                  // dt*(M^-1 dVdq(q_new))/2, reused next step
            p[e] = ph - t[e];                           // p_new  = p_half - ...
          }
        }
        if (cap) {
          capp[2 * (l + 1)] = q[0];
          capp[2 * (l + 1) + 1] = a.D > 1 ? q[1] : q[0];
        }
      }
    } else {
      for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int e = 2 * j + h;
            const DimConst c = slot_const<GEN>(a, kk[j], h, pv[j]);
            const double cc = GEN ? c.hd * (c.minv * c.prec) : c.hd;
            const double ph = __builtin_fma(-cc, q[e] - c.q0, p[e]);
            q[e] = __builtin_fma(c.dt, ph, q[e]);
            p[e] = __builtin_fma(-cc, q[e] - c.q0, ph);
          }
        }
        if (cap) {
          capp[2 * (l + 1)] = q[0];
          capp[2 * (l + 1) + 1] = a.D > 1 ? q[1] : q[0];
        }
      }
    }
    // lanes whose slot is past D carry zeros; keep them zero
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (!pv[j] || 2 * kk[j] + 1 >= a.D) {
        q[2 * j + 1] = 0.0;
        p[2 * j + 1] = 0.0;
        if (!pv[j]) q[2 * j] = p[2 * j] = 0.0;
      }
    }

    tm.lap(3);
    // ---- final energy and Metropolis test (:455-472)
    const double E1 = ablate(a, kAblateEnergy) ? 0.0 : chain_energy<K, GEN>(a, ln, kk, pv, q, p);
    tm.lap(4);
    const double dE = E1 - E0;
    const bool accept = (dE < 0.0) || (lnu < -dE);
    if (!accept) {
#pragma unroll
      for (int e = 0; e < 2 * K; ++e) q[e] = qi[e];
    }
    if (write_row && a.qc && !ablate(a, kAblateRowStores) && row >= a.q_row0)
      store_row<K>(a.qc + (ln.c * (int64_t)a.Lq + row % a.Lq) * a.D, a, kk, pv, q);
    if (cap) {
      a.traj_len[it - 1] = (L > 0 ? L : 0) + 1;
      a.decision[it - 1] = accept ? 1 : 0;
    }
    if (ln.leader) tally.count(a, it, post, accept, L);
    tm.lap(5);
  }

  // ---- state write-back and counters
  store_row<K>(a.q + ln.c * (int64_t)a.D, a, kk, pv, q);
  if (ln.leader) a.Eprev[ln.c] = Eprev;
  if (tm.on() && ln.lane == 0) {
    unsigned long long* row = tm.store((int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave));
    row[6] = t_start;
    row[7] = tm.now();
    stamp_hw_id(row + 5);
  }
  tally.flush(a, ln.lane, (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave));
}

}  // namespace

hipError_t launch_random_init(const RandArgs& a, const RandomRoute& r, bool replay, hipStream_t s) {
  return with_value<1, 2, 4, 5, 8, 16>(r.lay.K, [&](auto K) {
    return with_bool(r.gen, [&](auto GEN) {
      return with_bool(replay, [&](auto REPLAY) {
        k_random_init<K(), GEN(), REPLAY()><<<grid_for(a), 256, 0, s>>>(a);
        return hipGetLastError();
      });
    });
  });
}

hipError_t launch_random_iters(const RandArgs& a, const RandomRoute& r, bool exact, bool replay, hipStream_t s) {
  if (r.kernel == RandomKernel::Rows) return launch_rows_iters(a, s);
  if (r.kernel == RandomKernel::Wave) return launch_wave_iters(a, r.lay.K, exact, r.gen, replay, r.three_term, r.full, s);
  if (r.kernel != RandomKernel::Groups) return hipErrorInvalidValue;
  return with_value<1, 2, 4, 5, 8, 16>(r.lay.K, [&](auto K) {
    return with_bool(exact, [&](auto EXACT) {
      return with_bool(r.gen, [&](auto GEN) {
        return with_bool(replay, [&](auto REPLAY) {
          k_random_iters<K(), EXACT(), GEN(), REPLAY()><<<grid_for(a), 256, 0, s>>>(a);
          return hipGetLastError();
        });
      });
    });
  });
}

}  // namespace hmc
