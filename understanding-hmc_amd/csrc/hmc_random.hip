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
#include "hmc_internal.hpp"
#include "hmc_lane_group.hpp"
#include "hmc_random_iter.hpp"
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

template <int K>
hipError_t launch_init_k(const RandArgs& a, bool gen, bool replay, dim3 grid, hipStream_t s) {
  if (gen) {
    if (replay) k_random_init<K, true, true><<<grid, 256, 0, s>>>(a);
    else k_random_init<K, true, false><<<grid, 256, 0, s>>>(a);
  } else {
    if (replay) k_random_init<K, false, true><<<grid, 256, 0, s>>>(a);
    else k_random_init<K, false, false><<<grid, 256, 0, s>>>(a);
  }
  return hipGetLastError();
}

template <int K, bool EXACT>
hipError_t launch_iters_k2(const RandArgs& a, bool gen, bool replay, dim3 grid, hipStream_t s) {
  if (gen) {
    if (replay) k_random_iters<K, EXACT, true, true><<<grid, 256, 0, s>>>(a);
    else k_random_iters<K, EXACT, true, false><<<grid, 256, 0, s>>>(a);
  } else {
    if (replay) k_random_iters<K, EXACT, false, true><<<grid, 256, 0, s>>>(a);
    else k_random_iters<K, EXACT, false, false><<<grid, 256, 0, s>>>(a);
  }
  return hipGetLastError();
}

template <int K>
hipError_t launch_iters_k(const RandArgs& a, bool exact, bool gen, bool replay, dim3 grid, hipStream_t s) {
  return exact ? launch_iters_k2<K, true>(a, gen, replay, grid, s)
               : launch_iters_k2<K, false>(a, gen, replay, grid, s);
}

}  // namespace

// E[max of c iid U{lo..hi-1}] — the wave runs as long as its longest trajectory.
static double expected_max(int lo, int hi, int c) {
  const int n = hi - lo;
  if (n <= 1 || c <= 1) return 0.5 * (lo + hi - 1);
  double e = 0.0, prev = 0.0;
  for (int x = lo; x < hi; ++x) {
    const double F = pow((double)(x - lo + 1) / n, c);
    e += x * (F - prev);
    prev = F;
  }
  return e;
}

Layout choose_layout(int D, int L_low, int L_high) {
  static const int Ks[] = {1, 2, 4, 5, 8, 16};
  Layout best{0, 0, 0, (D + 1) / 2};
  if (const int K = force_K()) {   // debug build only: force the pairs-per-lane template
    const int lpc = (best.npairs + K - 1) / K;
    for (int k : Ks)
      if (k == K && lpc <= kWave) return Layout{K, lpc, kWave / lpc, best.npairs};
  }
  // D > 64: one wavefront per chain (hmc_wave.hip): no trajectory-length divergence inside a
  // wave, wave-uniform control flow; K pairs per lane.
  if (best.npairs > kWave / 2) {
    for (int K : {1, 2, 4, 8, 16})
      if (K * kWave >= best.npairs) return Layout{K, kWave, 1, best.npairs};
    return best;  // K = 0: unsupported
  }
  // small D: several chains per wave (lane groups); pick K by lane utilisation discounted by the
  // expected trajectory-length divergence between the chains sharing a wave
  double best_score = -1.0;
  const double mean = 0.5 * (L_low + L_high - 1);
  for (int K : Ks) {
    const int lpc = (best.npairs + K - 1) / K;
    if (lpc > kWave) continue;
    const int cpw = kWave / lpc;
    const double util = (double)best.npairs * cpw / (kWave * (double)K);
    const double emax = expected_max(L_low, L_high, cpw);
    const double score = util * (emax > 0 ? mean / emax : 1.0);
    if (score > best_score + 1e-9) {
      best_score = score;
      best.K = K;
      best.lpc = lpc;
      best.cpw = cpw;
    }
  }
  return best;
}

hipError_t launch_random_init(const RandArgs& a, const Layout& lay, bool gen, bool replay, hipStream_t s) {
  const dim3 grid = grid_for(a);
  switch (lay.K) {
    case 1: return launch_init_k<1>(a, gen, replay, grid, s);
    case 2: return launch_init_k<2>(a, gen, replay, grid, s);
    case 4: return launch_init_k<4>(a, gen, replay, grid, s);
    case 5: return launch_init_k<5>(a, gen, replay, grid, s);
    case 8: return launch_init_k<8>(a, gen, replay, grid, s);
    case 16: return launch_init_k<16>(a, gen, replay, grid, s);
  }
  return hipErrorInvalidValue;
}

// The wave-per-chain kernels (hmc_wave.hip) serve this layout.
bool wave_layout(const Layout& lay) {
  return lay.cpw == 1 && !force_group() && (lay.K == 1 || lay.K == 2 || lay.K == 4 || lay.K == 8 || lay.K == 16);
}

// Three-term leapfrog u[n+1] = (2 - (dt w)^2) u[n] - u[n-1] (hmc_wave.hip, TT): the momentum comes
// back as a difference of the last two points divided by dt, whose rounding error grows like
// eps |u| / (dt w).  Lower bound: the smallest dt w at which the NumPy model of the kernel's
// operation order keeps E within 1e-12 relative of a long-double integration over 19 steps at
// D = 100 (tests/leapfrog_model.py energy_deviation; DESIGN.md 3.1: below 1e-12 from 4.6e-4 up,
// the bound is set a factor 2 above that); upper bound: the integrator's stability limit
// dt w = 2.
// Trajectory length: the rounded coefficient c = fl(2 - (dt w)^2) turns the phase by
// (c - c_exact) / (2 sin theta) per step (cos theta = c / 2, sin theta = dt w sqrt(1 - (dt w)^2 / 4)),
// and the orbit's amplitude is |p| / sqrt(1 - (dt w)^2 / 4), so after L steps q is off by about
// |p| L |c - c_exact| / (2 dt w (1 - (dt w)^2 / 4)), with |c - c_exact| <= 2^-53 below (dt w)^2 = 2
// and <= 2^-52 from there on ((dt w)^2 is rounded in [2, 4)).  The same model (max |q - q_ld| over
// the trajectory at D = 100) stays below 2.2 x 2^-53 x L m / (dt w (1 - (dt w)^2 / 4)),
// m = 1 or 2; the bound keeps that below 5e-11, half of the 1e-10 the routing test allows
// (tests/test_leapfrog_form.py), i.e. a twentieth of FAST mode's 1e-9 on q.
// Outside the range the two-FMA loop runs.
// -DHMC_NO_THREE_TERM builds the library that never picks it (A/B).
bool leapfrog_three_term(const RandArgs& a, const Layout& lay, bool exact, bool gen) {
#ifdef HMC_NO_THREE_TERM
  return false;
#else
  constexpr double kThreeTermMinDtw = 1e-3;
  constexpr double kThreeTermMaxDrift = 2e5;   // L_high m / (dt w (1 - (dt w)^2 / 4)) at most
  if (exact || gen || !wave_layout(lay)) return false;
  const double dtw = a.dt < 0 ? -a.dt : a.dt;   // identity precision and mass: w = 1
  const double dtw2 = dtw * dtw;
  if (!(dtw2 >= kThreeTermMinDtw * kThreeTermMinDtw && dtw2 < 4.0)) return false;
  const double m = dtw2 >= 2.0 ? 2.0 : 1.0;
  return (double)a.L_high * m <= kThreeTermMaxDrift * dtw * (1.0 - 0.25 * dtw2);
#endif
}

bool full_variant(const RandArgs& a) { return a.traj_q != nullptr || instrumented(a); }

// Four chains per wavefront, one 16-lane row each (hmc_rows.hip): the shapes it is built for.  The
// kernel packs L in 24 bits for its tallies and takes no empty trajectory.
// -DHMC_NO_ROWS builds the library that never picks it (A/B).
bool rows_shape(int D, int L_low, int L_high) {
#ifdef HMC_NO_ROWS
  return false;
#else
  return D >= 97 && D <= 112 && L_low >= 1 && L_high <= (1 << 12);
#endif
}

// ... and the launches it takes: those of the production wave instance (FAST, identity target and
// mass, three-term leapfrog, Philox, no chain-0 capture or debug hooks), with a sample window whose
// rows of the wave's four chains lie within a 32-bit byte offset of the first, and so do their rows
// of the energy chains.
bool rows_kernel(const RandArgs& a, const Layout& lay, bool exact, bool gen, bool replay) {
  if (replay || full_variant(a) || !rows_shape(a.D, a.L_low, a.L_high) || !leapfrog_three_term(a, lay, exact, gen)) return false;
  if ((a.Ec || a.dEc) && 4 * (int64_t)a.Lc * 8 >= (int64_t)1 << 31) return false;
  return !a.qc || 4 * (int64_t)a.Lq * a.D * 8 < (int64_t)1 << 31;
}

hipError_t launch_random_iters(const RandArgs& a, const Layout& lay, bool exact, bool gen, bool replay,
                               hipStream_t s) {
  if (rows_kernel(a, lay, exact, gen, replay)) return launch_rows_iters(a, s);
  if (wave_layout(lay))
    return launch_wave_iters(a, lay.K, exact, gen, replay, leapfrog_three_term(a, lay, exact, gen), s);
  const dim3 grid = grid_for(a);
  switch (lay.K) {
    case 1: return launch_iters_k<1>(a, exact, gen, replay, grid, s);
    case 2: return launch_iters_k<2>(a, exact, gen, replay, grid, s);
    case 4: return launch_iters_k<4>(a, exact, gen, replay, grid, s);
    case 5: return launch_iters_k<5>(a, exact, gen, replay, grid, s);
    case 8: return launch_iters_k<8>(a, exact, gen, replay, grid, s);
    case 16: return launch_iters_k<16>(a, exact, gen, replay, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace hmc
