// hmc_route.cpp — the Random sampler's kernel choice (hmc_route.hpp): every condition that sends a
// call to one kernel family, layout or leapfrog form stands here and nowhere else.
#include "hmc_route.hpp"

#include <cmath>

#include "hmc_debug.hpp"

namespace hmc {

namespace {

constexpr int kWave = 64;   // lanes of a wavefront; hmc_device.hpp's own is behind device-only code

// Large D (hmc_big.hip): dense targets past the MFMA tiles, diagonal ones past 16 pairs per lane.
bool big_path(bool dense, int D) { return dense ? dense_tiles(D) == 0 : (D + 1) / 2 > 16 * kWave; }

bool general_diag(const hmc_target* t, const hmc_kinetic* k) {
  return t->q0 || t->prec || (k && (k->minv || k->p_scale || k->dt_vec));
}

// E[max of c iid U{lo..hi-1}] — the wave runs as long as its longest trajectory.
double expected_max(int lo, int hi, int c) {
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
  Layout best = flat_layout(D);
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
    return best;  // K = 0: past 16 pairs per lane, which big_path takes
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

// The wave-per-chain kernels (hmc_wave.hip) serve this layout.
bool wave_layout(const Layout& lay) {
  return lay.cpw == 1 && !force_group() && (lay.K == 1 || lay.K == 2 || lay.K == 4 || lay.K == 8 || lay.K == 16);
}

// Three-term leapfrog u[n+1] = (2 - (dt w)^2) u[n] - u[n-1] (hmc_wave.hip, TT): wave-per-chain
// layout, FAST mode, identity target and mass with a scalar dt inside the range where recovering
// the momentum from the last two points is safe.  The momentum comes back as a difference of the
// last two points divided by dt, whose rounding error grows like eps |u| / (dt w).  Lower bound: the
// smallest dt w at which the NumPy model of the kernel's operation order keeps E within 1e-12
// relative of a long-double integration over 19 steps at D = 100 (tests/leapfrog_model.py
// energy_deviation; DESIGN.md 3.1: below 1e-12 from 4.6e-4 up, the bound is set a factor 2 above
// that); upper bound: the integrator's stability limit dt w = 2.
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
bool leapfrog_three_term(double dt, int L_high, const Layout& lay, bool exact, bool gen) {
#ifdef HMC_NO_THREE_TERM
  return false;
#else
  constexpr double kThreeTermMinDtw = 1e-3;
  constexpr double kThreeTermMaxDrift = 2e5;   // L_high m / (dt w (1 - (dt w)^2 / 4)) at most
  if (exact || gen || !wave_layout(lay)) return false;
  const double dtw = dt < 0 ? -dt : dt;   // identity precision and mass: w = 1
  const double dtw2 = dtw * dtw;
  if (!(dtw2 >= kThreeTermMinDtw * kThreeTermMinDtw && dtw2 < 4.0)) return false;
  const double m = dtw2 >= 2.0 ? 2.0 : 1.0;
  return (double)L_high * m <= kThreeTermMaxDrift * dtw * (1.0 - 0.25 * dtw2);
#endif
}

// Whether a launch takes the FULL instances of the iteration kernels (chain-0 capture and, in the
// debug build, the hooks of hmc_debug.hpp) instead of the production ones.
bool full_variant(const hmc_state* st) { return (st && captures_chain0(st)) || instrumented(); }

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
bool rows_kernel(const hmc_target* t, const hmc_schedule* s, const hmc_state* st, bool three_term, bool full) {
  if (s->rng_mode == HMC_RNG_REPLAY || full || !three_term || !rows_shape(t->D, s->L_low, s->L_high)) return false;
  if (!st) return true;
  if ((st->E_chain || st->dE_chain) && 4 * (int64_t)s->L_chain * 8 >= (int64_t)1 << 31) return false;
  return !st->q_chain || 4 * (int64_t)window_rows(s, st) * t->D * 8 < (int64_t)1 << 31;
}

}  // namespace

Layout flat_layout(int D) { return Layout{0, 0, 0, (D + 1) / 2}; }

TrajRange init_traj_range(const hmc_schedule* s) {
  return s->L_high > s->L_low ? TrajRange{s->L_low, s->L_high} : TrajRange{5, 20};
}

// choose_layout's lane groups, except that 16 pairs per lane (two lanes per chain) become 8 pairs
// on twice the lanes: with the gradient's component rows in flight a 16-pair instance does not fit
// the register file.  choose_layout's scoring never picks 16 pairs for D <= 64
// (tests/test_layout_query.py enumerates it) and the wave-per-chain shapes up to HMC_MIX_MAX_D take
// at most 4, so only HMC_FORCE_K = 16 in the debug build (hmc_debug.hpp) reaches the
// remap.  Results do not depend on the layout.
Layout mix_layout(int D, int L_low, int L_high) {
  Layout lay = choose_layout(D, L_low, L_high);
  if (lay.K == 16) {
    lay.K = 8;
    lay.lpc = (lay.npairs + 7) / 8;
    lay.cpw = kWave / lay.lpc;
  }
  return lay;
}

int64_t random_workspace_bytes(const hmc_target* t, const hmc_kinetic* k, int64_t n) {
  const bool dense = t->kind == HMC_TARGET_DENSE;
  if (big_path(dense, t->D)) return big_workspace_bytes(n, t->D, dense, !k || k->minv_full);
  return dense ? dense_workspace_bytes(n, t->D) : 0;
}

int64_t random_order_bytes(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_state* st) {
  return st && st->order && s->n_chains > 0 ? random_workspace_bytes(t, k, s->n_chains) : 0;
}

RandomRoute random_route(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_state* st,
                         bool init) {
  RandomRoute r{};
  const bool dense = t->kind == HMC_TARGET_DENSE;
  r.order_bytes = random_order_bytes(t, k, s, st);
  r.lay = flat_layout(t->D);
  if (big_path(dense, t->D) || dense) {
    r.kernel = big_path(dense, t->D) ? RandomKernel::Big : RandomKernel::Dense;
    return r;
  }
  const TrajRange L = init ? init_traj_range(s) : TrajRange{s->L_low, s->L_high};
  r.lay = choose_layout(t->D, L.lo, L.hi);
  r.gen = general_diag(t, k);
  r.full = full_variant(st);
  const bool exact = s->fp_mode == HMC_MODE_EXACT;
  r.three_term = k ? leapfrog_three_term(k->dt, s->L_high, r.lay, exact, r.gen)
                   : !exact && !r.gen && wave_layout(r.lay);
  if (!init && rows_kernel(t, s, st, r.three_term, r.full)) {
    r.kernel = RandomKernel::Rows;
    r.lay = Layout{4, 16, 4, r.lay.npairs};   // 16 lanes per chain with 7 coordinates each
  } else {
    r.kernel = wave_layout(r.lay) ? RandomKernel::Wave : RandomKernel::Groups;
  }
  return r;
}

}  // namespace hmc
