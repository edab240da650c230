// hmc_glm_nuts.hip — the reference's NUTS engine (samplers.py:495-808, utils.py:222-385) on a
// generalized-linear-model target (include/hmc.h: hmc_glm): Bernoulli (logistic) and Poisson
// regression.
//
// Semantics follow gen_sample_NUTS exactly, as hmc_nuts.hip does for MVN targets (quirks Q10-Q12:
// doubling until BOTH ends U-turn, the biased sub-tree acceptance, the running-max energy weights;
// the |E - E_init| > 1000 guard; d_max).  The per-chain scalar bookkeeping (save slots, check points,
// weights, draws, the row rule, the counter flush) is hmc_nuts_tree.hpp; the tile, its gradient
// logit_grad<FAMILY, MT> (both products on the f64 matrix cores), the half kicks, the kinetic
// energy and the momentum draw are hmc_glm_ops.hpp, shared with the Random kernels (hmc_logit.hip).
//
// Execution model, deliberately simpler than hmc_nuts.hip (no work queue, no chain hand-offs): one
// wave owns a fixed tile of 16 chains for the whole launch, lane (c = lane & 15, h = lane >> 4)
// holding dims h + 4m of chain c.  Every chain is its own state machine on per-lane scalars
// (identical in a chain's four lanes), and the wave advances in steps:
//   1. transitions of the chains between sub-trees: iteration end (q <- live old point, row store),
//      iteration start (momentum draw), sub-tree start (direction draw, that boundary's q, p, g);
//   2. kick_drift for the chains inside a sub-tree, under the EXEC mask;
//   3. one logit_grad pass for the whole wave; a chain at its iteration start takes part without
//      having moved: the pass gives its E_init = V + K(p) and the gradient both boundaries start from;
//   4. the second kick for the in-tree chains, then E = V + K for every chain;
//   5. the new point: unstable check, odd point -> save slot, even point -> the U-turn checks
//      against check_points, looped to the wave's largest count; progressive sampling; at the
//      sub-tree's last point the boundary store, the biased acceptance and the termination test.
// Every cross-lane operation (the MFMAs, chain_sum4, wave_max_i32) runs in converged control flow;
// chains that sit out a branch are masked and move no bytes.  The chains of a tile run through the
// launch's iterations independently (no barrier per iteration); the launch ends when every chain
// of the tile has finished iteration it1 - 1.
//
// The vectors a tree keeps per chain live in the caller's workspace, zero padded to 16 MT dims and
// tile-interleaved: element (tile, vec, m, lane) at ((tile nvec + vec) 4 MT + m) 64 + lane, so one
// register's load or store is one contiguous 512-byte access of the wave (a chain-contiguous layout
// would give 32-byte pieces).  nvec = 8 + 2 (d_max + 1): the two live points (their names swap on
// acceptance), left q, p, g, right q, p, g, and d_max + 1 save slots of (q, p).  (GlmNutsLayout)
#include "hmc_dispatch.hpp"
#include "hmc_glm_ops.hpp"
#include "hmc_nuts_layout.hpp"
#include "hmc_nuts_tree.hpp"

namespace hmc {

namespace {

// S_START: draws its momentum in the next transitions; S_INIT: waits for the gradient pass at its
// start point; S_SUB: starts a sub-tree in the next transitions; S_TREE: inside a sub-tree;
// S_END: ends its iteration in the next transitions.
enum : int { S_START = 0, S_INIT = 1, S_SUB = 2, S_TREE = 3, S_END = 4, S_DONE = 5 };

// workspace vector ids of a chain: live points 0 and 1 (`old` names the old one), then the ends
enum : int { V_LIVE = 0, V_LEFT = 2, V_RIGHT = 5, V_SLOTS = 8 };
static_assert(V_SLOTS == GlmNutsLayout::kFixedVecs, "the save slots follow the layout's fixed vectors");

// The wave's tile block, addressed through a wave-uniform buffer descriptor (SGPR base, 32-bit lane
// offset, constant part of the offset in the instruction): no 64-bit address per (vector, m) is
// kept live across the step loop, and an offset past the block could neither read nor write.
// A vector is named v + vl: v a constant of the call site, vl per lane (a chain's save slot, live
// point or end differs from its neighbours').
struct TileWS {
  __amdgpu_buffer_rsrc_t r;
  int lane_off;   // lane * 8
};
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int M>
__device__ __forceinline__ double ws_get(const TileWS& w, int v, int vl, int m) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(w.r, w.lane_off + vl * (M * kWave * 8),
                                                                         (v * M + m) * (kWave * 8), 0));
}
template <int M>
__device__ __forceinline__ void ws_put(const TileWS& w, int v, int vl, int m, double x) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, x), w.r, w.lane_off + vl * (M * kWave * 8),
                                        (v * M + m) * (kWave * 8), 0);
}
template <int M>
__device__ __forceinline__ void ws_store(const TileWS& w, int v, int vl, const double (&x)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) ws_put<M>(w, v, vl, m, x[m]);
}
template <int M>
__device__ __forceinline__ void ws_store_neg(const TileWS& w, int v, int vl, const double (&x)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) ws_put<M>(w, v, vl, m, -x[m]);
}
template <int M>
__device__ __forceinline__ void ws_load(const TileWS& w, int v, int vl, double (&x)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = ws_get<M>(w, v, vl, m);
}
template <int MT>
__device__ __forceinline__ void ws_store_g(const TileWS& w, int v, int vl, const d4 (&g)[MT]) {
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) ws_put<4 * MT>(w, v, vl, m, gval<MT>(g, m));
}
template <int MT>
__device__ __forceinline__ void ws_load_g(const TileWS& w, int v, int vl, d4 (&g)[MT]) {
#pragma unroll
  for (int m = 0; m < 4 * MT; ++m) g[m >> 2][m & 3] = ws_get<4 * MT>(w, v, vl, m);
}
// A = (q - qv).p and B = (q - qv).pv for the vectors qv = v + vl, pv = v + vl + 1, streamed (the
// lane's share; padding dims hold zeros everywhere)
template <int M>
__device__ __forceinline__ void ws_dots(const TileWS& w, int v, int vl, const double (&q)[M], const double (&p)[M],
                                        double& A, double& B) {
  A = B = 0.0;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const double dq = q[m] - ws_get<M>(w, v, vl, m);
    A = __builtin_fma(dq, p[m], A);
    B = __builtin_fma(dq, ws_get<M>(w, v + 1, vl, m), B);
  }
}

// ADAPT: every chain runs at its own multiple s of the step and adapts it during warm-up
// (hmc_adapt.hpp).  The lane holds its chain's state for the launch; the acceptance statistic is
// accumulated where a new point's energy is formed (step 5) and the update runs in the iteration-end
// transition, all on per-lane scalars.  With ADAPT = false none of it is compiled and the kernel
// takes the plain argument block: those instances are the code they were before the ADAPT form.
template <bool ADAPT>
using NutsKernelArgs = std::conditional_t<ADAPT, LogitAdaptArgs, LogitArgs>;

template <int FAMILY, int MT, bool REPLAY, bool ADAPT>
__global__ __launch_bounds__(64 * kLogitWaves) __attribute__((amdgpu_waves_per_eu(kItersWaves<MT>, kItersWaves<MT>)))
void k_glm_nuts(NutsKernelArgs<ADAPT> x) {
  constexpr int M = 4 * MT;
  const RandArgs& a = x.a;
  __shared__ DimTable sd;
  __shared__ double s_ntab[REPLAY ? 2 : kNormalTableDoubles];   // Box-Muller tables (Philox momentum)
  if constexpr (!REPLAY) init_normal_tables(s_ntab);             // synchronised by stage_dims
  stage_dims(x, sd);
  const TileLane t = tile_lane(a.n, a.D);
  if (t.tile >= a.ntiles) return;            // wave-uniform; no block barrier follows
  const uint64_t gc = (uint64_t)(a.chain_offset + t.c);
  const GlmNutsLayout L(a.n, MT, a.d_max);
  const int64_t tile = (int64_t)blockIdx.x * kLogitWaves + uniform_i(threadIdx.x / kWave);   // t.tile, in SGPRs
  const TileWS w{__builtin_amdgcn_make_buffer_rsrc(a.ws + L.slots(tile), 0, (int)(L.tile_doubles * 8), 0x00020000),
                 t.lane * 8};
  // L.cursors, through the tile count the launcher took from the same layout (launch_mt): dividing
  // a.n again here costs the Bernoulli MT = 8 replay ADAPT instance 16 bytes of scratch per lane
  int64_t* const tcur = reinterpret_cast<int64_t*>(a.ws + a.ntiles * L.tile_doubles) + t.tile * 16 + t.c16;

  double q[M], p[M];
  d4 g[MT];
  load_dims<MT>(a.q + t.c * (int64_t)a.D, t, q);
#pragma unroll
  for (int m = 0; m < M; ++m) p[m] = 0.0;
  double Eprev = t.live ? a.Eprev[t.c] : 0.0;
  int64_t tpos = (REPLAY && t.live) ? *tcur : 0;       // replay tape cursor (persists across launches)

  int state = (t.live && a.it0 < a.it1) ? S_START : S_DONE;
  int it = a.it0;
  int d = 0, k = 0, Lsub = 1, udir = 0, ndraw = 0, old = 0;
  double E_init = 0.0, E_max_now = 0.0, E_max_old = 0.0, pi_new = 1.0, pi_old = 1.0;   // TreeWeights
  unsigned long long n_lf = 0, n_unst = 0, n_dmax = 0, n_tape = 0, n_steps = 0;
  // ADAPT: the chain's state, the multiplier of the current iteration, the sum of the point
  // statistics of its tree and their number
  hmc_adapt ax{};
  AdaptParams adp{};
  AdaptState ad{};
  double s = 1.0, alpha_sum = 0.0;
  int alpha_n = 0;
  if constexpr (ADAPT) {
    ax = x.ad;
    adp = AdaptParams{ax.delta, ax.gamma, ax.t0, ax.kappa};
    ad = t.live ? adapt_load(ax.state + t.c * HMC_ADAPT_STRIDE) : adapt_initial(1.0);
    s = adapt_scale(ad, it < ax.adapt_end);
  }

  auto draw = [&](bool direction) {                     // next random number of this chain (reference order)
    if constexpr (REPLAY) return NutsDraws::tape(tpos, a, n_tape, t.c, direction);
    else return NutsDraws::philox(ndraw, it, gc, a, direction);
  };

  while (true) {
    // ================= 1. transitions
    if (state == S_END) {                               // samplers.py:786-791: q = live_point_q_old
      ws_load<M>(w, V_LIVE, old, q);
      const int qrow = (it - a.wu) / a.thin;
      if (stores_row(a, it) && a.qc && qrow >= a.q_row0) {
        double* rowp = a.qc + (t.c * (int64_t)a.Lq + qrow % a.Lq) * a.D;
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (dim_ok(t, m)) rowp[t.h + 4 * m] = q[m];
      }
      Eprev = E_init;                                   // :787
      if constexpr (ADAPT) {                            // every tree has a first point: alpha_n >= 1
        adapt_iteration(ad, adp, it < ax.adapt_end, alpha_sum / (double)alpha_n);
        s = adapt_scale(ad, it + 1 < ax.adapt_end);
        alpha_sum = 0.0;
        alpha_n = 0;
      }
      ++it;
      state = it < a.it1 ? S_START : S_DONE;
    }
    if (state == S_START) {                             // momentum (:565); E_init after the gradient pass
      draw_momentum<MT, REPLAY, true>(a, t, sd, it, gc, s_ntab, p);
      state = S_INIT;
    }
    if (state == S_SUB) {                               // :601-614: direction, that end's q, p, g
      udir = (int)draw(true);
      const int b = udir == 0 ? V_RIGHT - V_LEFT : 0;
      ws_load<M>(w, V_LEFT, b, q);
      ws_load<M>(w, V_LEFT + 1, b, p);
      ws_load_g<MT>(w, V_LEFT + 2, b, g);
      k = 0;
      state = S_TREE;
    }
    if (!__builtin_amdgcn_ballot_w64(state != S_DONE)) break;

    // ================= 2.-4. one leapfrog for every chain inside a sub-tree (:612-614, :639)
    const bool act = state == S_TREE;
    if (act) kick_drift<MT, ADAPT>(t, sd, g, p, q, s);
    const double vp = logit_grad<FAMILY, MT>(x, t, sd, q, g);
    if (act) kick<MT, ADAPT>(t, sd, g, p, s);
    const double E = chain_sum4(vp + kinetic_part<MT>(t, sd, p));   // :569 / :618 / :643
    if (act && t.h == 0) ++n_lf;
    ++n_steps;

    if (state == S_INIT) {                              // iteration start (:569-590)
      E_init = E;
      if (stores_row(a, it) && t.h == 0) {              // :571-573
        const int64_t row = t.c * (int64_t)a.Lc + (it - a.wu) / a.thin;
        if (a.Ec) a.Ec[row] = E_init;
        if (a.dEc) a.dEc[row] = E_init - Eprev;
      }
      ws_store<M>(w, V_LIVE, old, q);                   // live_point_q_old = q (:577)
      ws_store<M>(w, V_LEFT, 0, q);                     // left = (q, -p), right = (q, p) (:581-584)
      ws_store_neg<M>(w, V_LEFT + 1, 0, p);
      ws_store_g<MT>(w, V_LEFT + 2, 0, g);
      ws_store<M>(w, V_RIGHT, 0, q);
      ws_store<M>(w, V_RIGHT + 1, 0, p);
      ws_store_g<MT>(w, V_RIGHT + 2, 0, g);
      E_max_old = E_init;
      pi_old = 1.0;
      d = 0;
      Lsub = 1;
      ndraw = 0;
      state = S_SUB;
    }

    // ================= 5. the new point
    bool reject = false, sub_end = false;
    const int mpt = k + 1;                              // point number within the sub-tree
    const bool first = act && k == 0, later = act && k > 0;
    if constexpr (ADAPT) {
      if (act) {                                        // every point whose energy is evaluated
        alpha_sum += adapt_alpha(E - E_init, E);
        ++alpha_n;
      }
    }
    if (first) {                                        // first point (:617-626)
      ws_store<M>(w, V_LIVE, 1 - old, q);               // live_point_new
      E_max_now = E;
      pi_new = 1.0;
      ws_store<M>(w, V_SLOTS, 2 * a.d_max, q);          // point 1: save_slot(1) = d_max
      ws_store<M>(w, V_SLOTS + 1, 2 * a.d_max, p);
      k = 1;
      sub_end = Lsub == 1;
    } else if (later) {
      if (fabs(E - E_init) > 1000.0) {                  // :647-651
        reject = true;
        if (t.h == 0) ++n_unst;
      } else if (mpt & 1) {                             // odd point: save (:654-658)
        const int s = save_slot(mpt, a.d_max);
        ws_store<M>(w, V_SLOTS, 2 * s, q);
        ws_store<M>(w, V_SLOTS + 1, 2 * s, p);
      }
    }
    // even point: U-turn checks against check_points(mpt) (:699-736), looped to the wave's largest
    // count.  Forward the ends are left = (q_check, -p_check), right = (q, p), backward left = (q, p),
    // right = (q_check, -p_check): both reduce, up to exact sign flips, to A = (q - q_check).p and
    // B = (q - q_check).p_check, and the sub-tree is rejected when both are negative (:727-732).
    const bool checking = later && !reject && (mpt & 1) == 0;
    CheckPoints cp(checking ? mpt : 2);
    int ncheck = checking ? cp.count() : 0;
    const int ncheck_w = wave_max_i32(ncheck);
    for (int ci = 0; ci < ncheck_w; ++ci) {
      const bool doit = ci < ncheck;
      double A = 0.0, B = 0.0;
      if (doit) ws_dots<M>(w, V_SLOTS, 2 * save_slot(cp.pt, a.d_max), q, p, A, B);   // retrieve_save_index (:715)
      A = chain_sum4(A);
      B = chain_sum4(B);
      if (doit) {
        if (A < 0.0 && B < 0.0) {
          reject = true;
          ncheck = 0;
        } else {
          cp.next();                                    // (release, :735-736: nothing to free)
        }
      }
    }
    if (later && !reject) {                             // progressive sampling (:743-751)
      const auto wt = TreeWeights::add_point(E_max_now, pi_new, E);
      E_max_now = wt.E_max_now;
      pi_new = wt.pi_new;
      if (draw(false) < wt.r) ws_store<M>(w, V_LIVE, 1 - old, q);
      ++k;
      sub_end = k == Lsub;
    }
    if (act && reject) state = S_END;                   // q = live_point_q_old (:649, :731, :754)

    // ================= sub-tree end: boundary, biased acceptance, termination (:757-784)
    // A = (q - q_other).p, B = (q - q_other).p_other; (right, left) term dots = (A, -B) forward,
    // (-B, A) backward: the reference's terms up to exact sign flips
    double tA = 0.0, tB = 0.0;
    if (sub_end) {
      const int b = udir == 0 ? V_RIGHT - V_LEFT : 0;   // this end <- (q, p, g), after the other's dots
      ws_dots<M>(w, V_LEFT, V_RIGHT - V_LEFT - b, q, p, tA, tB);
      ws_store<M>(w, V_LEFT, b, q);
      ws_store<M>(w, V_LEFT + 1, b, p);
      ws_store_g<MT>(w, V_LEFT + 2, b, g);
    }
    tA = chain_sum4(tA);
    tB = chain_sum4(tB);
    if (sub_end) {
      const auto wt = TreeWeights::merge(E_max_now, pi_new, E_max_old, pi_old);   // :766-771 (Q11)
      E_max_old = wt.E_max_old;
      pi_old = wt.pi_old;
      if (draw(false) < wt.A) old = 1 - old;            // :773-775: old <- new, as a swap of names
      const bool rterm = (udir == 0 ? tA : -tB) < 0.0;  // :779-784 (Q10: stop when BOTH ends turn)
      const bool lterm = (udir == 0 ? -tB : tA) < 0.0;
      ++d;
      if (lterm && rterm) {
        state = S_END;
      } else if (d > a.d_max - 1) {                     // :596-598 (the reference aborts the run)
        if (t.h == 0) ++n_dmax;
        state = S_END;
      } else {
        Lsub = 1 << d;
        state = S_SUB;
      }
    }
  }

  // ---- state write-back and counters
  store_dims<MT>(a.q + t.c * (int64_t)a.D, t, q);
  if (t.live && t.h == 0) {
    a.Eprev[t.c] = Eprev;
    if constexpr (REPLAY) *tcur = tpos;
    if constexpr (ADAPT) adapt_store(ax.state + t.c * HMC_ADAPT_STRIDE, ad);
  }
  n_lf = wave_sum_u64(n_lf);
  n_unst = wave_sum_u64(n_unst);
  n_dmax = wave_sum_u64(n_dmax);
  n_tape = wave_sum_u64(t.h == 0 ? n_tape : 0ull);
  if (t.lane == 0) nuts_flush_counters(a.cnt, tile, n_lf, n_unst, n_dmax, n_tape, n_steps);
}

template <int FAMILY, int MT>
hipError_t launch_mt(const LogitArgs& x0, bool replay, const hmc_adapt* ad, hipStream_t s) {
  LogitArgs x = x0;
  x.a.ntiles = GlmNutsLayout(x.a.n, MT, x.a.d_max).tiles;
  const dim3 grid((unsigned)((x.a.ntiles + kLogitWaves - 1) / kLogitWaves)), block(64 * kLogitWaves);
  return with_bool(replay, [&](auto REPLAY) {
    if (ad) k_glm_nuts<FAMILY, MT, REPLAY(), true><<<grid, block, 0, s>>>(LogitAdaptArgs{x, *ad});
    else k_glm_nuts<FAMILY, MT, REPLAY(), false><<<grid, block, 0, s>>>(x);
    return hipGetLastError();
  });
}

// 16-dim tiles per chain of the instance that runs D: 1, 2, 4 or 8 (0: D out of range)
int glm_tiles(int D) {
  if (D < 1 || D > HMC_LOGIT_MAX_D) return 0;
  const int mt = (D + 15) / 16;
  return mt <= 1 ? 1 : mt <= 2 ? 2 : mt <= 4 ? 4 : 8;
}

template <int FAMILY>
hipError_t launch_family(const LogitArgs& x, bool replay, const hmc_adapt* ad, hipStream_t s) {
  return with_value<1, 2, 4, 8>(glm_tiles(x.a.D), [&](auto MT) { return launch_mt<FAMILY, MT()>(x, replay, ad, s); });
}

}  // namespace

int64_t glm_nuts_ws_doubles(int64_t n, int D, int d_max) {
  const int MT = glm_tiles(D);
  if (!MT || n < 0 || d_max < 1 || d_max > kNutsDmaxMax) return 0;
  return GlmNutsLayout(n, MT, d_max).total;
}

hipError_t launch_glm_nuts(const LogitArgs& x, int family, bool replay, hipStream_t s, const hmc_adapt* ad) {
  if (x.a.n == 0 || x.a.it1 <= x.a.it0) return hipSuccess;
  switch (family) {
    case HMC_GLM_BERNOULLI: return launch_family<HMC_GLM_BERNOULLI>(x, replay, ad, s);
    case HMC_GLM_POISSON: return launch_family<HMC_GLM_POISSON>(x, replay, ad, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace hmc
