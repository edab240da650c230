// hmc_route.hpp — which kernel a Random-sampler call runs, decided once (hmc_route.cpp) and read by
// the launch entries, the host queries and the workspace sizing alike.
#pragma once
#include "hmc_internal.hpp"

namespace hmc {

enum class RandomKernel {
  Big,      // large D, chain state in the workspace (hmc_big.hip): dense D > 128, diagonal D > 2048
  Dense,    // dense precision in 16-dim MFMA tiles (hmc_dense.hip)
  Rows,     // four chains per wavefront, 97 <= D <= 112 (hmc_rows.hip)
  Wave,     // one wavefront per chain (hmc_wave.hip)
  Groups,   // several chains per wavefront in lane groups (hmc_random.hip)
};

struct RandomRoute {
  RandomKernel kernel;
  Layout lay;            // Groups / Wave: the lane-group layout; Rows: the four-chain shape; Big / Dense: flat_layout.
                         // The argument block copies it; hmc_rows.hip reads only npairs, debug stamp rows go by cpw.
  bool gen;              // general diagonal target / kinetic (q0, prec, minv, p_scale or dt_vec set)
  bool three_term;       // the FAST leapfrog in its three-term form (hmc_wave.hip, TT)
  bool full;             // the FULL iteration instances: chain-0 capture or the debug build's hooks
                         // (launch_wave_iters takes it; the four-chain kernel has no such instance)
  int64_t order_bytes;   // what this call reads or writes of state.order (0: none)
};

// The route of a chain-init call (init: the layout is chosen for the schedule's trajectory range, or
// the reference's default (5, 20) where the caller left it unset, and no iteration kernel is picked
// beyond its family) or of an iteration call.  st NULL: a production launch, i.e. no chain-0
// capture, sample window within the four-chain kernel's offsets, no workspace.  k NULL (layout
// queries only): identity mass, and the three-term rule taken as met wherever the mode and the
// target allow it.
RandomRoute random_route(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_state* st,
                         bool init);

// What of hmc_state both the route and the argument block read: whether the call captures chain 0's
// trajectory, and the rows per chain of the q_chain window.
inline bool captures_chain0(const hmc_state* st) {
  return st->traj_q && st->traj_len && st->decision && st->n_save > 0;
}
inline int window_rows(const hmc_schedule* s, const hmc_state* st) {
  return st->qc_rows > 0 ? (int)st->qc_rows : s->L_chain;
}

// RandomRoute::order_bytes on its own (the sized entries check it before anything else runs).
int64_t random_order_bytes(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_state* st);

// Bytes of state.order the Random sampler needs for n chains (0: none); k NULL: enough for either cov_p.
int64_t random_workspace_bytes(const hmc_target* t, const hmc_kinetic* k, int64_t n);

// The diagonal-target launches of a route (hmc_random.hip): chain init, and iterations [it0, it1) by
// the four-chain, the wave-per-chain or the lane-group kernel.
hipError_t launch_random_init(const RandArgs& a, const RandomRoute& r, bool replay, hipStream_t s);
hipError_t launch_random_iters(const RandArgs& a, const RandomRoute& r, bool exact, bool replay, hipStream_t s);

// The trajectory range a lane-group layout is chosen for at chain init: the schedule's, or the
// reference's default (5, 20) when the caller left it unset (init draws no trajectory length).
struct TrajRange { int lo, hi; };
TrajRange init_traj_range(const hmc_schedule* s);

Layout flat_layout(int D);  // no lane groups (dense, large-D, GLM and NUTS argument blocks): only npairs
Layout mix_layout(int D, int L_low, int L_high);   // the lane-group layout with at most 8 pairs per lane

}  // namespace hmc
