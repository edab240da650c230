// hmc_logit.hpp — argument block and launchers of the generalized-linear-model kernels: the
// Random-trajectory kernels (hmc_logit.hip) and the NUTS kernel (hmc_glm_nuts.hip).
#pragma once
#include <type_traits>

#include "hmc_internal.hpp"

namespace hmc {

// The Random-trajectory argument block (schedule, kinetic part, replay streams, state, outputs;
// its MVN target fields q0 / prec / logc and its lane-group fields are unused) plus the data and,
// for the row-wise entries, the rows.
struct LogitArgs {
  RandArgs a;
  int nrows;               // data rows n, 1 .. HMC_LOGIT_MAX_N
  int64_t ldx;             // row stride of X in doubles, >= D
  const double* X;         // [n][ldx]
  const double* y;         // [n] 0.0 / 1.0 (Bernoulli), counts (Poisson)
  const double* pprec;     // [D] 1 / prior variance
  const double* row_p;     // row-wise entries: [n][D] inputs ...
  const double* row_q;
  double* row_po;          // ... and outputs (leapfrog)
  double* row_qo;
  double* row_E;           // [n] (energy)
};

// The argument block of the ADAPT forms of the iteration kernels (per-chain step multiplier and its
// warm-up adaptation, hmc_adapt.hpp): the plain kernels' block, then the caller's hmc_adapt.  The
// plain kernels take LogitArgs as before, so their argument layout and code do not change.
struct LogitAdaptArgs : LogitArgs {
  hmc_adapt ad;
};

// family: HMC_GLM_BERNOULLI (the logistic target) or HMC_GLM_POISSON; a template parameter of the
// kernels, so it is no part of the argument block.
hipError_t launch_logit_init(const LogitArgs& x, int family, bool replay, hipStream_t s);
// ad: NULL launches the plain kernel; otherwise its ADAPT form on LogitAdaptArgs{x, *ad}
hipError_t launch_logit_iters(const LogitArgs& x, int family, bool replay, hipStream_t s,
                              const hmc_adapt* ad = nullptr);
hipError_t launch_adapt_init(double* state, int64_t n, const double* s0, hipStream_t s);
hipError_t launch_logit_rows(const LogitArgs& x, int family, bool leapfrog, hipStream_t s);

// NUTS on a GLM target (hmc_glm_nuts.hip): one wave owns a tile of 16 chains for the whole launch;
// a.ws is the tile-interleaved workspace of glm_nuts_ws_doubles(n, D, d_max) doubles (the tree
// vectors, then one replay-tape cursor per chain), a.tape / a.tape_stride the replay tape.
int64_t glm_nuts_ws_doubles(int64_t n, int D, int d_max);   // 0: unsupported D
hipError_t launch_glm_nuts(const LogitArgs& x, int family, bool replay, hipStream_t s,
                           const hmc_adapt* ad = nullptr);   // ad: as launch_logit_iters

}  // namespace hmc
