// hmc_mix.hpp — argument block and launchers of the Gaussian-mixture kernels (hmc_mix.hip).
#pragma once
#include "hmc_internal.hpp"

namespace hmc {

// The Random-trajectory argument block (schedule, kinetic part, replay streams, state, outputs;
// its MVN target fields q0 / prec / logc are unused) plus the mixture and, for the row-wise
// entries, the rows.
struct MixArgs {
  RandArgs a;
  int Kc;                // components, 1 .. HMC_MIX_MAX_COMPONENTS
  const double* logw;    // [Kc]
  const double* mu;      // [Kc][D]
  const double* prec;    // [Kc][D]
  const double* ldc;     // [Kc]  D*log(2 pi) + sum_d log var_kd
  const double* row_p;   // row-wise entries: [n][D] inputs ...
  const double* row_q;
  double* row_po;        // ... and outputs (leapfrog)
  double* row_qo;
  double* row_E;         // [n] (energy)
};

hipError_t launch_mix_init(const MixArgs& m, const Layout& lay, bool replay, hipStream_t s);
hipError_t launch_mix_iters(const MixArgs& m, const Layout& lay, bool replay, hipStream_t s);
hipError_t launch_mix_rows(const MixArgs& m, const Layout& lay, bool leapfrog, hipStream_t s);

}  // namespace hmc
