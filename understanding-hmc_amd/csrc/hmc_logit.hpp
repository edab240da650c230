// hmc_logit.hpp — argument block and launchers of the logistic-regression kernels (hmc_logit.hip).
#pragma once
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
  const double* y;         // [n] 0.0 / 1.0
  const double* pprec;     // [D] 1 / prior variance
  const double* row_p;     // row-wise entries: [n][D] inputs ...
  const double* row_q;
  double* row_po;          // ... and outputs (leapfrog)
  double* row_qo;
  double* row_E;           // [n] (energy)
};

hipError_t launch_logit_init(const LogitArgs& x, bool replay, hipStream_t s);
hipError_t launch_logit_iters(const LogitArgs& x, bool replay, hipStream_t s);
hipError_t launch_logit_rows(const LogitArgs& x, bool leapfrog, hipStream_t s);

}  // namespace hmc
