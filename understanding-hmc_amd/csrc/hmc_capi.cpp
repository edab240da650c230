// hmc_capi.cpp — extern "C" entry points of libhmc.so (declared in include/hmc.h).
//
// Validation mirrors the reference's asserts (samplers.py:331-348, :396) and returns
// HMC_EINVAL instead of raising; the Python mirror re-raises AssertionError.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <unordered_map>

#include "hmc.h"
#include "hmc_debug.hpp"
#include "hmc_internal.hpp"
#include "hmc_logit.hpp"
#include "hmc_mix.hpp"
#include "hmc_pred.hpp"
#include "hmc_route.hpp"
#include "hmc_select.hpp"

namespace {

thread_local std::string g_err;

hmc_status fail(hmc_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return st;
}

hmc_status hip_status(hipError_t e, const char* where) {
  if (e == hipSuccess) return HMC_OK;
  return fail(HMC_EHIP, "%s: %s", where, hipGetErrorString(e));
}

// Python floor division (the reference computes (i - warm_up)//thin with Python ints).
int64_t floordiv(int64_t a, int64_t b) {
  int64_t q = a / b;
  if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
  return q;
}

hmc_status check_schedule(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, bool random) {
  if (!t || !k || !s) return fail(HMC_EINVAL, "null target/kinetic/schedule");
  if (t->D < 1) return fail(HMC_EINVAL, "D must be >= 1");
  if (t->kind != HMC_TARGET_DIAG && t->kind != HMC_TARGET_DENSE) return fail(HMC_EINVAL, "bad target kind");
  if (t->kind == HMC_TARGET_DENSE && !t->prec) return fail(HMC_EINVAL, "dense target needs prec");
  if (s->n_chains < 0) return fail(HMC_EINVAL, "n_chains < 0");
  if (s->n_iter < 1 || s->thin < 1 || s->warm_up < 0) return fail(HMC_EINVAL, "bad Niter/thin/warm_up");
  const int64_t Lc = 1 + floordiv(s->n_iter - s->warm_up, s->thin);  // samplers.py:31
  if (Lc < 1 || Lc != s->L_chain) return fail(HMC_EINVAL, "L_chain must be 1+(Niter-warm_up)//thin >= 1");
  if (!(std::isfinite(k->dt)) && !k->dt_vec) return fail(HMC_EINVAL, "dt must be set (samplers.py:332)");
  if (random && s->L_high <= s->L_low) return fail(HMC_EINVAL, "L_low must be < L_high (randint)");
  if (random && s->rng_mode == HMC_RNG_PHILOX && s->L_low < 0) return fail(HMC_EINVAL, "L_low < 0");
  if (s->rng_mode != HMC_RNG_REPLAY && s->rng_mode != HMC_RNG_PHILOX) return fail(HMC_EINVAL, "bad rng_mode");
  if (s->fp_mode != HMC_MODE_EXACT && s->fp_mode != HMC_MODE_FAST) return fail(HMC_EINVAL, "bad fp_mode");
  return HMC_OK;
}

// q_chain buffer geometry shared by the Random and NUTS kernels: the kernels index one chain's
// rows with 32-bit row numbers (row % Lq), so a chain's rows must stay within 2 GiB.
hmc_status check_window(const hmc_target* t, const hmc_schedule* s, const hmc_state* st) {
  if (st->qc_rows < 0 || st->qc_row0 < 0) return fail(HMC_EINVAL, "qc_rows, qc_row0 must be >= 0");
  if (st->qc_rows > 0x7FFFFFFFll || st->qc_row0 > 0x7FFFFFFFll) return fail(HMC_EINVAL, "qc_rows/qc_row0 too large");
  if ((st->qc_rows > 0 ? st->qc_rows : (int64_t)s->L_chain) * t->D * 8 > 0x7FFFFFFFll)
    return fail(HMC_ENOTSUP, "one chain's q_chain rows exceed 2 GiB (use a streaming window)");
  return HMC_OK;
}

// Dense mass matrix (full cov_p, samplers.py:352-356): only the dense-target Random kernels take it.
hmc_status check_mass(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s) {
  if (!k->minv_full && !k->p_chol_t && !k->kick) return HMC_OK;
  if (!k->minv_full || !k->kick) return fail(HMC_EINVAL, "dense mass matrix needs minv_full and kick");
  if (k->minv || k->p_scale) return fail(HMC_EINVAL, "dense mass matrix: minv/p_scale must be NULL");
  if (t->kind != HMC_TARGET_DENSE) return fail(HMC_ENOTSUP, "dense mass matrix needs a dense target (pass prec dense)");
  if (s && s->rng_mode == HMC_RNG_PHILOX && !k->p_chol_t)
    return fail(HMC_EINVAL, "dense mass matrix with Philox draws needs p_chol_t");
  return HMC_OK;
}

hmc_status check_iter_range(const hmc_schedule* s) {
  if (s->iter_begin < 1 || s->iter_end < s->iter_begin || s->iter_end > s->n_iter + 1)
    return fail(HMC_EINVAL, "iteration range must satisfy 1 <= begin <= end <= Niter+1");
  return HMC_OK;
}

// What the chain-init entries (MVN, mixture, GLM) check alike once the target and the schedule have
// passed.  *run: there are chains to initialise; HMC_OK without it is the entry's answer (empty batch).
hmc_status check_chain_init(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                            const double* q_start, const hmc_state* st, bool* run) {
  *run = false;
  if (!st) return fail(HMC_EINVAL, "null state");
  if (hmc_status e = check_mass(t, k, s)) return e;
  if (s->n_chains == 0) return HMC_OK;   // empty batch: zero-size buffers may be NULL
  if (!st->q || !st->E_prev || !q_start) return fail(HMC_EINVAL, "null state/q_start");
  if (s->rng_mode == HMC_RNG_REPLAY && (!r || !r->p0)) return fail(HMC_EINVAL, "replay mode needs p0");
  *run = true;
  return HMC_OK;
}

// What the Random iteration entries (MVN, mixture, GLM) check alike once the target and the schedule
// have passed, in the order the entries have always checked it.  *run: there is something to launch;
// HMC_OK without it is the entry's answer (empty batch or empty iteration range).
hmc_status check_random_iters(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                              const hmc_state* st, bool* run) {
  *run = false;
  if (!st) return fail(HMC_EINVAL, "null state");
  if (hmc_status e = check_window(t, s, st)) return e;
  if (hmc_status e = check_mass(t, k, s)) return e;
  if (hmc_status e = check_iter_range(s)) return e;
  if (s->n_chains == 0) return HMC_OK;   // empty batch: zero-size buffers may be NULL
  if (!st->q || !st->E_prev) return fail(HMC_EINVAL, "null state");
  if (s->rng_mode == HMC_RNG_REPLAY && (!r || !r->p || !r->L || !r->lnu))
    return fail(HMC_EINVAL, "replay mode needs p, L, lnu");
  if (s->iter_end == s->iter_begin) return HMC_OK;
  if (st->n_save > 0 && st->traj_q && st->traj_stride < s->L_high)
    return fail(HMC_EINVAL, "traj_stride must be >= L_high");
  *run = true;
  return HMC_OK;
}

hmc::RandArgs rand_args(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                        hmc_state* st, const hmc::Layout& lay) {
  hmc::RandArgs a{};
  a.n = s->n_chains;
  a.chain_offset = s->chain_offset;
  a.D = t->D;
  a.npairs = lay.npairs;
  a.lpc = lay.lpc;
  a.cpw = lay.cpw;
  a.niter = s->n_iter;
  a.wu = s->warm_up;
  a.thin = s->thin;
  a.Lc = s->L_chain;
  a.L_low = s->L_low;
  a.L_high = s->L_high;
  a.it0 = s->iter_begin;
  a.it1 = s->iter_end;
  a.ntiles = (s->n_chains + 15) / 16;
  a.i_oob = (int)(s->warm_up - (int64_t)s->L_chain * s->thin);  // rejections at i < i_oob index < -L_chain
  a.k0 = (uint32_t)s->seed;
  a.k1 = (uint32_t)(s->seed >> 32);
  a.dt = k->dt;
  a.h = k->dt * 0.5;
  a.lf_c = 2.0 - k->dt * k->dt;
  a.lf_ch = 0.5 * a.lf_c;
  a.lf_idt2 = 1.0 / (k->dt * k->dt);
  a.logc = t->logdet_const;
  a.q0 = t->q0;
  a.prec = t->prec;
  a.minv = k->minv;
  a.pscale = k->p_scale;
  a.dtv = k->dt_vec;
  a.minvf = k->minv_full;
  a.cholt = k->p_chol_t;
  a.kick = k->kick;
  if (r && s->rng_mode == HMC_RNG_REPLAY) {   // Philox draws read no replay block
    a.rp0 = r->p0;
    a.rp = r->p;
    a.rlnu = r->lnu;
    a.rL = r->L;
  }
  a.q = st->q;
  a.Eprev = st->E_prev;
  a.qc = st->q_chain;
  a.Lq = hmc::window_rows(s, st);
  a.q_row0 = (int)st->qc_row0;
  a.Ec = st->E_chain;
  a.dEc = st->dE_chain;
  a.cnt = st->counters;
  hmc::apply_env(a, lay, s->n_chains);   // debug build only (hmc_debug.hpp)
  if (hmc::captures_chain0(st)) {
    a.traj_q = st->traj_q;
    a.traj_len = st->traj_len;
    a.decision = st->decision;
    a.n_save = st->n_save;
    a.traj_stride = st->traj_stride;
  }
  return a;
}

// rand_args plus what the NUTS kernels take: the tree's depth limit, the workspace, the replay tape;
// no chain-0 capture (the reference never fills it for NUTS)
hmc::RandArgs nuts_args(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                        hmc_state* st, int D, void* workspace) {
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::Layout lay{0, 0, 16, (D + 1) / 2};   // 16 chain slots per wave
  hmc::RandArgs a = rand_args(t, k, s, r, st, lay);
  a.d_max = s->d_max;
  a.on_dmax = s->on_dmax;
  a.ws = static_cast<double*>(workspace);
  if (replay) {
    a.tape = r->tape;
    a.tape_stride = r->tape_stride;
  }
  a.traj_q = nullptr;
  a.n_save = 0;
  return a;
}

constexpr int32_t kMaxLags = 1 << 20;   // lag passes of the diagnostics (any n the samples allow)

// Host-side record of the scratch buffers' sizes (device pointer -> bytes): the sized entries
// (*_ws) record what they were given, hmc_workspace_register records a caller's buffer, and every
// entry that takes scratch refuses (HMC_EINVAL) a buffer recorded as smaller than the call needs,
// before any kernel could write past its end.  No device access: the check stays graph-capturable.
std::mutex g_ws_mu;
std::unordered_map<const void*, int64_t> g_ws_bytes;

void ws_record(const void* p, int64_t bytes) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (bytes > 0) g_ws_bytes[p] = bytes;
  else g_ws_bytes.erase(p);
}

hmc_status ws_check(const void* p, int64_t need, const char* what) {
  if (!p || need <= 0) return HMC_OK;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const auto it = g_ws_bytes.find(p);
  if (it != g_ws_bytes.end() && it->second < need)
    return fail(HMC_EINVAL, "%s: scratch buffer of %lld bytes, this call needs %lld", what, (long long)it->second,
                (long long)need);
  return HMC_OK;
}

// What the sized Random entries (*_ws) do before the plain entry runs: the schedule's checks, then
// state.order against what the call's route reads or writes of it, recorded for later calls.
hmc_status check_order_bytes(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_state* st,
                             int64_t order_bytes, bool iters, const char* what) {
  if (hmc_status e = check_schedule(t, k, s, iters)) return e;
  if (!st) return fail(HMC_EINVAL, "null state");
  const int64_t need = hmc::random_order_bytes(t, k, s, st);
  if (order_bytes < need)
    return fail(HMC_EINVAL, "%s: state.order of %lld bytes, this call needs %lld (hmc_random_workspace_size_ex)", what,
                (long long)order_bytes, (long long)need);
  if (st->order) ws_record(st->order, order_bytes);
  return HMC_OK;
}

// The NUTS depth limit's range; status: HMC_EINVAL from the MVN entries, HMC_ENOTSUP from the GLM one.
hmc_status check_d_max(const hmc_schedule* s, hmc_status status, const char* what) {
  if (s->d_max >= 1 && s->d_max <= hmc::kNutsDmaxMax) return HMC_OK;
  return fail(status, "%s: d_max=%d must be in [1, %d]", what, s->d_max, hmc::kNutsDmaxMax);
}

hmc_status view_too_large(const char* what) {
  return fail(HMC_ENOTSUP,
              "%s: one chain's samples span more than the lag kernel's 1 GiB buffer offsets; pass fewer "
              "dimensions per call (the Python layer splits such views by dimension)", what);
}

}  // namespace

extern "C" {

const char* hmc_version(void) { return "hmc_amd 0.1.0 gfx950 (diag random kernels, C ABI v1)"; }

const char* hmc_last_error(void) { return g_err.c_str(); }

hmc_status hmc_chain_init(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                          const double* q_start, hmc_state* st, void* stream) {
  if (hmc_status e = check_schedule(t, k, s, false)) return e;
  bool run;
  if (hmc_status e = check_chain_init(t, k, s, r, q_start, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::RandomRoute route = hmc::random_route(t, k, s, st, true);
  if (hmc_status e = ws_check(st->order, route.order_bytes, "hmc_chain_init: state.order")) return e;
  hmc::RandArgs a = rand_args(t, k, s, r, st, route.lay);
  a.qstart = q_start;
  if (route.kernel == hmc::RandomKernel::Big) {   // chain state in the workspace (hmc_big.hip)
    if (!st->order) return fail(HMC_EINVAL, "D=%d needs hmc_random_workspace_size() bytes in state.order", t->D);
    const bool dense = t->kind == HMC_TARGET_DENSE;
    return hip_status(hmc::launch_big_init(hmc::big_args(a, st->order, dense), dense, replay, (hipStream_t)stream),
                      "hmc_chain_init(large D)");
  }
  if (route.kernel == hmc::RandomKernel::Dense) {
    if (st->order) {   // the gradient cache no longer matches q: the next launch recomputes it
      int32_t* valid = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(st->order) +
                                                  hmc::dense_gcache_offset_bytes(s->n_chains) - 16);
      if (hmc_status e = hip_status(hipMemsetAsync(valid, 0, sizeof(int32_t), (hipStream_t)stream), "hmc_chain_init"))
        return e;
    }
    return hip_status(hmc::launch_dense_init(a, replay, (hipStream_t)stream), "hmc_chain_init(dense)");
  }
  return hip_status(hmc::launch_random_init(a, route, replay, (hipStream_t)stream), "hmc_chain_init");
}

hmc_status hmc_random_iters(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                            hmc_state* st, void* stream) {
  if (hmc_status e = check_schedule(t, k, s, true)) return e;
  bool run;
  if (hmc_status e = check_random_iters(t, k, s, r, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const bool exact = s->fp_mode == HMC_MODE_EXACT;
  const hmc::RandomRoute route = hmc::random_route(t, k, s, st, false);
  if (hmc_status e = ws_check(st->order, route.order_bytes, "hmc_random_iters: state.order")) return e;
  hmc::RandArgs a = rand_args(t, k, s, r, st, route.lay);
  if (route.kernel == hmc::RandomKernel::Big) {   // chain state in the workspace (hmc_big.hip)
    if (!st->order) return fail(HMC_EINVAL, "D=%d needs hmc_random_workspace_size() bytes in state.order", t->D);
    const bool dense = t->kind == HMC_TARGET_DENSE;
    return hip_status(hmc::launch_big_iters(hmc::big_args(a, st->order, dense), dense, exact, replay,
                                            (hipStream_t)stream),
                      "hmc_random_iters(large D)");
  }
  if (route.kernel == hmc::RandomKernel::Dense) {
    int32_t* gvalid = nullptr;
    if (st->order) {   // gradient cache in the workspace (hmc_random_workspace_size)
      char* base = reinterpret_cast<char*>(st->order);
      gvalid = reinterpret_cast<int32_t*>(base + hmc::dense_gcache_offset_bytes(s->n_chains) - 16);
      a.gcache = reinterpret_cast<double*>(base + hmc::dense_gcache_offset_bytes(s->n_chains));
      a.gvalid = gvalid;
    }
    // every launch leaves the cache holding the gradient at each chain's q
    auto mark_valid = [&]() -> hmc_status {
      return gvalid ? hip_status(hipMemsetAsync(gvalid, 1, 1, (hipStream_t)stream), "hmc_random_iters") : HMC_OK;
    };
    if (!st->order || a.traj_q || !hmc::dense_order_ok(a)) {
      if (hmc_status e = hip_status(hmc::launch_dense_iters(a, exact, replay, (hipStream_t)stream),
                                    "hmc_random_iters(dense)"))
        return e;
      return mark_valid();
    }
    // L-ordered tiles: one launch per iteration, chains counting-sorted by that iteration's L
    for (int it = s->iter_begin; it < s->iter_end; ++it) {
      if (hmc_status e = hip_status(hmc::launch_dense_order(a, it, replay, st->order, (hipStream_t)stream),
                                    "hmc_random_iters(dense order)"))
        return e;
      a.it0 = it;
      a.it1 = it + 1;
      a.order = st->order;
      if (hmc_status e = hip_status(hmc::launch_dense_iters(a, exact, replay, (hipStream_t)stream),
                                    "hmc_random_iters(dense)"))
        return e;
      if (hmc_status e = mark_valid()) return e;
    }
    return HMC_OK;
  }
  // the kernels keep per-launch tallies in 32 bits: Sum L^2 over one launch must stay < 2^31
  // (only very long trajectories, e.g. L_high = 200, with thousands of iterations split here)
  const int64_t lmax = std::max<int64_t>(std::max(s->L_high, 1), hmc::forced_L(a));
  const int64_t chunk = std::max<int64_t>(1, 0x7FFFFFFFll / (lmax * lmax));
  for (int it = s->iter_begin; it < s->iter_end;) {
    const int end = (int)std::min<int64_t>(s->iter_end, it + chunk);
    a.it0 = it;
    a.it1 = end;
    if (hmc_status e = hip_status(hmc::launch_random_iters(a, route, exact, replay, (hipStream_t)stream),
                                  "hmc_random_iters"))
      return e;
    it = end;
  }
  return HMC_OK;
}

int32_t hmc_random_leapfrog_form(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s) {
  if (!t || !k || !s || t->D < 1) return 0;
  return hmc::random_route(t, k, s, nullptr, false).three_term ? 1 : 0;   // false on the dense and large-D paths
}

hmc_status hmc_random_layout(const hmc_target* t, const hmc_schedule* s, int32_t out[4]) {
  return hmc_random_layout_ex(t, nullptr, s, out);
}

hmc_status hmc_random_layout_ex(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, int32_t out[4]) {
  if (!t || !s || !out) return fail(HMC_EINVAL, "hmc_random_layout: null target/schedule/out");
  if (t->D < 1) return fail(HMC_EINVAL, "D must be >= 1");
  if (s->L_high <= s->L_low) return fail(HMC_EINVAL, "L_low must be < L_high (randint)");
  if (t->kind == HMC_TARGET_DENSE) return fail(HMC_ENOTSUP, "hmc_random_layout: dense targets have no such layout");
  // the route of a production launch (no capture); without a kinetic descriptor the mass and the
  // three-term rule, which the four-chain kernel needs, are taken as met
  const hmc::RandomRoute route = hmc::random_route(t, k, s, nullptr, false);
  if (route.kernel == hmc::RandomKernel::Big)
    return fail(HMC_ENOTSUP, "hmc_random_layout: D=%d runs the large-D path", t->D);
  // the four-chain kernel reports 16 lanes per chain with 7 coordinates each as ceil(7 / 2) pairs per lane
  out[0] = route.lay.K;
  out[1] = route.lay.lpc;
  out[2] = route.lay.cpw;
  out[3] = route.kernel == hmc::RandomKernel::Wave ? 1 : 0;
  return HMC_OK;
}

int64_t hmc_random_workspace_size_ex(const hmc_target* t, const hmc_kinetic* k, int64_t n_chains) {
  if (!t || n_chains < 0 || t->D < 1) return 0;
  return hmc::random_workspace_bytes(t, k, n_chains);
}

int64_t hmc_random_workspace_size(const hmc_target* t, int64_t n_chains) {
  return hmc_random_workspace_size_ex(t, nullptr, n_chains);   // enough for either cov_p
}

int64_t hmc_nuts_workspace_size_ex(int32_t D, int64_t n_chains, int32_t d_max, int32_t iters_per_call,
                                   int32_t philox_momenta) {
  if (D < 1 || n_chains < 0 || d_max < 1 || d_max > hmc::kNutsDmaxMax || iters_per_call < 1) return 0;
  int64_t doubles = 0;
  switch (hmc::nuts_kernel(D)) {
    case hmc::NutsKernel::Tree:
      doubles = hmc::nuts_ws_doubles(n_chains, D, d_max, philox_momenta ? iters_per_call : 0);
      break;
    case hmc::NutsKernel::Lock:   // philox_momenta 0: replay tapes, or a full cov_p (its fragments too)
      doubles = hmc::nuts_lock_ws_doubles(n_chains, D, d_max, !philox_momenta);
      break;
    case hmc::NutsKernel::PerChain:
      doubles = hmc::nuts_big_ws_doubles(n_chains, D, d_max);
      break;
  }
  return doubles * (int64_t)sizeof(double);
}

int64_t hmc_nuts_workspace_size(int32_t D, int64_t n_chains, int32_t d_max) {
  return std::max(hmc_nuts_workspace_size_ex(D, n_chains, d_max, 32, 1),
                  hmc_nuts_workspace_size_ex(D, n_chains, d_max, 32, 0));
}

// Bytes of NUTS workspace this call needs (0: nothing to run, -1: unsupported shape).
static int64_t nuts_need(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s) {
  if (s->iter_end <= s->iter_begin || s->n_chains == 0) return 0;
  // its Philox momenta drawn ahead (diagonal cov_p) for this call's iterations, or the tree vectors
  // of the kernel this call takes
  const int32_t pm = s->rng_mode == HMC_RNG_PHILOX && !k->minv_full ? 1 : 0;
  const int64_t need = hmc_nuts_workspace_size_ex(t->D, s->n_chains, s->d_max, s->iter_end - s->iter_begin, pm);
  return need > 0 ? need : -1;
}

hmc_status hmc_workspace_register(const void* workspace, int64_t bytes) {
  if (!workspace || bytes < 0) return fail(HMC_EINVAL, "hmc_workspace_register: null pointer or negative size");
  ws_record(workspace, bytes);
  return HMC_OK;
}

hmc_status hmc_chain_init_ws(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                             const double* q_start, hmc_state* st, int64_t order_bytes, void* stream) {
  if (hmc_status e = check_order_bytes(t, k, s, st, order_bytes, false, "hmc_chain_init_ws")) return e;
  return hmc_chain_init(t, k, s, r, q_start, st, stream);
}

hmc_status hmc_random_iters_ws(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                               hmc_state* st, int64_t order_bytes, void* stream) {
  if (hmc_status e = check_order_bytes(t, k, s, st, order_bytes, true, "hmc_random_iters_ws")) return e;
  return hmc_random_iters(t, k, s, r, st, stream);
}

// hmc_nuts_iters once the schedule has passed; sized_need: nuts_need of this call where the sized
// entry has computed it already, or NULL
static hmc_status nuts_iters(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                             hmc_state* st, void* workspace, void* stream, const int64_t* sized_need) {
  if (!st) return fail(HMC_EINVAL, "null state");
  if (hmc_status e = check_window(t, s, st)) return e;
  if (hmc_status e = check_iter_range(s)) return e;
  if (s->n_chains == 0) return HMC_OK;   // empty batch: zero-size buffers may be NULL
  if (!st->q || !st->E_prev) return fail(HMC_EINVAL, "null state");
  if (hmc_status e = check_d_max(s, HMC_EINVAL, "hmc_nuts_iters")) return e;
  if (hmc_status e = check_mass(t, k, s)) return e;
  if (t->kind != HMC_TARGET_DENSE) return fail(HMC_ENOTSUP, "NUTS runs the dense kernel: pass prec as dense");
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  if (replay && (!r || !r->p || !r->tape || r->tape_stride < 1)) return fail(HMC_EINVAL, "replay mode needs p and tape");
  if (s->n_chains == 0 || s->iter_end == s->iter_begin) return HMC_OK;
  if (!workspace) return fail(HMC_EINVAL, "null workspace");
  const int64_t need = sized_need ? *sized_need : nuts_need(t, k, s);
  if (need < 0) return fail(HMC_EINVAL, "NUTS workspace: unsupported D=%d / d_max=%d", t->D, s->d_max);
  if (hmc_status e = ws_check(workspace, need, "hmc_nuts_iters: workspace")) return e;
  const hmc::RandArgs a = nuts_args(t, k, s, r, st, t->D, workspace);
  const bool exact = s->fp_mode == HMC_MODE_EXACT;
  switch (hmc::nuts_kernel(t->D)) {
    case hmc::NutsKernel::Lock:
      return hip_status(hmc::launch_nuts_lock(a, exact, replay, (hipStream_t)stream), "hmc_nuts_iters(lockstep)");
    case hmc::NutsKernel::PerChain:
      return hip_status(hmc::launch_nuts_big(a, exact, replay, (hipStream_t)stream), "hmc_nuts_iters(large D)");
    case hmc::NutsKernel::Tree:
      break;
  }
  return hip_status(hmc::launch_nuts_iters(a, exact, replay, (hipStream_t)stream), "hmc_nuts_iters");
}

hmc_status hmc_nuts_iters_ws(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                             hmc_state* st, void* workspace, int64_t workspace_bytes, void* stream) {
  if (hmc_status e = check_schedule(t, k, s, false)) return e;   // also rejects a NULL k
  if (hmc_status e = check_d_max(s, HMC_EINVAL, "hmc_nuts_iters_ws")) return e;
  const int64_t need = nuts_need(t, k, s);
  if (need < 0) return fail(HMC_EINVAL, "NUTS workspace: unsupported D=%d / d_max=%d", t->D, s->d_max);
  if (workspace_bytes < need)
    return fail(HMC_EINVAL, "NUTS workspace of %lld bytes; this call (D=%d, %lld chains, d_max=%d, %d iterations, "
                "%s momenta) needs %lld (hmc_nuts_workspace_size_ex)", (long long)workspace_bytes, t->D,
                (long long)s->n_chains, s->d_max, s->iter_end - s->iter_begin,
                s->rng_mode == HMC_RNG_PHILOX && !k->minv_full ? "Philox" : "no pre-drawn", (long long)need);
  ws_record(workspace, workspace_bytes);
  return nuts_iters(t, k, s, r, st, workspace, stream, &need);
}

hmc_status hmc_nuts_iters(const hmc_target* t, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                          hmc_state* st, void* workspace, void* stream) {
  if (hmc_status e = check_schedule(t, k, s, false)) return e;
  return nuts_iters(t, k, s, r, st, workspace, stream, nullptr);
}

hmc_status hmc_leapfrog(const hmc_target* t, const hmc_kinetic* k, int64_t n, const double* p, const double* q,
                        double* p_out, double* q_out, int32_t fp_mode, void* stream) {
  if (!t || !k || t->D < 1 || n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !p_out || !q_out)) return fail(HMC_EINVAL, "null row pointers");
  if (p_out == p || q_out == q || p_out == q || q_out == p) return fail(HMC_EINVAL, "outputs alias inputs");
  hmc::RowArgs a{};
  a.n = n;
  a.D = t->D;
  a.dense = t->kind == HMC_TARGET_DENSE;
  a.q0 = t->q0;
  a.prec = t->prec;
  if (hmc_status e = check_mass(t, k, nullptr)) return e;
  a.minv = k->minv;
  a.minvf = k->minv_full;
  a.dtv = k->dt_vec;
  a.dt = k->dt;
  a.logc = t->logdet_const;
  a.p = p;
  a.q = q;
  a.po = p_out;
  a.qo = q_out;
  return hip_status(hmc::launch_leapfrog_rows(a, fp_mode == HMC_MODE_EXACT, (hipStream_t)stream), "hmc_leapfrog");
}

hmc_status hmc_energy(const hmc_target* t, const hmc_kinetic* k, int64_t n, const double* q, const double* p,
                      double* E_out, void* stream) {
  if (!t || !k || t->D < 1 || n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !E_out)) return fail(HMC_EINVAL, "null row pointers");
  hmc::RowArgs a{};
  a.n = n;
  a.D = t->D;
  a.dense = t->kind == HMC_TARGET_DENSE;
  a.q0 = t->q0;
  a.prec = t->prec;
  if (hmc_status e = check_mass(t, k, nullptr)) return e;
  a.minv = k->minv;
  a.minvf = k->minv_full;
  a.logc = t->logdet_const;
  a.p = p;
  a.q = q;
  a.E = E_out;
  return hip_status(hmc::launch_energy_rows(a, (hipStream_t)stream), "hmc_energy");
}

// ---------------------------------------------------------------- Gaussian-mixture target
namespace {

hmc_status check_mixture(const hmc_mixture* m, const hmc_kinetic* k, const char* what) {
  if (!m || !k) return fail(HMC_EINVAL, "%s: null mixture/kinetic", what);
  if (m->D < 1) return fail(HMC_EINVAL, "%s: D must be >= 1", what);
  if (m->K < 1) return fail(HMC_EINVAL, "%s: K must be >= 1", what);
  if (!m->logw || !m->mu || !m->prec || !m->logdet_const)
    return fail(HMC_EINVAL, "%s: mixture needs logw, mu, prec and logdet_const", what);
  if (m->D > HMC_MIX_MAX_D) return fail(HMC_ENOTSUP, "%s: D=%d, the mixture kernels take D <= %d", what, m->D, HMC_MIX_MAX_D);
  if (m->K > HMC_MIX_MAX_COMPONENTS)
    return fail(HMC_ENOTSUP, "%s: K=%d, the mixture kernels take K <= %d", what, m->K, HMC_MIX_MAX_COMPONENTS);
  if (k->minv_full || k->p_chol_t || k->kick)
    return fail(HMC_ENOTSUP, "%s: a full cov_p is not supported for mixture targets (diagonal minv/p_scale only)", what);
  return HMC_OK;
}

hmc_target mix_shape(const hmc_mixture* m) { return hmc_target{m->D, HMC_TARGET_DIAG, nullptr, nullptr, 0.0}; }

hmc::MixArgs mix_args(const hmc_mixture* m, const hmc::RandArgs& a) {
  hmc::MixArgs x{};
  x.a = a;
  x.Kc = m->K;
  x.logw = m->logw;
  x.mu = m->mu;
  x.prec = m->prec;
  x.ldc = m->logdet_const;
  return x;
}

// Row-wise entries: the rows take the chains' place in the lane-group layout.
hmc::MixArgs mix_row_args(const hmc_mixture* m, const hmc_kinetic* k, int64_t n, const hmc::Layout& lay) {
  hmc::RandArgs a{};
  a.n = n;
  a.D = m->D;
  a.npairs = lay.npairs;
  a.lpc = lay.lpc;
  a.cpw = lay.cpw;
  a.dt = k->dt;
  a.h = k->dt * 0.5;
  a.minv = k->minv;
  a.dtv = k->dt_vec;
  return mix_args(m, a);
}

}  // namespace

hmc_status hmc_mix_chain_init(const hmc_mixture* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                              const double* q_start, hmc_state* st, void* stream) {
  if (hmc_status e = check_mixture(m, k, "hmc_mix_chain_init")) return e;
  const hmc_target t = mix_shape(m);
  if (hmc_status e = check_schedule(&t, k, s, false)) return e;
  bool run;
  if (hmc_status e = check_chain_init(&t, k, s, r, q_start, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::TrajRange L = hmc::init_traj_range(s);
  const hmc::Layout lay = hmc::mix_layout(m->D, L.lo, L.hi);
  if (lay.K == 0) return fail(HMC_ENOTSUP, "D=%d too large for the mixture kernels", m->D);
  hmc::RandArgs a = rand_args(&t, k, s, r, st, lay);
  a.qstart = q_start;
  return hip_status(hmc::launch_mix_init(mix_args(m, a), lay, replay, (hipStream_t)stream), "hmc_mix_chain_init");
}

hmc_status hmc_mix_random_iters(const hmc_mixture* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                                hmc_state* st, void* stream) {
  if (hmc_status e = check_mixture(m, k, "hmc_mix_random_iters")) return e;
  const hmc_target t = mix_shape(m);
  if (hmc_status e = check_schedule(&t, k, s, true)) return e;
  bool run;
  if (hmc_status e = check_random_iters(&t, k, s, r, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::Layout lay = hmc::mix_layout(m->D, s->L_low, s->L_high);
  if (lay.K == 0) return fail(HMC_ENOTSUP, "D=%d too large for the mixture kernels", m->D);
  const hmc::RandArgs a = rand_args(&t, k, s, r, st, lay);
  return hip_status(hmc::launch_mix_iters(mix_args(m, a), lay, replay, (hipStream_t)stream), "hmc_mix_random_iters");
}

hmc_status hmc_mix_leapfrog(const hmc_mixture* m, const hmc_kinetic* k, int64_t n, const double* p, const double* q,
                            double* p_out, double* q_out, void* stream) {
  if (hmc_status e = check_mixture(m, k, "hmc_mix_leapfrog")) return e;
  if (n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !p_out || !q_out)) return fail(HMC_EINVAL, "null row pointers");
  if (p_out == p || q_out == q || p_out == q || q_out == p) return fail(HMC_EINVAL, "outputs alias inputs");
  if (!std::isfinite(k->dt) && !k->dt_vec) return fail(HMC_EINVAL, "dt must be set (samplers.py:332)");
  const hmc::Layout lay = hmc::mix_layout(m->D, 5, 20);
  hmc::MixArgs x = mix_row_args(m, k, n, lay);
  x.row_p = p;
  x.row_q = q;
  x.row_po = p_out;
  x.row_qo = q_out;
  return hip_status(hmc::launch_mix_rows(x, lay, true, (hipStream_t)stream), "hmc_mix_leapfrog");
}

hmc_status hmc_mix_energy(const hmc_mixture* m, const hmc_kinetic* k, int64_t n, const double* q, const double* p,
                          double* E_out, void* stream) {
  if (hmc_status e = check_mixture(m, k, "hmc_mix_energy")) return e;
  if (n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !E_out)) return fail(HMC_EINVAL, "null row pointers");
  const hmc::Layout lay = hmc::mix_layout(m->D, 5, 20);
  hmc::MixArgs x = mix_row_args(m, k, n, lay);
  x.row_p = p;
  x.row_q = q;
  x.row_E = E_out;
  return hip_status(hmc::launch_mix_rows(x, lay, false, (hipStream_t)stream), "hmc_mix_energy");
}

// ---------------------------------------------------------------- logistic-regression target
namespace {

hmc_status check_logistic(const hmc_logistic* m, const hmc_kinetic* k, const char* what) {
  if (!m || !k) return fail(HMC_EINVAL, "%s: null logistic/kinetic", what);
  if (m->D < 1) return fail(HMC_EINVAL, "%s: D must be >= 1", what);
  if (m->n < 1) return fail(HMC_EINVAL, "%s: n must be >= 1", what);
  if (!m->X || !m->y || !m->prior_prec) return fail(HMC_EINVAL, "%s: logistic target needs X, y and prior_prec", what);
  if (m->ldx < m->D) return fail(HMC_EINVAL, "%s: ldx=%lld < D=%d", what, (long long)m->ldx, m->D);
  if (m->D > HMC_LOGIT_MAX_D)
    return fail(HMC_ENOTSUP, "%s: D=%d, the logistic kernels take D <= %d", what, m->D, HMC_LOGIT_MAX_D);
  if (m->n > HMC_LOGIT_MAX_N)
    return fail(HMC_ENOTSUP, "%s: n=%d, the logistic kernels take n <= %d", what, m->n, HMC_LOGIT_MAX_N);
  if (k->minv_full || k->p_chol_t || k->kick)
    return fail(HMC_ENOTSUP, "%s: a full cov_p is not supported for logistic targets (diagonal minv/p_scale only)", what);
  return HMC_OK;
}

hmc_target logit_shape(const hmc_logistic* m) { return hmc_target{m->D, HMC_TARGET_DIAG, nullptr, nullptr, 0.0}; }

hmc::LogitArgs logit_args(const hmc_logistic* m, const hmc::RandArgs& a) {
  hmc::LogitArgs x{};
  x.a = a;
  x.nrows = m->n;
  x.ldx = m->ldx;
  x.X = m->X;
  x.y = m->y;
  x.pprec = m->prior_prec;
  return x;
}

// Row-wise entries: the rows take the chains' place in the 16-column tiles.
hmc::LogitArgs logit_row_args(const hmc_logistic* m, const hmc_kinetic* k, int64_t n) {
  hmc::RandArgs a{};
  a.n = n;
  a.D = m->D;
  a.dt = k->dt;
  a.h = k->dt * 0.5;
  a.minv = k->minv;
  a.dtv = k->dt_vec;
  return logit_args(m, a);
}

}  // namespace

// The four entries for either family: hmc_logit_* pass HMC_GLM_BERNOULLI, hmc_glm_* their own.
namespace {

hmc_status glm_chain_init(const hmc_logistic* m, int family, const hmc_kinetic* k, const hmc_schedule* s,
                          const hmc_replay* r, const double* q_start, hmc_state* st, void* stream, const char* what) {
  if (hmc_status e = check_logistic(m, k, what)) return e;
  const hmc_target t = logit_shape(m);
  if (hmc_status e = check_schedule(&t, k, s, false)) return e;
  bool run;
  if (hmc_status e = check_chain_init(&t, k, s, r, q_start, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::Layout lay = hmc::flat_layout(m->D);
  hmc::RandArgs a = rand_args(&t, k, s, r, st, lay);
  a.qstart = q_start;
  return hip_status(hmc::launch_logit_init(logit_args(m, a), family, replay, (hipStream_t)stream), what);
}

// The _adapt entries' own argument: HMC_EINVAL for a null block or state, a delta outside (0, 1),
// a non-positive (or NaN) gamma, t0 or kappa.
hmc_status check_adapt(const hmc_adapt* ad, const char* what) {
  if (!ad || !ad->state) return fail(HMC_EINVAL, "%s: null adapt block / state", what);
  if (!(ad->delta > 0.0 && ad->delta < 1.0))
    return fail(HMC_EINVAL, "%s: delta=%g, the target acceptance statistic lies in (0, 1)", what, ad->delta);
  if (!(ad->gamma > 0.0) || !(ad->t0 > 0.0) || !(ad->kappa > 0.0))
    return fail(HMC_EINVAL, "%s: gamma=%g, t0=%g, kappa=%g must be positive", what, ad->gamma, ad->t0, ad->kappa);
  return HMC_OK;
}

// ad: NULL for the plain entry; the _adapt entry has checked it (check_adapt)
hmc_status glm_random_iters(const hmc_logistic* m, int family, const hmc_kinetic* k, const hmc_schedule* s,
                            const hmc_replay* r, hmc_state* st, void* stream, const char* what,
                            const hmc_adapt* ad = nullptr) {
  if (hmc_status e = check_logistic(m, k, what)) return e;
  const hmc_target t = logit_shape(m);
  if (hmc_status e = check_schedule(&t, k, s, true)) return e;
  bool run;
  if (hmc_status e = check_random_iters(&t, k, s, r, st, &run); e != HMC_OK || !run) return e;
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  const hmc::Layout lay = hmc::flat_layout(m->D);
  const hmc::RandArgs a = rand_args(&t, k, s, r, st, lay);
  return hip_status(hmc::launch_logit_iters(logit_args(m, a), family, replay, (hipStream_t)stream, ad), what);
}

hmc_status glm_leapfrog(const hmc_logistic* m, int family, const hmc_kinetic* k, int64_t n, const double* p,
                        const double* q, double* p_out, double* q_out, void* stream, const char* what) {
  if (hmc_status e = check_logistic(m, k, what)) return e;
  if (n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !p_out || !q_out)) return fail(HMC_EINVAL, "null row pointers");
  if (p_out == p || q_out == q || p_out == q || q_out == p) return fail(HMC_EINVAL, "outputs alias inputs");
  if (!std::isfinite(k->dt) && !k->dt_vec) return fail(HMC_EINVAL, "dt must be set (samplers.py:332)");
  hmc::LogitArgs x = logit_row_args(m, k, n);
  x.row_p = p;
  x.row_q = q;
  x.row_po = p_out;
  x.row_qo = q_out;
  return hip_status(hmc::launch_logit_rows(x, family, true, (hipStream_t)stream), what);
}

hmc_status glm_energy(const hmc_logistic* m, int family, const hmc_kinetic* k, int64_t n, const double* q,
                      const double* p, double* E_out, void* stream, const char* what) {
  if (hmc_status e = check_logistic(m, k, what)) return e;
  if (n < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n > 0 && (!p || !q || !E_out)) return fail(HMC_EINVAL, "null row pointers");
  hmc::LogitArgs x = logit_row_args(m, k, n);
  x.row_q = q;
  x.row_p = p;
  x.row_E = E_out;
  return hip_status(hmc::launch_logit_rows(x, family, false, (hipStream_t)stream), what);
}

hmc_status check_family(int family, const char* what) {
  if (family == HMC_GLM_BERNOULLI || family == HMC_GLM_POISSON) return HMC_OK;
  return fail(HMC_EINVAL, "%s: unknown family %d (HMC_GLM_BERNOULLI, HMC_GLM_POISSON)", what, family);
}

// hmc_glm -> the data descriptor the kernels take; HMC_EINVAL for a null descriptor or an unknown family
hmc_status glm_data(const hmc_glm* m, const char* what, hmc_logistic* out) {
  if (!m) return fail(HMC_EINVAL, "%s: null glm target", what);
  if (hmc_status e = check_family(m->family, what)) return e;
  *out = hmc_logistic{m->D, m->n, m->ldx, m->X, m->y, m->prior_prec};
  return HMC_OK;
}

// A sample view's strides and row range (hmc_samples), and its row and sample counts.
hmc_status check_view_rows(const hmc_samples* s, int32_t D, const char* what) {
  if (s->row_stride < D) return fail(HMC_EINVAL, "%s: row_stride=%lld < D=%d", what, (long long)s->row_stride, D);
  if (s->row_step < 1) return fail(HMC_EINVAL, "%s: row_step=%lld must be >= 1", what, (long long)s->row_step);
  if (s->row_begin < 0 || s->row_end < s->row_begin || s->n_chains < 0)
    return fail(HMC_EINVAL, "%s: rows [%lld, %lld) of %lld chains", what, (long long)s->row_begin,
                (long long)s->row_end, (long long)s->n_chains);
  return HMC_OK;
}

hmc_status view_counts(const hmc_samples* s, const char* what, int64_t* rows, int64_t* n_samples) {
  *rows = (s->row_end - s->row_begin + s->row_step - 1) / s->row_step;
  if (*rows > 0 && s->n_chains > INT64_MAX / *rows) return fail(HMC_EINVAL, "%s: chains x rows overflows", what);
  *n_samples = s->n_chains * *rows;
  return HMC_OK;
}

}  // namespace

hmc_status hmc_logit_chain_init(const hmc_logistic* m, const hmc_kinetic* k, const hmc_schedule* s,
                                const hmc_replay* r, const double* q_start, hmc_state* st, void* stream) {
  return glm_chain_init(m, HMC_GLM_BERNOULLI, k, s, r, q_start, st, stream, "hmc_logit_chain_init");
}

hmc_status hmc_logit_random_iters(const hmc_logistic* m, const hmc_kinetic* k, const hmc_schedule* s,
                                  const hmc_replay* r, hmc_state* st, void* stream) {
  return glm_random_iters(m, HMC_GLM_BERNOULLI, k, s, r, st, stream, "hmc_logit_random_iters");
}

hmc_status hmc_logit_leapfrog(const hmc_logistic* m, const hmc_kinetic* k, int64_t n, const double* p, const double* q,
                              double* p_out, double* q_out, void* stream) {
  return glm_leapfrog(m, HMC_GLM_BERNOULLI, k, n, p, q, p_out, q_out, stream, "hmc_logit_leapfrog");
}

hmc_status hmc_logit_energy(const hmc_logistic* m, const hmc_kinetic* k, int64_t n, const double* q, const double* p,
                            double* E_out, void* stream) {
  return glm_energy(m, HMC_GLM_BERNOULLI, k, n, q, p, E_out, stream, "hmc_logit_energy");
}

// ---------------------------------------------------------------- generalized-linear-model targets
hmc_status hmc_glm_chain_init(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                              const double* q_start, hmc_state* st, void* stream) {
  hmc_logistic d;
  if (hmc_status e = glm_data(m, "hmc_glm_chain_init", &d)) return e;
  return glm_chain_init(&d, m->family, k, s, r, q_start, st, stream, "hmc_glm_chain_init");
}

hmc_status hmc_glm_random_iters(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                                hmc_state* st, void* stream) {
  hmc_logistic d;
  if (hmc_status e = glm_data(m, "hmc_glm_random_iters", &d)) return e;
  return glm_random_iters(&d, m->family, k, s, r, st, stream, "hmc_glm_random_iters");
}

hmc_status hmc_glm_leapfrog(const hmc_glm* m, const hmc_kinetic* k, int64_t n, const double* p, const double* q,
                            double* p_out, double* q_out, void* stream) {
  hmc_logistic d;
  if (hmc_status e = glm_data(m, "hmc_glm_leapfrog", &d)) return e;
  return glm_leapfrog(&d, m->family, k, n, p, q, p_out, q_out, stream, "hmc_glm_leapfrog");
}

hmc_status hmc_glm_energy(const hmc_glm* m, const hmc_kinetic* k, int64_t n, const double* q, const double* p,
                          double* E_out, void* stream) {
  hmc_logistic d;
  if (hmc_status e = glm_data(m, "hmc_glm_energy", &d)) return e;
  return glm_energy(&d, m->family, k, n, q, p, E_out, stream, "hmc_glm_energy");
}

int64_t hmc_glm_nuts_workspace_size(int32_t D, int64_t n_chains, int32_t d_max) {
  return hmc::glm_nuts_ws_doubles(n_chains, D, d_max) * (int64_t)sizeof(double);
}

namespace {

// ad: NULL for the plain entry; the _adapt entry has checked it (check_adapt)
hmc_status glm_nuts_iters(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                          hmc_state* st, void* workspace, int64_t workspace_bytes, void* stream, const char* what,
                          const hmc_adapt* ad) {
  hmc_logistic d;
  if (hmc_status e = glm_data(m, what, &d)) return e;
  if (hmc_status e = check_logistic(&d, k, what)) return e;
  const hmc_target t = logit_shape(&d);
  if (hmc_status e = check_schedule(&t, k, s, false)) return e;
  if (!st) return fail(HMC_EINVAL, "null state");
  if (hmc_status e = check_window(&t, s, st)) return e;
  if (hmc_status e = check_iter_range(s)) return e;
  if (hmc_status e = check_d_max(s, HMC_ENOTSUP, what)) return e;
  if (s->n_chains == 0) return HMC_OK;   // empty batch: zero-size buffers may be NULL
  if (!st->q || !st->E_prev) return fail(HMC_EINVAL, "null state");
  const bool replay = s->rng_mode == HMC_RNG_REPLAY;
  if (replay && (!r || !r->p || !r->tape || r->tape_stride < 1)) return fail(HMC_EINVAL, "replay mode needs p and tape");
  if (!workspace) return fail(HMC_EINVAL, "%s: null workspace", what);
  const int64_t need = hmc_glm_nuts_workspace_size(d.D, s->n_chains, s->d_max);
  if (workspace_bytes < need)
    return fail(HMC_EINVAL, "%s: workspace of %lld bytes, D=%d, %lld chains, d_max=%d need %lld "
                "(hmc_glm_nuts_workspace_size)", what, (long long)workspace_bytes, d.D, (long long)s->n_chains,
                s->d_max, (long long)need);
  if (s->iter_end == s->iter_begin) return HMC_OK;
  const hmc::RandArgs a = nuts_args(&t, k, s, r, st, d.D, workspace);
  return hip_status(hmc::launch_glm_nuts(logit_args(&d, a), m->family, replay, (hipStream_t)stream, ad), what);
}

}  // namespace

hmc_status hmc_glm_nuts_iters(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s, const hmc_replay* r,
                              hmc_state* st, void* workspace, int64_t workspace_bytes, void* stream) {
  return glm_nuts_iters(m, k, s, r, st, workspace, workspace_bytes, stream, "hmc_glm_nuts_iters", nullptr);
}

// ---------------------------------------------------------------- step-size adaptation (GLM)
hmc_status hmc_adapt_init(double* state, int64_t n_chains, const double* s0, void* stream) {
  if (n_chains < 0 || (n_chains > 0 && !state)) return fail(HMC_EINVAL, "hmc_adapt_init: null state / n_chains < 0");
  return hip_status(hmc::launch_adapt_init(state, n_chains, s0, (hipStream_t)stream), "hmc_adapt_init");
}

hmc_status hmc_glm_random_iters_adapt(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s,
                                      const hmc_replay* r, hmc_state* st, const hmc_adapt* ad, void* stream) {
  const char* what = "hmc_glm_random_iters_adapt";
  if (hmc_status e = check_adapt(ad, what)) return e;
  hmc_logistic d;
  if (hmc_status e = glm_data(m, what, &d)) return e;
  return glm_random_iters(&d, m->family, k, s, r, st, stream, what, ad);
}

hmc_status hmc_glm_nuts_iters_adapt(const hmc_glm* m, const hmc_kinetic* k, const hmc_schedule* s,
                                    const hmc_replay* r, hmc_state* st, void* workspace, int64_t workspace_bytes,
                                    const hmc_adapt* ad, void* stream) {
  const char* what = "hmc_glm_nuts_iters_adapt";
  if (hmc_status e = check_adapt(ad, what)) return e;
  return glm_nuts_iters(m, k, s, r, st, workspace, workspace_bytes, stream, what, ad);
}

// ---------------------------------------------------------------- posterior predictive (GLM)
int32_t hmc_glm_predictive_blocks(int32_t D, int64_t n_eval, int64_t n_samples) {
  return (int32_t)hmc::pred_sample_blocks(D, n_eval, n_samples);
}

int64_t hmc_glm_predictive_workspace_size(int32_t D, int64_t n_eval, int64_t n_samples) {
  return hmc::pred_sample_blocks(D, n_eval, n_samples) * n_eval * HMC_PRED_STRIDE * (int64_t)sizeof(double);
}

hmc_status hmc_glm_predictive(const hmc_glm* eval, const hmc_samples* s, double* out, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  const char* what = "hmc_glm_predictive";
  if (!eval || !s) return fail(HMC_EINVAL, "%s: null evaluation set / sample set", what);
  if (!eval->X || !s->q || !out) return fail(HMC_EINVAL, "%s: null X, q or out", what);
  if (hmc_status e = check_family(eval->family, what)) return e;
  if (eval->D < 1 || eval->n < 0) return fail(HMC_EINVAL, "%s: D must be >= 1 and n >= 0", what);
  if (eval->ldx < eval->D) return fail(HMC_EINVAL, "%s: ldx=%lld < D=%d", what, (long long)eval->ldx, eval->D);
  if (hmc_status e = check_view_rows(s, eval->D, what)) return e;
  if (eval->D > HMC_LOGIT_MAX_D)
    return fail(HMC_ENOTSUP, "%s: D=%d, the kernel takes D <= %d", what, eval->D, HMC_LOGIT_MAX_D);
  if (eval->n > HMC_LOGIT_MAX_N)
    return fail(HMC_ENOTSUP, "%s: n=%d, the kernel takes n <= %d", what, eval->n, HMC_LOGIT_MAX_N);
  int64_t rows = 0, n_samples = 0;
  if (hmc_status e = view_counts(s, what, &rows, &n_samples)) return e;
  if (eval->n == 0 || n_samples == 0) return HMC_OK;   // nothing to reduce: out stays as it is
  const int64_t need = hmc_glm_predictive_workspace_size(eval->D, eval->n, n_samples);
  if (!workspace) return fail(HMC_EINVAL, "%s: null workspace", what);
  if (workspace_bytes < need)
    return fail(HMC_EINVAL, "%s: workspace of %lld bytes, D=%d, %d rows, %lld samples need %lld "
                "(hmc_glm_predictive_workspace_size)", what, (long long)workspace_bytes, eval->D, eval->n,
                (long long)n_samples, (long long)need);
  return hip_status(hmc::launch_pred(*eval, *s, rows, n_samples, out, (double*)workspace, (hipStream_t)stream), what);
}

// ---------------------------------------------------------------- order statistics (radix select)
namespace {

// The view's own checks; *rows and *n_samples on success.
hmc_status select_view(const hmc_samples* s, int32_t D, const char* what, int64_t* rows, int64_t* n_samples) {
  if (!s) return fail(HMC_EINVAL, "%s: null sample set", what);
  if (D < 1) return fail(HMC_EINVAL, "%s: D must be >= 1", what);
  if (hmc_status e = check_view_rows(s, D, what)) return e;
  if (hmc_status e = view_counts(s, what, rows, n_samples)) return e;
  if (*n_samples > 0 && !s->q) return fail(HMC_EINVAL, "%s: null q", what);   // an empty view has no storage
  return HMC_OK;
}

hmc_status select_shape(int32_t D, int32_t T, const char* what) {
  if (D < 1) return fail(HMC_EINVAL, "%s: D must be >= 1", what);
  if (T < 1 || T > HMC_SELECT_MAX_RANKS)
    return fail(HMC_EINVAL, "%s: T=%d ranks, a call takes 1 .. %d", what, T, HMC_SELECT_MAX_RANKS);
  if (hmc::select_tiles(D) > hmc::kSelMaxTiles)
    return fail(HMC_ENOTSUP, "%s: D=%d, the kernel takes D <= %lld", what, D,
                (long long)(hmc::kSelMaxTiles * hmc::kSelTile));
  return HMC_OK;
}

hmc_status select_pass(int32_t pass, const char* what) {
  if (pass < 0 || pass >= hmc::kSelPasses)
    return fail(HMC_EINVAL, "%s: pass=%d outside 0 .. %d", what, pass, hmc::kSelPasses - 1);
  return HMC_OK;
}

hmc_status select_ranks(const int64_t* ranks, int32_t T, int64_t n_samples, const char* what, hmc::SelectRanks* out) {
  if (!ranks) return fail(HMC_EINVAL, "%s: null ranks", what);
  for (int t = 0; t < HMC_SELECT_MAX_RANKS; ++t) out->r[t] = 0;
  for (int t = 0; t < T; ++t) {
    if (ranks[t] < 0 || ranks[t] >= n_samples)
      return fail(HMC_EINVAL, "%s: rank %lld outside [0, %lld)", what, (long long)ranks[t], (long long)n_samples);
    out->r[t] = ranks[t];
  }
  return HMC_OK;
}

}  // namespace

int64_t hmc_select_workspace_size(int32_t D, int32_t T) {
  if (D < 1 || T < 1 || T > HMC_SELECT_MAX_RANKS) return 0;
  return (hmc::select_state_words(D, T) + hmc::select_count_words(D, T)) * (int64_t)sizeof(int64_t);
}

int64_t hmc_select_grid(int32_t D, int64_t n_samples) { return hmc::select_blocks(D, n_samples); }

hmc_status hmc_select_init(int64_t* state, int32_t D, int32_t T, const int64_t* ranks, int64_t n_samples,
                           void* stream) {
  const char* what = "hmc_select_init";
  if (hmc_status e = select_shape(D, T, what)) return e;
  if (n_samples < 0) return fail(HMC_EINVAL, "%s: n_samples < 0", what);
  if (n_samples == 0) return HMC_OK;
  hmc::SelectRanks r;
  if (hmc_status e = select_ranks(ranks, T, n_samples, what, &r)) return e;
  if (!state) return fail(HMC_EINVAL, "%s: null state", what);
  return hip_status(hmc::launch_select_init(state, D, T, r, (hipStream_t)stream), what);
}

hmc_status hmc_select_count(const hmc_samples* s, int32_t D, int32_t T, int32_t pass, const int64_t* state,
                            int64_t* counts, void* stream) {
  const char* what = "hmc_select_count";
  if (hmc_status e = select_shape(D, T, what)) return e;
  if (hmc_status e = select_pass(pass, what)) return e;
  int64_t rows = 0, n_samples = 0;
  if (hmc_status e = select_view(s, D, what, &rows, &n_samples)) return e;
  if (!state || !counts) return fail(HMC_EINVAL, "%s: null state or counts", what);
  if (n_samples > 0 && hmc::select_blocks(D, n_samples) == 0)
    return fail(HMC_ENOTSUP, "%s: D=%d with %lld samples is past the launch's limits (2^48 samples, 2^31 blocks)",
                what, D, (long long)n_samples);
  // an empty shard still contributes a table of zeros to the sum over shards
  if (n_samples == 0) return hip_status(hmc::zero_select_counts(counts, D, T, (hipStream_t)stream), what);
  return hip_status(hmc::launch_select_count(*s, rows, n_samples, D, T, pass, state, counts, (hipStream_t)stream),
                    what);
}

hmc_status hmc_select_pick(int32_t D, int32_t T, int32_t pass, int64_t* state, const int64_t* counts, void* stream) {
  const char* what = "hmc_select_pick";
  if (hmc_status e = select_shape(D, T, what)) return e;
  if (hmc_status e = select_pass(pass, what)) return e;
  if (!state || !counts) return fail(HMC_EINVAL, "%s: null state or counts", what);
  return hip_status(hmc::launch_select_pick(D, T, state, counts, (hipStream_t)stream), what);
}

hmc_status hmc_select_values(int32_t D, int32_t T, const int64_t* state, double* out, void* stream) {
  const char* what = "hmc_select_values";
  if (hmc_status e = select_shape(D, T, what)) return e;
  if (!state || !out) return fail(HMC_EINVAL, "%s: null state or out", what);
  return hip_status(hmc::launch_select_values(D, T, state, out, (hipStream_t)stream), what);
}

hmc_status hmc_order_stats(const hmc_samples* s, int32_t D, int32_t T, const int64_t* ranks, double* out,
                           void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "hmc_order_stats";
  if (hmc_status e = select_shape(D, T, what)) return e;
  int64_t rows = 0, n_samples = 0;
  if (hmc_status e = select_view(s, D, what, &rows, &n_samples)) return e;
  if (!ranks) return fail(HMC_EINVAL, "%s: null ranks", what);
  if (n_samples == 0) return HMC_OK;                     // no order statistic exists: out stays as it is
  if (n_samples > 0 && hmc::select_blocks(D, n_samples) == 0)
    return fail(HMC_ENOTSUP, "%s: D=%d with %lld samples is past the launch's limits (2^48 samples, 2^31 blocks)",
                what, D, (long long)n_samples);
  hmc::SelectRanks r;
  if (hmc_status e = select_ranks(ranks, T, n_samples, what, &r)) return e;
  if (!out) return fail(HMC_EINVAL, "%s: null out", what);
  const int64_t need = hmc_select_workspace_size(D, T);
  if (!workspace) return fail(HMC_EINVAL, "%s: null workspace", what);
  if (workspace_bytes < need)
    return fail(HMC_EINVAL, "%s: workspace of %lld bytes, D=%d with %d ranks needs %lld (hmc_select_workspace_size)",
                what, (long long)workspace_bytes, D, T, (long long)need);
  int64_t* state = (int64_t*)workspace;
  int64_t* counts = state + hmc::select_state_words(D, T);
  hipStream_t st = (hipStream_t)stream;
  if (hmc_status e = hip_status(hmc::launch_select_init(state, D, T, r, st), what)) return e;
  for (int pass = 0; pass < hmc::kSelPasses; ++pass) {
    if (hmc_status e = hip_status(hmc::launch_select_count(*s, rows, n_samples, D, T, pass, state, counts, st), what))
      return e;
    if (hmc_status e = hip_status(hmc::launch_select_pick(D, T, state, counts, st), what)) return e;
  }
  return hip_status(hmc::launch_select_values(D, T, state, out, st), what);
}

hmc_status hmc_rng_normals(uint64_t seed, int64_t chain0, int64_t n, int32_t iteration, int32_t npairs, double* out,
                           void* stream) {
  if (n < 0 || npairs < 0 || iteration < 0) return fail(HMC_EINVAL, "bad arguments");
  if (n * npairs > 0 && !out) return fail(HMC_EINVAL, "null out");
  return hip_status(hmc::launch_rng_normals((uint32_t)seed, (uint32_t)(seed >> 32), chain0, n, iteration, npairs,
                                            out, (hipStream_t)stream),
                    "hmc_rng_normals");
}

hmc_status hmc_philox(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t k0, uint32_t k1, int64_t n,
                      uint32_t* out, void* stream) {
  if (n < 0 || (n > 0 && !out)) return fail(HMC_EINVAL, "bad arguments");
  return hip_status(hmc::launch_philox(make_uint4(x0, x1, x2, x3), k0, k1, n, out, (hipStream_t)stream),
                    "hmc_philox");
}

int64_t hmc_rowsum_work_size(int64_t rows, int32_t D) { return hmc::diag_rowsum_work(rows, D); }

int64_t hmc_variogram_work_size(int64_t n_chains, int32_t D, int32_t nlags) {
  return hmc::diag_variogram_work(n_chains, D, nlags);
}

hmc_status hmc_split_moments(const double* x, int64_t n_chains, int64_t chain_stride, int64_t sample_stride,
                             int64_t base, int32_t n, int32_t D, double* mean_out, double* std_out, void* stream) {
  if (!x || !mean_out || !std_out || n_chains < 1 || n < 1 || D < 1) return fail(HMC_EINVAL, "bad arguments");
  return hip_status(hmc::launch_split_moments(x, n_chains, chain_stride, sample_stride, base, n, D, mean_out,
                                              std_out, (hipStream_t)stream),
                    "hmc_split_moments");
}

hmc_status hmc_rowsum(const double* x, int64_t n_outer, int64_t outer_stride, int64_t n_inner, int64_t inner_stride,
                      int64_t base, int32_t D, const double* center, double* work, double* out, void* stream) {
  if (!x || !work || !out || n_outer < 1 || n_inner < 1 || D < 1) return fail(HMC_EINVAL, "bad arguments");
  return hip_status(hmc::launch_rowsum(x, n_outer, outer_stride, n_inner, inner_stride, base, D, center, work, out,
                                       (hipStream_t)stream),
                    "hmc_rowsum");
}

hmc_status hmc_variogram(const double* x, int64_t n_chains, int64_t chain_stride, int64_t sample_stride,
                         int64_t base, int32_t n, int32_t D, int32_t t0, int32_t t1, double* work, double* out,
                         void* stream) {
  if (!x || !work || !out || n_chains < 1 || n < 1 || D < 1 || t0 < 1 || t1 <= t0 || t1 - t0 > kMaxLags)
    return fail(HMC_EINVAL, "bad arguments (1 <= t0 < t1, t1 - t0 <= %d)", kMaxLags);
  if (!hmc::diag_view_ok(n_chains, chain_stride, sample_stride, n, D, 2, 0, 0)) return view_too_large("hmc_variogram");
  return hip_status(hmc::launch_variogram(x, n_chains, chain_stride, sample_stride, base, n, D, t0, t1, work, out,
                                          (hipStream_t)stream),
                    "hmc_variogram (the view must keep one chain's samples within 1 GiB, include/hmc.h)");
}

static bool conv_tmax_ok(int32_t t) { return t >= 1 && t <= kMaxLags; }

int64_t hmc_convergence_work_size(int64_t n_chains, int32_t D, int32_t tmax) {
  if (n_chains < 1 || D < 1 || !conv_tmax_ok(tmax)) return 0;
  return hmc::diag_conv_work(n_chains, D, tmax);
}

hmc_status hmc_convergence_sums(const double* x, int64_t n_chains, int64_t chain_stride, int64_t sample_stride,
                                int64_t base, int32_t n, int32_t D, int32_t tmax, double* work, double* out,
                                void* stream) {
  if (!x || !work || !out || n_chains < 1 || n < 2 || D < 1) return fail(HMC_EINVAL, "bad arguments");
  if (!conv_tmax_ok(tmax)) return fail(HMC_EINVAL, "tmax must be in 1 .. %d", kMaxLags);
  if (!hmc::diag_view_ok(n_chains, chain_stride, sample_stride, n, D, 2, 0, 0))
    return view_too_large("hmc_convergence_sums");
  return hip_status(hmc::launch_conv_fused(x, n_chains, chain_stride, sample_stride, base, n, D, tmax, work, out,
                                           (hipStream_t)stream),
                    "hmc_convergence_sums");
}

hmc_status hmc_half_sums(const double* window, int64_t n_chains, int64_t chain_stride, int64_t sample_stride,
                         int32_t D, int32_t wrap, int32_t slot0, int32_t n, int32_t tmax, double* work, double* out,
                         void* stream) {
  if (!window || !work || !out || n_chains < 1 || n < 2 || D < 1 || slot0 < 0 || wrap < 0 ||
      (wrap > 0 && (slot0 >= wrap || n > wrap)))
    return fail(HMC_EINVAL, "bad arguments");
  if (!conv_tmax_ok(tmax)) return fail(HMC_EINVAL, "tmax must be in 1 .. %d", kMaxLags);
  if (!hmc::diag_view_ok(n_chains, chain_stride, sample_stride, n, D, 1, wrap, slot0))
    return view_too_large("hmc_half_sums");
  return hip_status(hmc::launch_half_sums(window, n_chains, chain_stride, sample_stride, D, wrap, slot0, n, tmax, work,
                                          out, (hipStream_t)stream),
                    "hmc_half_sums");
}

int64_t hmc_stream_work_size(int64_t n_chains, int32_t D, int32_t tmax) {
  if (n_chains < 1 || D < 1 || (tmax != 8 && tmax != 16 && tmax != 32 && tmax != 64)) return 0;
  return hmc::diag_stream_groups(n_chains) * (int64_t)tmax * D;
}

hmc_status hmc_stream_accumulate(const double* window, int64_t n_chains, int64_t chain_stride, int64_t sample_stride,
                                 int32_t D, int32_t wrap, int32_t slot0, int32_t carry, int32_t rows, int64_t pos0,
                                 int32_t n_half, double* shift, double* s1, double* s2, int32_t tmax, double* work,
                                 double* vsum, void* stream) {
  if (!window || !shift || !s1 || !s2 || !work || !vsum || n_chains < 1 || D < 1 || rows < 0 || carry < 0 ||
      n_half < 2 || pos0 < 0 || wrap < 1 || slot0 < 0 || slot0 >= wrap || carry + rows > wrap)
    return fail(HMC_EINVAL, "bad arguments");
  if (tmax != 8 && tmax != 16 && tmax != 32 && tmax != 64) return fail(HMC_EINVAL, "tmax must be 8, 16, 32 or 64");
  if (carry < (pos0 < tmax ? pos0 : tmax)) return fail(HMC_EINVAL, "carry must be >= min(tmax, pos0)");
  if (rows == 0) return HMC_OK;
  return hip_status(hmc::launch_stream_accum(window, n_chains, chain_stride, sample_stride, D, wrap, slot0, carry, rows,
                                             pos0, n_half, shift, s1, s2, tmax, work, vsum, (hipStream_t)stream),
                    "hmc_stream_accumulate");
}

}  // extern "C"
