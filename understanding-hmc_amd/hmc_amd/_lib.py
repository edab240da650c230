"""ctypes binding of libhmc.so (the C ABI declared in include/hmc.h).

The product path has no CPU fallback: if the HIP library is missing or cannot
be loaded this module raises at import of the engine (`lib()`), loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMC_AMD_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libhmc.so"))

HMC_OK, HMC_EINVAL, HMC_EDMAX, HMC_EHIP, HMC_EINDEX, HMC_ENOTSUP = range(6)
HMC_TARGET_DIAG, HMC_TARGET_DENSE = 0, 1
HMC_RNG_REPLAY, HMC_RNG_PHILOX = 0, 1
HMC_MODE_EXACT, HMC_MODE_FAST = 0, 1
(CNT_ACCEPT, CNT_ACCEPT_WU, CNT_LEAPFROG, CNT_LEAPFROG_SQ, CNT_OOB_REJECT, CNT_UNSTABLE, CNT_DMAX,
 CNT_ENERGY_EVALS, CNT_HANDOFF_GIVEUP) = range(9)
NCOUNTERS = 9
COUNTER_SLOTS = 4096   # include/hmc.h HMC_COUNTER_SLOTS: counters buffer is [slots][NCOUNTERS]
MIX_MAX_COMPONENTS, MIX_MAX_D = 8, 512   # include/hmc.h HMC_MIX_MAX_COMPONENTS, HMC_MIX_MAX_D
LOGIT_MAX_D, LOGIT_MAX_N = 128, 1 << 20   # include/hmc.h HMC_LOGIT_MAX_D, HMC_LOGIT_MAX_N
HMC_GLM_BERNOULLI, HMC_GLM_POISSON = 0, 1   # include/hmc.h hmc_glm.family

c_dp = ctypes.c_void_p  # device pointers are passed as integers (torch data_ptr())


class Target(ctypes.Structure):
    _fields_ = [("D", ctypes.c_int32), ("kind", ctypes.c_int32), ("q0", c_dp), ("prec", c_dp),
                ("logdet_const", ctypes.c_double)]


class Kinetic(ctypes.Structure):
    _fields_ = [("minv", c_dp), ("p_scale", c_dp), ("dt_vec", c_dp), ("dt", ctypes.c_double),
                ("minv_full", c_dp), ("p_chol_t", c_dp), ("kick", c_dp)]


class Schedule(ctypes.Structure):
    _fields_ = [("n_chains", ctypes.c_int64), ("chain_offset", ctypes.c_int64), ("n_iter", ctypes.c_int32),
                ("warm_up", ctypes.c_int32), ("thin", ctypes.c_int32), ("L_chain", ctypes.c_int32),
                ("L_low", ctypes.c_int32), ("L_high", ctypes.c_int32), ("iter_begin", ctypes.c_int32),
                ("iter_end", ctypes.c_int32), ("rng_mode", ctypes.c_int32), ("fp_mode", ctypes.c_int32),
                ("d_max", ctypes.c_int32), ("on_dmax", ctypes.c_int32), ("seed", ctypes.c_uint64)]


class Replay(ctypes.Structure):
    _fields_ = [("p0", c_dp), ("p", c_dp), ("L", c_dp), ("lnu", c_dp), ("tape", c_dp),
                ("tape_stride", ctypes.c_int64)]


class State(ctypes.Structure):
    _fields_ = [("q", c_dp), ("E_prev", c_dp), ("q_chain", c_dp), ("E_chain", c_dp), ("dE_chain", c_dp),
                ("counters", c_dp), ("traj_q", c_dp), ("traj_len", c_dp), ("decision", c_dp),
                ("n_save", ctypes.c_int32), ("traj_stride", ctypes.c_int32),
                ("qc_rows", ctypes.c_int64), ("qc_row0", ctypes.c_int64), ("order", c_dp)]


class Mixture(ctypes.Structure):
    """hmc_mixture: K Gaussians with diagonal covariances (device pointers)."""
    _fields_ = [("D", ctypes.c_int32), ("K", ctypes.c_int32), ("logw", c_dp), ("mu", c_dp), ("prec", c_dp),
                ("logdet_const", c_dp)]


class Logistic(ctypes.Structure):
    """hmc_logistic: design matrix, labels and prior precisions (device pointers)."""
    _fields_ = [("D", ctypes.c_int32), ("n", ctypes.c_int32), ("ldx", ctypes.c_int64), ("X", c_dp), ("y", c_dp),
                ("prior_prec", c_dp)]


class GLM(ctypes.Structure):
    """hmc_glm: hmc_logistic's data plus the family (device pointers)."""
    _fields_ = [("D", ctypes.c_int32), ("n", ctypes.c_int32), ("ldx", ctypes.c_int64), ("X", c_dp), ("y", c_dp),
                ("prior_prec", c_dp), ("family", ctypes.c_int32)]


ADAPT_STRIDE = 8   # include/hmc.h HMC_ADAPT_STRIDE: doubles of adaptation state per chain
(ADAPT_LOG_S, ADAPT_LOG_S_BAR, ADAPT_H_BAR, ADAPT_M, ADAPT_MU, ADAPT_SUM_ADAPT, ADAPT_SUM_AFTER,
 ADAPT_N_AFTER) = range(8)


class Adapt(ctypes.Structure):
    """hmc_adapt: the per-chain step-size adaptation state (device pointer) and its parameters."""
    _fields_ = [("state", c_dp), ("adapt_end", ctypes.c_int32), ("delta", ctypes.c_double),
                ("gamma", ctypes.c_double), ("t0", ctypes.c_double), ("kappa", ctypes.c_double)]


PRED_STRIDE = 8    # include/hmc.h HMC_PRED_STRIDE: doubles of one predictive record
(PRED_N, PRED_MU_MEAN, PRED_MU_M2, PRED_LL_MEAN, PRED_LL_M2, PRED_LL_MAX, PRED_LL_SUMEXP, PRED_RESERVED) = range(8)


class Samples(ctypes.Structure):
    """hmc_samples: a strided view of stored samples (device pointer) and the rows to read."""
    _fields_ = [("q", c_dp), ("n_chains", ctypes.c_int64), ("chain_stride", ctypes.c_int64),
                ("row_stride", ctypes.c_int64), ("row_begin", ctypes.c_int64), ("row_end", ctypes.c_int64),
                ("row_step", ctypes.c_int64)]


# include/hmc.h HMC_SELECT_BITS, HMC_SELECT_MAX_RANKS, HMC_SELECT_STATE_STRIDE (radix select)
SELECT_BITS, SELECT_MAX_RANKS, SELECT_STATE_STRIDE = 8, 8, 4
SELECT_BINS, SELECT_PASSES = 1 << SELECT_BITS, 64 // SELECT_BITS


# Exported symbols (tests check every one of these is present; keep in sync with include/hmc.h)
SYMBOLS = {
    "hmc_version": (ctypes.c_char_p, []),
    "hmc_last_error": (ctypes.c_char_p, []),
    "hmc_chain_init": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                      ctypes.POINTER(Replay), c_dp, ctypes.POINTER(State), c_dp]),
    "hmc_random_iters": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                        ctypes.POINTER(Replay), ctypes.POINTER(State), c_dp]),
    "hmc_chain_init_ws": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                         ctypes.POINTER(Replay), c_dp, ctypes.POINTER(State), ctypes.c_int64, c_dp]),
    "hmc_random_iters_ws": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic),
                                           ctypes.POINTER(Schedule), ctypes.POINTER(Replay), ctypes.POINTER(State),
                                           ctypes.c_int64, c_dp]),
    "hmc_random_leapfrog_form": (ctypes.c_int32, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic),
                                                  ctypes.POINTER(Schedule)]),
    "hmc_random_layout": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Schedule),
                                         ctypes.POINTER(ctypes.c_int32 * 4)]),
    "hmc_random_layout_ex": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic),
                                            ctypes.POINTER(Schedule), ctypes.POINTER(ctypes.c_int32 * 4)]),
    "hmc_workspace_register": (ctypes.c_int, [c_dp, ctypes.c_int64]),
    "hmc_stream_work_size": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "hmc_stream_accumulate": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int64, ctypes.c_int32, c_dp, c_dp, c_dp, ctypes.c_int32, c_dp,
                                             c_dp, c_dp]),
    "hmc_random_workspace_size": (ctypes.c_int64, [ctypes.POINTER(Target), ctypes.c_int64]),
    "hmc_random_workspace_size_ex": (ctypes.c_int64, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic),
                                                      ctypes.c_int64]),
    "hmc_nuts_workspace_size": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    "hmc_nuts_workspace_size_ex": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                                    ctypes.c_int32]),
    "hmc_nuts_iters": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                      ctypes.POINTER(Replay), ctypes.POINTER(State), c_dp, c_dp]),
    "hmc_nuts_iters_ws": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                         ctypes.POINTER(Replay), ctypes.POINTER(State), c_dp, ctypes.c_int64, c_dp]),
    "hmc_leapfrog": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                    c_dp, c_dp, ctypes.c_int32, c_dp]),
    "hmc_energy": (ctypes.c_int, [ctypes.POINTER(Target), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                  c_dp, c_dp]),
    "hmc_mix_chain_init": (ctypes.c_int, [ctypes.POINTER(Mixture), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                          ctypes.POINTER(Replay), c_dp, ctypes.POINTER(State), c_dp]),
    "hmc_mix_random_iters": (ctypes.c_int, [ctypes.POINTER(Mixture), ctypes.POINTER(Kinetic),
                                            ctypes.POINTER(Schedule), ctypes.POINTER(Replay), ctypes.POINTER(State),
                                            c_dp]),
    "hmc_mix_leapfrog": (ctypes.c_int, [ctypes.POINTER(Mixture), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                        c_dp, c_dp, c_dp]),
    "hmc_mix_energy": (ctypes.c_int, [ctypes.POINTER(Mixture), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                      c_dp, c_dp]),
    "hmc_logit_chain_init": (ctypes.c_int, [ctypes.POINTER(Logistic), ctypes.POINTER(Kinetic),
                                            ctypes.POINTER(Schedule), ctypes.POINTER(Replay), c_dp,
                                            ctypes.POINTER(State), c_dp]),
    "hmc_logit_random_iters": (ctypes.c_int, [ctypes.POINTER(Logistic), ctypes.POINTER(Kinetic),
                                              ctypes.POINTER(Schedule), ctypes.POINTER(Replay),
                                              ctypes.POINTER(State), c_dp]),
    "hmc_logit_leapfrog": (ctypes.c_int, [ctypes.POINTER(Logistic), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp,
                                          c_dp, c_dp, c_dp, c_dp]),
    "hmc_logit_energy": (ctypes.c_int, [ctypes.POINTER(Logistic), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                        c_dp, c_dp]),
    "hmc_glm_chain_init": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                          ctypes.POINTER(Replay), c_dp, ctypes.POINTER(State), c_dp]),
    "hmc_glm_random_iters": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                            ctypes.POINTER(Replay), ctypes.POINTER(State), c_dp]),
    "hmc_glm_leapfrog": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                        c_dp, c_dp, c_dp]),
    "hmc_glm_energy": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic), ctypes.c_int64, c_dp, c_dp,
                                      c_dp, c_dp]),
    "hmc_glm_nuts_workspace_size": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]),
    "hmc_glm_nuts_iters": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic), ctypes.POINTER(Schedule),
                                          ctypes.POINTER(Replay), ctypes.POINTER(State), c_dp, ctypes.c_int64, c_dp]),
    "hmc_adapt_init": (ctypes.c_int, [c_dp, ctypes.c_int64, c_dp, c_dp]),
    "hmc_glm_random_iters_adapt": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic),
                                                  ctypes.POINTER(Schedule), ctypes.POINTER(Replay),
                                                  ctypes.POINTER(State), ctypes.POINTER(Adapt), c_dp]),
    "hmc_glm_nuts_iters_adapt": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Kinetic),
                                                ctypes.POINTER(Schedule), ctypes.POINTER(Replay),
                                                ctypes.POINTER(State), c_dp, ctypes.c_int64,
                                                ctypes.POINTER(Adapt), c_dp]),
    "hmc_glm_predictive_workspace_size": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]),
    "hmc_glm_predictive_blocks": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64, ctypes.c_int64]),
    "hmc_glm_predictive": (ctypes.c_int, [ctypes.POINTER(GLM), ctypes.POINTER(Samples), c_dp, c_dp, ctypes.c_int64,
                                          c_dp]),
    "hmc_select_workspace_size": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32]),
    "hmc_select_grid": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int64]),
    "hmc_select_init": (ctypes.c_int, [c_dp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                       ctypes.c_int64, c_dp]),
    "hmc_select_count": (ctypes.c_int, [ctypes.POINTER(Samples), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                        c_dp, c_dp, c_dp]),
    "hmc_select_pick": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_dp, c_dp, c_dp]),
    "hmc_select_values": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, c_dp, c_dp, c_dp]),
    "hmc_order_stats": (ctypes.c_int, [ctypes.POINTER(Samples), ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_int64), c_dp, c_dp, ctypes.c_int64, c_dp]),
    "hmc_rng_normals": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_int32, c_dp, c_dp]),
    "hmc_philox": (ctypes.c_int, [ctypes.c_uint32] * 6 + [ctypes.c_int64, c_dp, c_dp]),
    "hmc_split_moments": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_int32, c_dp, c_dp, c_dp]),
    "hmc_rowsum_work_size": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "hmc_rowsum": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.c_int32, c_dp, c_dp, c_dp, c_dp]),
    "hmc_convergence_work_size": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "hmc_convergence_sums": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_dp, c_dp, c_dp]),
    "hmc_half_sums": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_dp, c_dp,
                                     c_dp]),
    "hmc_variogram_work_size": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "hmc_variogram": (ctypes.c_int, [c_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, c_dp, c_dp,
                                     c_dp]),
}

_lib = None


class HMCError(RuntimeError):
    pass


def lib():
    """Load libhmc.so once.  Raises (no fallback) when it is absent."""
    global _lib
    if _lib is None:
        path = os.environ.get("HMC_LIB_PATH", LIB_PATH)      # A/B builds of the same tree
        if not os.path.exists(path):
            raise RuntimeError(f"libhmc.so not found at {path}: build it with "
                               f"`python -c 'import __graft_entry__ as g; g.build()'` (make in csrc/)")
        L = ctypes.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what=""):
    """Map hmc_status to the exception type the reference raises for the same condition."""
    if status == HMC_OK:
        return
    msg = lib().hmc_last_error().decode(errors="replace")
    text = f"{what}: {msg}" if what else msg
    if status in (HMC_EINVAL, HMC_EDMAX):
        raise AssertionError(text)       # reference validates with assert (samplers.py:331-348, :598)
    if status == HMC_EINDEX:
        raise IndexError(text)           # samplers.py:471 negative-index write (Q5)
    if status == HMC_ENOTSUP:
        raise NotImplementedError(text)
    raise HMCError(text)


def random_layout(D, L_low, L_high, dt=None):
    """hmc_random_layout for a diagonal target (host only): (K pairs per lane, lanes per chain,
    chains per wave, 1 for the wave-per-chain kernels / 0 for the lane-group kernel and for the
    four-chains-per-wave kernel of D = 97..112, which answers (4, 16, 4, 0)).  With a scalar `dt`
    (hmc_random_layout_ex, identity mass) the four-chain answer also depends on the three-term rule
    for that step size and L_high, as the launch does."""
    T = Target(D, HMC_TARGET_DIAG, None, None, 0.0)
    S = Schedule(0, 0, 1, 0, 1, 2, L_low, L_high, 1, 1, HMC_RNG_PHILOX, HMC_MODE_FAST, 10, 0, 0)
    out = (ctypes.c_int32 * 4)()
    if dt is None:
        check(lib().hmc_random_layout(ctypes.byref(T), ctypes.byref(S), ctypes.byref(out)), "hmc_random_layout")
    else:
        K = Kinetic(None, None, None, float(dt), None, None, None)
        check(lib().hmc_random_layout_ex(ctypes.byref(T), ctypes.byref(K), ctypes.byref(S), ctypes.byref(out)),
              "hmc_random_layout_ex")
    return tuple(out)


def random_leapfrog_form(D, L_low, L_high, dt):
    """hmc_random_leapfrog_form for an identity target and mass in FAST mode with Philox draws
    (host only): 1 for the three-term recurrence, 0 for the two-FMA loops."""
    T = Target(D, HMC_TARGET_DIAG, None, None, 0.0)
    K = Kinetic(None, None, None, float(dt), None, None, None)
    S = Schedule(0, 0, 1, 0, 1, 2, L_low, L_high, 1, 1, HMC_RNG_PHILOX, HMC_MODE_FAST, 10, 0, 0)
    return int(lib().hmc_random_leapfrog_form(ctypes.byref(T), ctypes.byref(K), ctypes.byref(S)))


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    return None if t is None else t.data_ptr()
