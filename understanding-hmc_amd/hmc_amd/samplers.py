"""HMC_sampler — the reference's sampler-class surface, running on MI355X.

Mirror of jaekor91/understanding-HMC `samplers.py` (class `sampler`, :4-291, and
`HMC_sampler`, :297-924): same constructor signature and defaults, same
`gen_sample` / `compute_convergence_stats` entry points, same result attributes
(NumPy arrays of the same shapes and dtypes).  The chains run in the fused HIP
kernels of libhmc.so (understanding-hmc_amd/csrc); this module only prepares
device buffers and random streams and calls the C ABI.  There is no CPU engine.

Randomness (new optional kwarg `rng`):
  * "replay" (default): the momentum / trajectory-length / uniform draws are taken
    from the global legacy `np.random` in exactly the reference's order
    (samplers.py:415, :431, :441, :461 — SURVEY Q7) and replayed on the GPU, so
    with the same `np.random.seed` the results equal the reference's
    (bit-identical q_chain for diagonal targets in fp_mode="exact").
  * "philox": in-kernel Philox4x32-10 keyed by (seed, global chain id, iteration):
    for production sizes (the host streams would not fit); statistically
    equivalent, independent of launch geometry and GPU count.
"""
import time
import warnings

import numpy as np
import torch

from . import _lib as H
from . import descriptors as Dsc
from .descriptors import dev_tensor as _dev_tensor
from .diagnostics import StreamingDiagnostics
from .engine import NutsEngine, RandomEngine, kernel_target
from .target import GLMTarget, LogisticTarget, MixtureTarget, MVNTarget, probe_closures  # noqa: F401
from . import utils as U


class sampler(object):
    """Parent class (samplers.py:4-64): storage of chains and convergence stats."""

    def __init__(self, D, target_lnL, Nchain=2, Niter=1000, thin_rate=1, warm_up_num=0):
        self.D = D
        self.target_lnL = target_lnL
        self.Nchain = Nchain
        self.Niter = Niter
        self.thin_rate = thin_rate
        self.warm_up_num = warm_up_num
        self.L_chain = 1 + ((self.Niter - self.warm_up_num) // self.thin_rate)   # samplers.py:31
        if self.L_chain < 0:
            raise ValueError("negative dimensions are not allowed")             # np.zeros at :33
        self.q_chain = np.zeros((self.Nchain, self.L_chain, self.D), dtype=float)
        self.lnL_chain = np.zeros((self.Nchain, self.L_chain, 1))
        self.R_q = None
        self.R_lnL = None
        self.n_eff_q = None
        self.accept_R_warm_up = None
        self.accept_R = None
        self.dt_total = 0
        self.N_total_steps = 0

    def compute_convergence_stats(self):
        """samplers.py:53-64: stats over q_chain[:, 1:, :] (the first point is dropped, Q16).
        Computed on the device by the diagnostics kernels when the chain lives there."""
        src = getattr(self, "q_chain_device", None)
        if src is None:
            src = self.q_chain
        self.R_q, self.n_eff_q = U.convergence_stats(src[:, 1:, :], warm_up_num=0, thin_rate=1)
        return

    def plot_samples(self, title_prefix, show=False, savefig=False, xmax=None, dx=None, plot_normal=True,
                     plot_cov=True, q0=None, cov0=None):
        """samplers.py:67-291: the 3x3 summary figure, drawn on the host from the GPU results
        (hmc_amd.plots).  Returns the figure's numbers (plots.sample_summary)."""
        from . import plots
        return plots.plot_samples(self, title_prefix, show=show, savefig=savefig, xmax=xmax, dx=dx,
                                  plot_normal=plot_normal, plot_cov=plot_cov, q0=q0, cov0=cov0)


class HMC_sampler(sampler):
    """HMC sampler for a multivariate-normal (or Gaussian-mixture, or logistic-regression) target on
    MI355X (samplers.py:297-924).

    Extra optional kwargs (all new; defaults keep the reference behaviour):
      target   : MVNTarget; if None, V/dVdq are affine-probed (target.probe_closures).  Or a
                 MixtureTarget (K Gaussians with diagonal covariances; sampler_type="Random", a
                 diagonal cov_p, D <= 512, K <= 8: anything else raises NotImplementedError here,
                 before any launch; fp_mode changes nothing for it).  Or a LogisticTarget (design
                 matrix X (n, D), labels y, normal prior; sampler_type="Random", a diagonal cov_p,
                 D <= 128, n <= 2^20: anything else raises NotImplementedError here; fp_mode changes
                 nothing for it either).  Or a GLMTarget (the logistic target's data and limits plus a
                 family, "poisson" or "bernoulli"): sampler_type="Random" or "NUTS", the one target
                 with kernels of its own that NUTS runs on.  With a target, V / dVdq may be None:
                 they are set to the target's host methods
      rng      : "replay" | "philox"
      seed     : Philox key (rng="philox")
      fp_mode  : "exact" (reference rounding, no FMA) | "fast" (FMA-contracted integrator)
      device   : torch device (default: current CUDA device)
      store_chain : keep the full (Nchain, L_chain, D) chain (default True).  False = streaming
                    mode: q_chain is None, R_q / n_eff_q come from on-device streamed sums
      stream_tmax, stream_feed : streaming mode's largest variogram lag and the iterations
                    between diagnostics updates
      iters_per_launch : iterations fused in one kernel launch (default: all)
      chain_offset : global id of this object's first chain (multi-GPU sharding)
      adapt_step : GLMTarget only (anything else raises NotImplementedError here, before any launch).
                 Every chain adapts a multiplier s of `dt` (effective step s * dt, scalar or vector;
                 cov_p unchanged) during the reference's warm-up iterations 1 <= i < warm_up_num, by
                 the dual averaging of Hoffman & Gelman 2014 towards a mean acceptance statistic
                 `adapt_delta`, and runs at the averaged multiplier from warm_up_num on.  Per chain:
                 results still depend on nothing but the global chain id.  mu = log(step_scale0), so
                 `dt` is the point the iterates shrink to (Stan's log(10 s0) overflows exp(z) of the
                 Poisson family on its first jump).  After a run: `step_scale` (Nchain,)
                 the final multipliers exp(log_s_bar); `accept_stat_warm_up`, `accept_stat` the mean
                 acceptance statistic over chains and iterations before / from warm_up_num (Random:
                 min(1, exp(-dE)); NUTS: the mean over the tree's points of min(1, exp(E_init - E)));
                 `adapt_state` the (Nchain, 8) state array.  accept_R keeps the reference's meaning
      adapt_delta : target of the mean acceptance statistic, in (0, 1) (default 0.8)
      step_scale0 : multipliers to start from, a scalar or (Nchain,) (default 1), e.g. a pooled
                 `step_scale` of an earlier run; without adapt_step they stay as given
    """

    def __init__(self, D, V, dVdq, Nchain=2, Niter=1000, thin_rate=1, warm_up_num=0,
                 cov_p=None, sampler_type="Fixed", L=None, global_dt=True, dt=None,
                 L_low=None, L_high=None, log2L=None, d_max=10, target=None, rng="replay", seed=0,
                 fp_mode="exact", device=None, store_chain=True, iters_per_launch=None, chain_offset=0,
                 stream_tmax=64, stream_feed=60, adapt_step=False, adapt_delta=0.8, step_scale0=None):
        sampler.__init__(self, D=D, target_lnL=None, Nchain=Nchain, Niter=Niter, thin_rate=thin_rate,
                         warm_up_num=warm_up_num)
        self.V = V
        self.dVdq = dVdq
        assert (sampler_type == "Fixed") or (sampler_type == "Random") or (sampler_type == "NUTS") or \
            (sampler_type == "Static")                                            # samplers.py:331
        assert (dt is not None)                                                   # :332
        self.dt = dt
        self.global_dt = global_dt
        self.sampler_type = sampler_type
        if self.sampler_type == "Fixed":
            assert (L is not None)
            self.L = L
        elif self.sampler_type == "Random":
            assert (L_low is not None) and (L_high is not None)
            self.L_low = L_low
            self.L_high = L_high
        elif self.sampler_type == "Static":
            assert (log2L is not None)
            self.log2L = log2L
        elif self.sampler_type == "NUTS":
            assert d_max is not None
            self.d_max = d_max
        if cov_p is None:                                                         # :352-356
            self.cov_p = np.diag(np.ones(self.D))
        else:
            self.cov_p = cov_p
        self.inv_cov_p = np.linalg.inv(self.cov_p)
        self.E_chain = np.zeros((self.Nchain, self.L_chain, 1), dtype=float)     # :359-360
        self.dE_chain = np.zeros((self.Nchain, self.L_chain, 1), dtype=float)

        assert rng in ("replay", "philox")
        assert fp_mode in ("exact", "fast")
        self.rng = rng
        self.seed = int(seed)
        self.fp_mode = fp_mode
        self.store_chain = store_chain
        self.stream_tmax, self.stream_feed = int(stream_tmax), int(stream_feed)
        if not store_chain:
            self.q_chain = None
        self.iters_per_launch = iters_per_launch
        self.chain_offset = int(chain_offset)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._target = target
        if target is not None:
            if self.V is None:
                self.V = target.V
            if self.dVdq is None:
                self.dVdq = target.dVdq
        self._kernel_target = row = kernel_target(target)       # engine.KERNEL_TARGETS; None: MVN
        if row:
            assert target.D == self.D
            if self.sampler_type == "NUTS" and row.nuts_engine is None:
                raise NotImplementedError("NUTS on a %s target is not supported (sampler_type='Random')" % row.name)
            row.engine.check_supported(target, self.cov_p)
        # step-size adaptation: the GLM kernels alone have the ADAPT forms
        self._adapt_kw = {}
        if adapt_step or step_scale0 is not None:
            if not isinstance(target, GLMTarget):
                raise NotImplementedError("adapt_step / step_scale0 are supported for a GLMTarget only "
                                          "(sampler_type 'Random' or 'NUTS')")
            if not 0.0 < float(adapt_delta) < 1.0:
                raise AssertionError("adapt_delta=%r: the target acceptance statistic lies in (0, 1)" % (adapt_delta,))
            self._adapt_kw = dict(adapt_step=bool(adapt_step), adapt_delta=float(adapt_delta),
                                  step_scale0=step_scale0)
        self.step_scale = self.accept_stat_warm_up = self.accept_stat = self.adapt_state = None
        self.n_leapfrog = 0
        self.q_chain_device = None

    # ------------------------------------------------------------------ target / descriptors
    def target(self):
        if self._target is None:
            self._target = probe_closures(self.D, self.V, self.dVdq)
        return self._target

    def _row_call(self, which, rows, out_shapes, what=None, extra=()):
        """The row-wise C call `which` ("leapfrog" | "energy") of this target's kernels on the host
        arrays `rows`; returns its outputs, of shapes `out_shapes`, as NumPy arrays.  `what` names
        the call in error messages (default: the entry); `extra`: arguments before the stream.
        p_chol_t is not built: these calls draw no momenta, so a cov_p with an inverse and no
        Cholesky factor works here."""
        dev, row = self.device, self._kernel_target
        if row:
            T, keep = row.upload(self._target, dev)
            kin = Dsc.host_kinetic(self.D, self.cov_p, self.dt)
            entry = getattr(row, which)
        else:
            mvn, kin = Dsc.host_descriptors(self.target(), self.cov_p, self.dt)
            T, keep = Dsc.upload_mvn(self.target(), mvn, dev)
            entry = "hmc_" + which
        K, keep_k = Dsc.upload_kinetic(kin, dev)
        ins = [_dev_tensor(r, dev) for r in rows]
        outs = [torch.empty(shape, dtype=torch.float64, device=dev) for shape in out_shapes]
        H.check(getattr(H.lib(), entry)(T, K, rows[0].shape[0], *[H.ptr(x) for x in ins + outs], *extra,
                                        torch.cuda.current_stream(dev).cuda_stream), what or entry)
        return [o.cpu().numpy() for o in outs]

    # ------------------------------------------------------------------ public API
    def gen_sample(self, q_start, N_save_chain0=0, verbose=True):
        """samplers.py:363-383: dispatch Random / NUTS; other types silently do nothing."""
        if self.sampler_type == "Random":
            self.gen_sample_random(q_start, N_save_chain0, verbose)
        elif self.sampler_type == "NUTS":
            self.gen_sample_NUTS(q_start, N_save_chain0, verbose)
        return

    def _replay_streams_random(self):
        """Draw p0, p, L, u from the global legacy np.random in the reference order (Q7):
        per chain: p0 (:415), then per iteration: p (:431), L (:441), u (:461)."""
        N, I, D = self.Nchain, self.Niter, self.D
        if N * I * D > (1 << 28):
            raise MemoryError("replay streams too large for the host; use rng='philox'")
        p0 = np.empty((N, D))
        P = np.empty((N, I, D))
        Ls = np.empty((N, I), dtype=np.int32)
        U_ = np.empty((N, I))
        ident = np.array_equal(self.cov_p, np.eye(D))
        zeros = np.zeros(D)
        for m in range(N):
            p0[m] = np.random.standard_normal(D) if ident else \
                np.random.multivariate_normal(zeros, self.cov_p, size=1)[0]
            for i in range(I):
                P[m, i] = np.random.standard_normal(D) if ident else \
                    np.random.multivariate_normal(zeros, self.cov_p, size=1)[0]
                Ls[m, i] = np.random.randint(low=self.L_low, high=self.L_high, size=1)[0]
                U_[m, i] = np.random.random(1)[0]
        with np.errstate(divide="ignore"):
            lnu = np.log(U_)
        return p0, P, Ls, lnu

    def set_random_replay(self, p0, P, Ls, lnu):
        """Explicit draw streams for rng="replay" with the Random sampler: p0 (Nchain, D), p (Nchain,
        Niter, D), L (Nchain, Niter), log u (Nchain, Niter), used instead of drawing them from the
        global np.random (RandomEngine.set_replay)."""
        self._random_replay = (np.asarray(p0, np.float64), np.asarray(P, np.float64), np.asarray(Ls),
                               np.asarray(lnu, np.float64))

    def gen_sample_random(self, q_start, N_save_chain0, verbose):
        """samplers.py:387-491 on the GPU (fused kernel hmc_random_iters via RandomEngine)."""
        q_start = np.asarray(q_start, dtype=np.float64)
        assert q_start.shape[0] == self.Nchain                                    # :396
        torch.cuda.set_device(self.device)
        n_save = int(N_save_chain0) if N_save_chain0 > 0 else 0
        # the target's own kernels (hmc_mix.hip, hmc_logit.hip) or the MVN kernels
        engine = self._kernel_target.engine if self._kernel_target else RandomEngine
        eng = engine(self.target(), self.Nchain, self.Niter, self.warm_up_num, self.thin_rate, self.L_low,
                     self.L_high, self.dt, cov_p=self.cov_p, rng=self.rng, seed=self.seed,
                     fp_mode=self.fp_mode, chain_offset=self.chain_offset, store_chain=self.store_chain,
                     n_save=n_save, device=self.device, **self._adapt_kw)
        if self.rng == "replay":
            eng.set_replay(*(getattr(self, "_random_replay", None) or self._replay_streams_random()))
        t0 = time.time()
        eng.init(q_start.reshape(self.Nchain, self.D))
        self._run(eng)
        torch.cuda.synchronize(self.device)
        elapsed = time.time() - t0
        self._finish(eng, elapsed, verbose)
        print("Compute acceptance rate")                                         # :483-489
        if self.warm_up_num > 0:
            self.accept_R_warm_up = self._acc_wu / float(self.Nchain * self.warm_up_num)
            print("During warm up: %.3f" % self.accept_R_warm_up)
        self.accept_R = self._acc / float(self.Nchain * (self.Niter - self.warm_up_num + 1))
        print("After warm up: %.3f" % self.accept_R)
        print("Completed.")
        return

    def _run(self, eng):
        """All Niter iterations.  With store_chain the whole q_chain stays on the device and one
        launch covers `iters_per_launch` iterations (default: the whole run).  Without it
        (streaming mode) the rows go to a circular device window that feeds
        StreamingDiagnostics after every `stream_feed` iterations, so memory is
        O(Nchain * (stream_tmax + window) * D) and compute_convergence_stats() reads the
        streamed sums instead of a q_chain."""
        self._stream_diag = None
        if self.store_chain:
            step = self.iters_per_launch or self.Niter
            for it0 in range(1, self.Niter + 1, step):
                eng.run(it0, min(it0 + step, self.Niter + 1))
            return
        n_samples = self.L_chain - 1
        if n_samples < 4:
            raise AssertionError("streaming statistics need L_chain - 1 >= 4 samples per chain")
        tmax = next(t for t in (8, 16, 32, 64) if t >= min(int(self.stream_tmax), 64))   # kernel lag rings
        diag = StreamingDiagnostics(self.Nchain, self.D, n_samples, tmax=tmax, device=self.device)
        step = self.iters_per_launch or 20
        feed = max(step, (int(self.stream_feed) // step) * step)
        eng.run_streaming(diag, 1, self.Niter + 1, step, feed=feed)
        self._stream_diag = diag

    def compute_convergence_stats(self):
        """samplers.py:53-64.  In streaming mode (store_chain=False) the split-chain sums were
        accumulated on the device during the run: R-hat is exact, the ESS sum stops at lag
        stream_tmax if the reference's criterion has not fired by then."""
        diag = getattr(self, "_stream_diag", None)
        if diag is not None:
            self.R_q, self.n_eff_q = diag.finish()
            self.stream_info = dict(diag.info)
            if diag.info["truncated_dims"]:
                warnings.warn("streaming ESS: %d of %d dimensions need variogram lags beyond stream_tmax=%d; "
                              "their n_eff is the sum truncated there, not the reference's value.  The exact "
                              "estimator streams up to %s samples per chain (2*(stream_tmax + stream_feed/thin) "
                              "+ 1); this run has %d: raise stream_feed or store q_chain"
                              % (diag.info["truncated_dims"], self.D, diag.tmax, diag.info.get("exact_max_samples"),
                                 diag.info.get("n_samples", 0)), UserWarning, stacklevel=2)
            return
        sampler.compute_convergence_stats(self)

    # ------------------------------------------------------------------ posterior predictive / WAIC
    def _predictive_partials(self, X, y, what):
        """Records of hmc_amd.predictive over rows 1.. of every chain (the start row is dropped, as
        compute_convergence_stats does): of _stored_samples."""
        from . import predictive as P
        t = self._target
        if not isinstance(t, GLMTarget):
            raise NotImplementedError("%s is supported for a GLMTarget only" % what)
        return P.glm_predictive_partials(X, y, t.family, self._stored_samples(what), rows=slice(1, None),
                                         device=self.device)

    def posterior_predictive(self, X_new=None):
        """Posterior predictive mean and variance of a new observation at the rows X_new (n_eval, D)
        (default: the target's own X), reduced on the device (hmc_amd.predictive): a dict with n,
        mean and var per row.  GLMTarget only; after gen_sample."""
        from . import predictive as P
        t = self._target
        X = t.X if (X_new is None and isinstance(t, GLMTarget)) else X_new
        part = self._predictive_partials(X, None, "posterior_predictive")
        return P.finish(part, None, t.family)

    def waic(self):
        """lppd, p_waic, elpd_waic, waic = -2 elpd_waic and its standard error on the data the target
        was fitted on (Gelman, Hwang & Vehtari 2014), with the per-row terms (hmc_amd.predictive.finish).
        GLMTarget only; after gen_sample."""
        from . import predictive as P
        t = self._target
        part = self._predictive_partials(getattr(t, "X", None), getattr(t, "y", None), "waic")
        return P.finish(part, t.y, t.family)

    # ------------------------------------------------------------------ posterior quantiles
    def _stored_samples(self, what):
        """The stored samples of the last run: q_chain_device where the run left it, else q_chain."""
        src = getattr(self, "q_chain_device", None)
        if src is None and getattr(self, "engine", None) is not None:
            src = self.q_chain
        if src is None:
            raise RuntimeError("%s needs the samples of a run: call gen_sample first (with store_chain)" % what)
        return src

    def quantiles(self, probs=(0.05, 0.5, 0.95)):
        """Posterior quantiles of every coordinate over rows 1.. of every chain (the start row is
        dropped, as compute_convergence_stats does): a (len(probs), D) array equal to
        np.quantile(q_chain[:, 1:].reshape(-1, D), probs, axis=0), from exact order statistics selected
        on the device (hmc_amd.quantiles).  Any target, either sampler; after gen_sample."""
        from . import quantiles as Q
        return Q.quantiles(self._stored_samples("quantiles"), probs, rows=slice(1, None), device=self.device)

    def credible_interval(self, level=0.9):
        """The central credible interval of every coordinate: the (lo, hi) pair of (D,) arrays of the
        posterior quantiles (1 - level) / 2 and 1 - (1 - level) / 2 (hmc_amd.quantiles)."""
        from . import quantiles as Q
        return Q.credible_interval(self._stored_samples("credible_interval"), level, rows=slice(1, None),
                                   device=self.device)

    def _finish(self, eng, elapsed, verbose):
        """Copy results to the reference's NumPy attributes and derive the counters."""
        c = eng.read_counters()
        if c[H.CNT_OOB_REJECT] > 0:
            raise IndexError("index out of bounds for q_chain during warm-up (reference samplers.py:471)")
        self._acc, self._acc_wu = int(c[H.CNT_ACCEPT]), int(c[H.CNT_ACCEPT_WU])
        self.n_leapfrog = int(c[H.CNT_LEAPFROG])
        N, D = self.Nchain, self.D
        self.N_total_steps += N * (1 + 2 * self.Niter) + D * int(c[H.CNT_LEAPFROG_SQ])   # Q13
        if verbose:
            self.dt_total += elapsed
            print("Ran %d chains on %s: %.2f s" % (N, self.device, elapsed))
        self._publish(eng)
        if eng.n_save:
            n_save = eng.n_save
            self.decision_chain = np.zeros((n_save + 1, 1), dtype=int)
            self.decision_chain[:n_save, 0] = eng.decision.cpu().numpy()
            T_ = eng.traj.cpu().numpy()
            tl = eng.traj_len.cpu().numpy()
            self.phi_q = [T_[i, :tl[i]].copy() for i in range(n_save) if tl[i] > 0]

    def _publish(self, eng):
        """The run's results as the reference's NumPy attributes (q_chain None in streaming mode:
        statistics only), the engine and its device arrays, and, of a run through the _adapt entries,
        step_scale, accept_stat_warm_up, accept_stat and adapt_state (include/hmc.h: hmc_adapt state
        slots; None otherwise)."""
        self.engine = eng
        self.q_chain_device = eng.q_chain
        self.q_device = eng.q
        self.q_chain = eng.q_chain.cpu().numpy() if eng.q_chain is not None else None
        self.E_chain = eng.E_chain.cpu().numpy()[:, :, None]
        self.dE_chain = eng.dE_chain.cpu().numpy()[:, :, None]
        st = getattr(eng, "adapt_state", None)
        if st is None:
            return
        st = st.cpu().numpy()
        self.adapt_state = st
        self.step_scale = np.exp(st[:, H.ADAPT_LOG_S_BAR])
        n_adapt, n_after = st[:, H.ADAPT_M].sum(), st[:, H.ADAPT_N_AFTER].sum()
        self.accept_stat_warm_up = st[:, H.ADAPT_SUM_ADAPT].sum() / n_adapt if n_adapt > 0 else None
        self.accept_stat = st[:, H.ADAPT_SUM_AFTER].sum() / n_after if n_after > 0 else None

    def set_nuts_replay(self, p0, P, tape):
        """Explicit NUTS draw streams (rng="replay"): p0 (Nchain, D), p (Nchain, Niter, D) and a
        per-chain tape (Nchain, T) of the directions (:608) and uniforms (:750, :773) in the
        order the reference consumes them.  NUTS interleaves these draws with the data-dependent
        tree, so they cannot be pre-drawn from the global np.random; without a tape,
        rng="replay" NUTS runs the Philox streams keyed by a seed drawn from np.random (so
        np.random.seed still makes the run reproducible)."""
        self._nuts_replay = (np.asarray(p0, np.float64), np.asarray(P, np.float64), np.asarray(tape, np.float64))

    def gen_sample_NUTS(self, q_start, N_save_chain0, verbose, on_dmax="raise"):
        """samplers.py:495-808 on the GPU (hmc_nuts_iters via NutsEngine).  The reference's
        `assert False` at d > d_max-1 (:596-598) becomes AssertionError after the run
        (on_dmax="raise") or keeps the current sample (on_dmax="break")."""
        q_start = np.asarray(q_start, dtype=np.float64)
        assert q_start.shape[0] == self.Nchain                                    # :510
        if N_save_chain0 > 0:
            self.phi_q = []                                                       # :511-514 (never filled)
        torch.cuda.set_device(self.device)
        tape = getattr(self, "_nuts_replay", None)
        rng, seed = self.rng, self.seed
        if rng == "replay" and tape is None:
            # the reference draws directions and uniforms from np.random in a data-dependent order
            # (:608, :748, :773) that chain-parallel trees cannot follow: say that this run differs
            warnings.warn("NUTS rng='replay' without set_nuts_replay(): running Philox streams seeded "
                          "from np.random (reproducible, statistically equivalent, not the reference's "
                          "draws)", UserWarning, stacklevel=2)
            rng, seed = "philox", int(np.random.randint(0, 2 ** 62, dtype=np.int64))
        # the target's own NUTS kernel (hmc_glm_nuts.hip) or the MVN kernels
        engine = self._kernel_target.nuts_engine if self._kernel_target else NutsEngine
        eng = engine(self.target(), self.Nchain, self.Niter, self.warm_up_num, self.thin_rate, self.d_max,
                     self.dt, cov_p=self.cov_p, rng=rng, seed=seed, fp_mode=self.fp_mode,
                     chain_offset=self.chain_offset, store_chain=self.store_chain, on_dmax=on_dmax,
                     device=self.device,
                     iters_per_call=(self.iters_per_launch or self.Niter) if self.store_chain
                     else (self.iters_per_launch or 20),                      # (_run's launch sizes)
                     **self._adapt_kw)
        if rng == "replay":
            eng.set_replay(*tape)
        t0 = time.time()
        eng.init(q_start.reshape(self.Nchain, self.D))
        self._run(eng)
        torch.cuda.synchronize(self.device)
        elapsed = time.time() - t0
        c = eng.read_counters()
        if c[H.CNT_HANDOFF_GIVEUP] > 0:
            raise RuntimeError("NUTS kernel: %d chain hand-offs timed out" % c[H.CNT_HANDOFF_GIVEUP])
        if c[H.CNT_OOB_REJECT] > 0:
            raise IndexError("NUTS replay tape exhausted")
        if c[H.CNT_DMAX] > 0 and on_dmax == "raise":
            raise AssertionError("Doubling number d exceeds d_max = %d" % self.d_max)   # :596-598
        N, D = self.Nchain, self.D
        self.n_leapfrog = int(c[H.CNT_LEAPFROG])
        self.n_unstable = int(c[H.CNT_UNSTABLE])
        self.n_dmax = int(c[H.CNT_DMAX])
        self.N_total_steps += N * (1 + self.Niter) + (D + 1) * self.n_leapfrog  # :553, :570, :614-619, :640-644
        if verbose:
            self.dt_total += elapsed
            print("Ran %d NUTS chains on %s: %.2f s" % (N, self.device, elapsed))
        self._publish(eng)
        print("Compute acceptance rate: By default equal to 1.")                 # :800-805
        if self.warm_up_num > 0:
            self.accept_R_warm_up = 1.
            print("During warm up: %.3f" % self.accept_R_warm_up)
        self.accept_R = 1.
        print("After warm up: %.3f" % self.accept_R)
        print("Completed.")
        return

    # ------------------------------------------------------------------ primitives (batched on GPU)
    def leap_frog(self, p_old, q_old):
        """samplers.py:831-839 for one (p, q) row or a batch of rows, on the GPU."""
        p = np.atleast_2d(np.asarray(p_old, dtype=np.float64))
        q = np.atleast_2d(np.asarray(q_old, dtype=np.float64))
        mode = () if self._kernel_target else (H.HMC_MODE_EXACT if self.fp_mode == "exact" else H.HMC_MODE_FAST,)
        pn, qn = self._row_call("leapfrog", [p, q], [p.shape, q.shape], extra=mode)
        if np.ndim(p_old) == 1:
            return pn[0], qn[0]
        return pn, qn

    def E(self, q, p):
        """samplers.py:819-823 (V of utils.py:218 + K of :817) for one row or a batch."""
        qq = np.atleast_2d(np.asarray(q, dtype=np.float64))
        pp = np.atleast_2d(np.asarray(p, dtype=np.float64))
        E, = self._row_call("energy", [qq, pp], [qq.shape[:1]], what="hmc_energy")
        return E[0] if np.ndim(q) == 1 else E

    def K(self, p):
        """samplers.py:811-817 (host; tiny)."""
        return np.dot(p, np.dot(self.inv_cov_p, p)) / 2.

    def p_sample(self):
        """samplers.py:825-829 (host draw from the global legacy RNG, as the reference)."""
        return np.random.multivariate_normal(np.zeros(self.D), self.cov_p, size=1)

    def make_movie(self, title_prefix, q0=None, cov0=None, plot_cov=True, qmin=-3, qmax=3, **kwargs):
        """samplers.py:843-880: PNG deck of chain 0's captured trajectories (hmc_amd.plots)."""
        from . import plots
        return plots.make_movie(self, title_prefix, q0=q0, cov0=cov0, plot_cov=plot_cov, qmin=qmin, qmax=qmax,
                                **kwargs)

    def make_slide(self, title_prefix, idx, phi_q, q_accepted, decision, q0=None, cov0=None, plot_cov=False,
                   qmin=-3, qmax=3):
        """samplers.py:883-924."""
        from . import plots
        return plots.make_slide(title_prefix, idx, phi_q, q_accepted, decision, q0, cov0, plot_cov, qmin, qmax)
