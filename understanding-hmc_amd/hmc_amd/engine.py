"""Device-resident chain batch: buffers + C-ABI calls for the Random-trajectory sampler.

`RandomEngine` owns the (Nchain x D) state and the output arrays as torch CUDA
tensors (memory/streams only — all arithmetic is in libhmc.so) and exposes the
two calls of the hot path: `init()` (samplers.py:413-420) and `run(it0, it1)`
(iterations of samplers.py:428-475, fused in one kernel launch).  HMC_sampler
and bench.py are both thin layers over it.
"""
import hashlib
import json

import numpy as np
import torch

from . import _lib as H
from . import descriptors as Dsc
from .descriptors import dev_tensor as _dev
from .target import GLMTarget, LogisticTarget, MixtureTarget


class RandomEngine:
    def __init__(self, target, n_chains, n_iter, warm_up, thin, L_low, L_high, dt, cov_p=None, rng="philox",
                 seed=0, fp_mode="fast", chain_offset=0, store_chain=True, store_energy=True, n_save=0,
                 device=None, dense=False, order_tiles=True, random_ws=True):
        self.t = target
        self.D = D = target.D
        self.N = int(n_chains)
        self.n_iter, self.warm_up, self.thin = int(n_iter), int(warm_up), int(thin)
        self.L_chain = 1 + (self.n_iter - self.warm_up) // self.thin
        self.L_low, self.L_high = int(L_low), int(L_high)
        self.rng, self.seed, self.fp_mode = rng, int(seed), fp_mode
        self.chain_offset = int(chain_offset)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        kind = self._descriptors(target, cov_p, dt, dense)
        # ---- state and outputs
        N, Lc = self.N, self.L_chain
        self.q = torch.zeros((N, D), dtype=torch.float64, device=dev)
        self.E_prev = torch.zeros(N, dtype=torch.float64, device=dev)
        self.q_chain = torch.zeros((N, Lc, D), dtype=torch.float64, device=dev) if store_chain else None
        self.E_chain = torch.zeros((N, Lc), dtype=torch.float64, device=dev) if store_energy else None
        self.dE_chain = torch.zeros((N, Lc), dtype=torch.float64, device=dev) if store_energy else None
        self.counters = torch.zeros((H.COUNTER_SLOTS, H.NCOUNTERS), dtype=torch.int64, device=dev)
        self.n_save = int(n_save)
        if self.n_save:
            self.traj_stride = max(self.L_high, 1)
            self.traj = torch.zeros((self.n_save, self.traj_stride, 2), dtype=torch.float64, device=dev)
            self.traj_len = torch.zeros(self.n_save, dtype=torch.int32, device=dev)
            self.decision = torch.zeros(self.n_save, dtype=torch.int32, device=dev)
        else:
            self.traj_stride, self.traj, self.traj_len, self.decision = 0, None, None, None
        self.S = H.State(H.ptr(self.q), H.ptr(self.E_prev), H.ptr(self.q_chain), H.ptr(self.E_chain),
                         H.ptr(self.dE_chain), H.ptr(self.counters), H.ptr(self.traj), H.ptr(self.traj_len),
                         H.ptr(self.decision), self.n_save, self.traj_stride)
        self._alloc_workspace(kind, order_tiles, random_ws)
        self._replay = None
        self._streams = []

    def _descriptors(self, target, cov_p, dt, dense):
        """Target / kinetic descriptors self.T, self.K (their device arrays kept alive on the
        object); returns the target kind."""
        mvn, kin = Dsc.host_descriptors(target, cov_p, dt, dense, chol=True)
        self.T, self._target_keep = Dsc.upload_mvn(target, mvn, self.device)
        self._kinetic(cov_p, dt, kin)
        return mvn.kind

    def _kinetic(self, cov_p, dt, kin):
        """self.K from the host arrays `kin`, and the values of cov_p and dt a checkpoint records."""
        self.cov_p, self.dt = Dsc.host_cov_p(cov_p, self.D), np.asarray(dt, dtype=np.float64)
        self.K, self._kinetic_keep = Dsc.upload_kinetic(kin, self.device)
        self._full_mass = kin.minv_full is not None

    @staticmethod
    def _large_d(kind, D):
        """The route's large-D rule (csrc/hmc_route.cpp big_path, RandomKernel::Big), restated: dense
        D > 128 (no MFMA tile layout), diagonal D > 2048 (more than 16 coordinate pairs per lane of
        a wave)."""
        return D > 128 if kind == H.HMC_TARGET_DENSE else (D + 1) // 2 > 16 * 64

    def _alloc_workspace(self, kind, order_tiles, random_ws):
        D = self.D
        # dense targets: scratch for L-ordered MFMA tiles (chains sorted by trajectory length
        # every iteration; same results, no lane idling through a longer trajectory).  The large-D
        # path (dense D > 128, diagonal D > 2048) keeps its chain state there: always allocated (a
        # NUTS run only needs it for hmc_chain_init's start energies, random_ws=False: sized for the
        # init alone, i.e. without the full-cov_p products unless cov_p is full)
        L_ = H.lib()
        if self._large_d(kind, D):
            nbytes = L_.hmc_random_workspace_size_ex(self.T, self.K, self.N)
        elif order_tiles and random_ws:
            nbytes = L_.hmc_random_workspace_size(self.T, self.N)
        else:
            nbytes = 0
        self._order = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=self.device) if nbytes > 0 else None
        self._order_bytes = self._order.numel() * 4 if self._order is not None else 0
        self.S.order = H.ptr(self._order)

    def set_chain_window(self, window, row0):
        """Store q_chain rows [row0, row0 + window.shape[1]) into `window` (N, W, D) instead of a
        whole-chain array (streaming diagnostics); other rows are not stored."""
        assert window.shape[0] == self.N and window.shape[2] == self.D and window.is_contiguous()
        self._window = window
        self.S.q_chain = window.data_ptr()
        self.S.qc_rows = window.shape[1]
        self.S.qc_row0 = int(row0)

    def set_replay(self, p0, P, Ls, lnu):
        """Host-replayed draws (rng='replay'): p0 (N,D), p (N,Niter,D), L (N,Niter), log u (N,Niter).
        L must lie in [L_low, L_high), the range np.random.randint draws it from (samplers.py:441):
        the kernels size trajectories (and the large-D path its launch count) by L_high."""
        Ls = np.asarray(Ls)
        if Ls.size and (Ls.min() < self.L_low or Ls.max() >= self.L_high):
            raise AssertionError("replay tape L outside [L_low, L_high) = [%d, %d)" % (self.L_low, self.L_high))
        dev = self.device
        self._streams = [_dev(p0, dev), _dev(P, dev), _dev(Ls, dev, torch.int32), _dev(lnu, dev)]
        self._replay = H.Replay(*[H.ptr(x) for x in self._streams], None, 0)

    d_max, on_dmax = 10, 0

    def schedule(self, it0, it1):
        return H.Schedule(self.N, self.chain_offset, self.n_iter, self.warm_up, self.thin, self.L_chain,
                          self.L_low, self.L_high, it0, it1,
                          H.HMC_RNG_REPLAY if self.rng == "replay" else H.HMC_RNG_PHILOX,
                          H.HMC_MODE_EXACT if self.fp_mode == "exact" else H.HMC_MODE_FAST, self.d_max,
                          self.on_dmax, self.seed)

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _init_call(self):
        """init()'s C entry, its name in error messages, and its arguments between the state and
        the stream."""
        return "hmc_chain_init_ws", "hmc_chain_init", (self._order_bytes,)

    def init(self, q_start):
        qs = q_start if isinstance(q_start, torch.Tensor) else _dev(np.asarray(q_start).reshape(self.N, self.D),
                                                                    self.device)
        self._qs = qs.to(self.device, torch.float64).contiguous()
        entry, what, tail = self._init_call()
        H.check(getattr(H.lib(), entry)(self.T, self.K, self.schedule(1, 1), self._replay, H.ptr(self._qs), self.S,
                                        *tail, self.stream()), what)

    def run(self, it0, it1):
        """Iterations [it0, it1) of every chain in ONE fused kernel launch."""
        H.check(H.lib().hmc_random_iters_ws(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                            self._order_bytes, self.stream()), "hmc_random_iters")

    def run_streaming(self, diag, it_begin, it_end, step, events=None, feed=None):
        """Iterations [it_begin, it_end) in launches of `step`, with q_chain rows kept only in a
        circular device window (chain row r in window row r % W) that feeds `diag`
        (diagnostics.StreamingDiagnostics): memory O(N * (tmax + step/thin) * D) instead of
        O(N * L_chain * D), no copies.  Row 0 is not a sample of the statistics (Q16); rows are
        fed once complete (a thinned row is final after its last iteration).  May be called
        repeatedly with consecutive ranges and the same `step`.
        events: optional (start, end) CUDA events recorded around each sampler launch.
        feed: iterations between diagnostics updates (default `step`; a multiple of `step`).  Each
        update re-reads the last tmax rows (variogram carry), so feeding fewer, larger windows
        cuts the diagnostics' HBM traffic per sample from (rows + tmax + 12)/rows toward 1 row,
        for a window of tmax + (feed + step)/thin rows.  The last iteration always flushes."""
        N, D, T = self.N, self.D, diag.tmax
        feed = step if feed is None else int(feed)
        assert feed >= step and feed % step == 0, "feed must be a multiple of step"
        # exact mode (every lag of the reference's ESS loop) whenever a whole split half fits in no
        # more window than the segment mode would use: each half is fed once complete, from a
        # window of n + ceil(step/thin) + 2 rows; otherwise segments of `feed` iterations
        exact = diag.mode == "exact" or (diag.mode is None and diag.n <= T + feed // self.thin)
        W_seg = T + (feed + step) // self.thin + 2
        if exact:
            # both halves whole in the window (rows 1 .. 2n at slots 1 .. 2n: no half wraps, so the
            # lag pass reads plain strided rows) when that costs no more than the segment mode;
            # otherwise one half + a launch's rows, the second half wrapping
            W2 = 2 * diag.n + -(-step // self.thin) + 2
            W = W2 if W2 <= W_seg else diag.n + -(-step // self.thin) + 2
        else:
            W = W_seg
        # the mode and the window size are decided by the first call and recorded in `diag` (and
        # so in a checkpoint): a later call, or a resumed run, with another step or feed would
        # otherwise pick another mode or window size, and rows already written (the open half, the
        # variogram carry) would be silently replaced by a zeroed window (advisor r05)
        if diag.mode is None:
            diag._set_mode("exact" if exact else "stream")
            # the envelope of the exact mode for this feed: halves of n <= tmax + feed/thin samples
            diag.exact_max_samples = 2 * (T + feed // self.thin) + 1
        if diag.window_rows is not None and diag.window_rows != W:
            raise AssertionError("run_streaming continued with step/feed giving a %d-row window; the "
                                 "statistics' window has %d rows (use the same step and feed)" % (W, diag.window_rows))
        diag.window_rows = W
        st = getattr(self, "_stream", None)
        if st is None or st[0] is not diag or st[1].shape[1] != W:
            st = [diag, torch.zeros((N, W, D), dtype=torch.float64, device=self.device)]
            self._stream = st
        win = st[1]
        self.set_chain_window(win, 1)
        next_row = 1 + diag.pos            # next chain row the statistics need
        for a in range(it_begin, it_end, step):
            b = min(a + step, it_end)
            if events is not None:
                events[0].record(torch.cuda.current_stream(self.device))
            self.run(a, b)
            if events is not None:
                events[1].record(torch.cuda.current_stream(self.device))
            done = self.L_chain if b - 1 == self.n_iter else max(0, (b - self.warm_up) // self.thin)
            if exact:
                # split half h = chain rows 1 + h n .. (h + 1) n, whole in the window once complete
                h = len(diag.halves)
                while h < 2 and done >= 1 + (h + 1) * diag.n:
                    diag.add_half(win, h, (1 + h * diag.n) % W)
                    h += 1
                continue
            if done > next_row and (done - next_row >= feed // self.thin or b - 1 == self.n_iter):
                carry = min(T, next_row - 1)
                diag.update(win, carry, done - next_row, slot0=(next_row - carry) % W)
                next_row = done
        self.S.q_chain = H.ptr(self.q_chain)
        self.S.qc_rows = 0
        self.S.qc_row0 = 0

    # ---------------------------------------------------------------- checkpoint / resume
    def _target_arrays(self):
        return (self.t.q0, self.t.prec, np.float64(self.t.logdet_const))

    def _meta(self):
        """Everything that decides the chain's next values: a checkpoint restores only into an
        engine with the same schedule, step size, mass matrix and target."""
        return dict(kind=type(self).__name__, N=self.N, D=self.D, n_iter=self.n_iter, warm_up=self.warm_up,
                    thin=self.thin, L_chain=self.L_chain, L_low=self.L_low, L_high=self.L_high, seed=self.seed,
                    rng=self.rng, fp_mode=self.fp_mode, chain_offset=self.chain_offset, d_max=self.d_max,
                    order_tiles=self._order is not None,
                    dt=np.asarray(self.dt, dtype=np.float64).ravel().tolist(),
                    cov_p_sha256=hashlib.sha256(np.ascontiguousarray(self.cov_p, np.float64).tobytes()).hexdigest(),
                    target_sha256=Dsc.fingerprint(self._target_arrays()))

    def save(self, path, it_next, include_chain=True, diag=None):
        """Checkpoint after iteration it_next - 1 (.npz, no pickles).  Philox draws are keyed by
        (seed, global chain, iteration), so a run resumed from it_next reproduces the
        uninterrupted run bit for bit."""
        torch.cuda.synchronize(self.device)
        arr = dict(q=self.q, E_prev=self.E_prev, counters=self.counters)
        if include_chain and self.q_chain is not None:
            arr["q_chain"] = self.q_chain
        if self.E_chain is not None:
            arr["E_chain"], arr["dE_chain"] = self.E_chain, self.dE_chain
        if getattr(self, "ws", None) is not None:
            arr["ws"] = self.ws
        if getattr(self, "adapt_state", None) is not None:
            arr["adapt_state"] = self.adapt_state           # GLM engines: step-size adaptation state
        if self._order is not None:
            arr["order_ws"] = self._order                   # dense: tile order + gradient cache of q
        if diag is not None:
            if diag.mode == "exact":
                if diag.xsums is not None:
                    arr.update(diag_xsums=diag.xsums, diag_xshift=diag.xshift)
            else:
                arr.update(diag_shift=diag.shift, diag_s1=diag.s1, diag_s2=diag.s2, diag_vsum=diag.vsum)
            st = getattr(self, "_stream", None)
            if st is not None and st[0] is diag:
                arr["window"] = st[1]                       # rows of an open half / the lag carry
        meta = dict(self._meta(), it_next=int(it_next), diag_pos=None if diag is None else diag.pos,
                    diag_mode=None if diag is None else diag.mode,
                    diag_window_rows=None if diag is None else diag.window_rows,
                    diag_exact_max_samples=None if diag is None else diag.exact_max_samples,
                    diag_halves=None if diag is None else list(diag.halves))
        np.savez(path, meta=np.array(json.dumps(meta)), **{k: v.cpu().numpy() for k, v in arr.items()})

    def restore(self, path, diag=None):
        """Load a checkpoint written by save() into this (identically configured) engine;
        returns the iteration to continue from."""
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            mine = self._meta()
            bad = {k: (meta.get(k), v) for k, v in mine.items() if meta.get(k) != v}
            if bad:
                raise AssertionError(f"checkpoint does not match this engine: {bad}")
            for k, t in (("q", self.q), ("E_prev", self.E_prev), ("counters", self.counters),
                         ("q_chain", self.q_chain), ("E_chain", self.E_chain), ("dE_chain", self.dE_chain),
                         ("ws", getattr(self, "ws", None)), ("adapt_state", getattr(self, "adapt_state", None)),
                         ("order_ws", self._order)):
                if t is not None and k in z.files:
                    t.copy_(torch.as_tensor(z[k]).to(self.device))
            if self._order is not None and "order_ws" not in z.files:
                self._order.zero_()                         # no cached gradient: recomputed from q
            if diag is not None:
                diag.mode = meta.get("diag_mode")
                diag.window_rows = meta.get("diag_window_rows")
                diag.exact_max_samples = meta.get("diag_exact_max_samples")
                diag.halves = list(meta.get("diag_halves") or [])
                if diag.mode == "exact":
                    if "diag_xsums" in z.files:
                        diag.xsums = torch.as_tensor(z["diag_xsums"]).to(self.device)
                        diag.xshift = torch.as_tensor(z["diag_xshift"]).to(self.device)
                elif "diag_shift" in z.files:
                    for k, t in (("diag_shift", diag.shift), ("diag_s1", diag.s1), ("diag_s2", diag.s2),
                                 ("diag_vsum", diag.vsum)):
                        t.copy_(torch.as_tensor(z[k]).to(self.device))
                diag.pos = int(meta["diag_pos"])
                if "window" in z.files:
                    self._stream = [diag, torch.as_tensor(z["window"]).to(self.device)]
        return int(meta["it_next"])

    def read_counters(self):
        return self.counters.cpu().numpy().astype(np.int64).sum(axis=0)


class _KernelTargetEngine(RandomEngine):
    """What the engines of the targets with kernels of their own share (MixtureEngine,
    LogisticEngine, GLMEngine): RandomEngine's surface, state and outputs, a target descriptor of
    their own in place of the MVN one, a diagonal cov_p only, no workspace, and a pair of C entries
    that take that descriptor: all of it read from the target's row of KERNEL_TARGETS (`self.row`).
    `fp_mode` is accepted and changes nothing (one arithmetic: exp / log cannot be bit-identical to
    NumPy's)."""

    def __init__(self, target, n_chains, n_iter, warm_up, thin, L_low, L_high, dt, cov_p=None, rng="philox",
                 seed=0, fp_mode="fast", chain_offset=0, store_chain=True, store_energy=True, n_save=0,
                 device=None):
        super().__init__(target, n_chains, n_iter, warm_up, thin, L_low, L_high, dt, cov_p=cov_p, rng=rng, seed=seed,
                         fp_mode=fp_mode, chain_offset=chain_offset, store_chain=store_chain,
                         store_energy=store_energy, n_save=n_save, device=device)

    @classmethod
    def check_supported(cls, target, cov_p):
        """NotImplementedError, before anything touches the device, for what the kernels do not take."""
        row = kernel_target(target)
        row.check(target)
        if cov_p is not None and Dsc.full_mass(np.asarray(cov_p, dtype=np.float64)):
            raise NotImplementedError("%s kernels: a full cov_p is not supported (diagonal only)" % row.name)

    def _descriptors(self, target, cov_p, dt, dense):
        self.check_supported(target, cov_p)
        self.row = kernel_target(target)
        assert isinstance(self, self.row.engine), "%s does not run %s targets" % (type(self).__name__, self.row.name)
        self.T, self._target_keep = self.row.upload(target, self.device)
        self._kinetic(cov_p, dt, Dsc.host_kinetic(self.D, cov_p, dt))
        return None

    def _target_arrays(self):
        return self.row.fingerprint_arrays(self.t)

    def _alloc_workspace(self, kind, order_tiles, random_ws):
        self._order, self._order_bytes = None, 0        # hmc_state.order is ignored by these calls

    def _init_call(self):
        return self.row.init, self.row.init, ()

    def run(self, it0, it1):
        """Iterations [it0, it1) of every chain in ONE fused kernel launch."""
        H.check(getattr(H.lib(), self.row.iters)(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                                 self.stream()), self.row.iters)


class MixtureEngine(_KernelTargetEngine):
    """Chain batch of the Random-trajectory sampler on a MixtureTarget (hmc_mix_chain_init /
    hmc_mix_random_iters, csrc/hmc_mix.hip): RandomEngine's surface, state and outputs, with the
    mixture descriptor in place of the MVN one.  Diagonal cov_p only, D <= 512, K <= 8; `fp_mode`
    is accepted and changes nothing (one arithmetic: exp / log cannot be bit-identical to NumPy's)."""


class LogisticEngine(_KernelTargetEngine):
    """Chain batch of the Random-trajectory sampler on a LogisticTarget (hmc_logit_chain_init /
    hmc_logit_random_iters, csrc/hmc_logit.hip: 16 chains per wave, both products of the gradient
    on the f64 matrix cores).  Diagonal cov_p only, D <= 128, n <= 2^20; `fp_mode` is accepted and
    changes nothing.  A checkpoint fingerprints the data (X, y, 1 / prior_var)."""


class GLMEngine(_KernelTargetEngine):
    """Chain batch of the Random-trajectory sampler on a GLMTarget (hmc_glm_chain_init /
    hmc_glm_random_iters: the logistic kernels of csrc/hmc_logit.hip with the family as a template
    parameter).  LogisticEngine's limits: diagonal cov_p only, D <= 128, n <= 2^20; `fp_mode` is
    accepted and changes nothing.  A checkpoint fingerprints the data and the family."""

    def __init__(self, *args, adapt_step=False, adapt_delta=0.8, step_scale0=None, **kw):
        """adapt_step: every chain adapts a multiplier of `dt` during warm-up (iterations
        1 <= i < warm_up) by dual averaging towards a mean acceptance statistic adapt_delta, and runs
        at the averaged multiplier afterwards.  step_scale0: the multipliers to start from, a scalar
        or (N,) (default 1); without adapt_step they stay as given.  Either makes run() call the
        hmc_*_adapt entry with the (N, 8) state `adapt_state` (include/hmc.h: hmc_adapt), which
        save() / restore() carry."""
        super().__init__(*args, **kw)
        self._setup_adapt(adapt_step, adapt_delta, step_scale0)

    def _setup_adapt(self, adapt_step, adapt_delta, step_scale0):
        self.adapt_step, self.adapt_delta = bool(adapt_step), float(adapt_delta)
        self.adapt_state = self._adapt = self._s0 = None
        if not (adapt_step or step_scale0 is not None):
            return
        if not 0.0 < self.adapt_delta < 1.0:
            raise AssertionError("adapt_delta=%r: the target acceptance statistic lies in (0, 1)" % (adapt_delta,))
        if step_scale0 is not None:
            s0 = np.broadcast_to(np.asarray(step_scale0, dtype=np.float64), (self.N,))
            if not np.all(np.isfinite(s0) & (s0 > 0)):
                raise AssertionError("step_scale0 must be positive and finite")
            self._s0 = _dev(s0, self.device)
        if self.N == 0:
            return
        self.adapt_state = torch.zeros((self.N, H.ADAPT_STRIDE), dtype=torch.float64, device=self.device)
        H.check(H.lib().hmc_adapt_init(H.ptr(self.adapt_state), self.N, H.ptr(self._s0), self.stream()),
                "hmc_adapt_init")
        # Hoffman & Gelman's gamma, t0, kappa; adapt_end = warm_up: the reference's warm-up iterations
        self._adapt = H.Adapt(H.ptr(self.adapt_state), self.warm_up if self.adapt_step else 0, self.adapt_delta,
                              0.05, 10.0, 0.75)

    @property
    def step_scale(self):
        """(N,) device tensor of the adapted multipliers exp(log_s_bar); None without adaptation."""
        return None if self.adapt_state is None else torch.exp(self.adapt_state[:, H.ADAPT_LOG_S_BAR])

    def _meta(self):
        meta = super()._meta()
        if self.adapt_state is not None:       # a checkpoint of an adaptive run resumes only into one
            meta.update(adapt_step=self.adapt_step, adapt_delta=self.adapt_delta)
        return meta

    def restore(self, path, diag=None):
        with np.load(path, allow_pickle=False) as z:
            saved = "adapt_state" in z.files
        if saved != (self.adapt_state is not None):
            raise AssertionError("checkpoint %s a step-size adaptation state, this engine %s"
                                 % (("has", "runs without one") if saved else ("has no", "needs one")))
        return super().restore(path, diag)

    def run(self, it0, it1):
        """Iterations [it0, it1) of every chain in ONE fused kernel launch."""
        if self._adapt is None:
            return super().run(it0, it1)
        H.check(H.lib().hmc_glm_random_iters_adapt(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                                   self._adapt, self.stream()), "hmc_glm_random_iters_adapt")


class _NutsSurface:
    """What the NUTS engines share on top of their Random base: the tree's depth limit and what
    happens at it (`d_max`, `on_dmax`), the replay tape in place of (L, log u), and the tree
    workspace `ws`, allocated zeroed from the engine's size query, which stays on the device."""

    def _nuts_setup(self, d_max, on_dmax):
        assert on_dmax in ("raise", "break")
        self.d_max = int(d_max)
        self.on_dmax = 0 if on_dmax == "raise" else 1

    def _alloc_ws(self, nbytes):
        self.ws = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=self.device)

    def set_replay(self, p0, P, tape):
        """Host-replayed draws: p0 (N,D), p (N,Niter,D), tape (N,T) directions/uniforms in order."""
        dev = self.device
        tape = np.ascontiguousarray(tape, dtype=np.float64)
        self._streams = [_dev(p0, dev), _dev(P, dev), _dev(tape, dev)]
        self._replay = H.Replay(H.ptr(self._streams[0]), H.ptr(self._streams[1]), None, None,
                                H.ptr(self._streams[2]), tape.shape[1])


class GLMNutsEngine(_NutsSurface, GLMEngine):
    """Chain batch of the No-U-Turn sampler on a GLMTarget (hmc_glm_nuts_iters, csrc/hmc_glm_nuts.hip:
    one wave steps a tile of 16 chains, each its own tree).  NutsEngine's surface: `d_max`, `on_dmax`,
    `set_replay(p0, P, tape)`, `run(it0, it1)`; the workspace holds the tree vectors of every chain,
    then the replay-tape cursors.  `init()` is GLMEngine's (hmc_glm_chain_init serves both samplers)."""

    def __init__(self, target, n_chains, n_iter, warm_up, thin, d_max, dt, cov_p=None, rng="philox", seed=0,
                 fp_mode="fast", chain_offset=0, store_chain=True, store_energy=True, on_dmax="raise",
                 device=None, iters_per_call=None, adapt_step=False, adapt_delta=0.8, step_scale0=None):
        super().__init__(target, n_chains, n_iter, warm_up, thin, 5, 20, dt, cov_p=cov_p, rng=rng, seed=seed,
                         fp_mode=fp_mode, chain_offset=chain_offset, store_chain=store_chain,
                         store_energy=store_energy, n_save=0, device=device, adapt_step=adapt_step,
                         adapt_delta=adapt_delta, step_scale0=step_scale0)
        self._nuts_setup(d_max, on_dmax)
        nbytes = H.lib().hmc_glm_nuts_workspace_size(self.D, self.N, self.d_max)
        if nbytes <= 0 and self.N > 0:
            raise NotImplementedError("GLM NUTS kernel: d_max=%d not supported (1 <= d_max <= 30)" % self.d_max)
        self._alloc_ws(nbytes)

    def run(self, it0, it1):
        """Iterations [it0, it1) of every chain in one launch."""
        if self._adapt is not None:
            H.check(H.lib().hmc_glm_nuts_iters_adapt(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                                     H.ptr(self.ws), self.ws.numel() * 8, self._adapt,
                                                     self.stream()), "hmc_glm_nuts_iters_adapt")
            return
        H.check(H.lib().hmc_glm_nuts_iters(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                           H.ptr(self.ws), self.ws.numel() * 8, self.stream()), "hmc_glm_nuts_iters")


class NutsEngine(_NutsSurface, RandomEngine):
    """Chain batch of the No-U-Turn sampler (samplers.py:495-808) on the dense-precision
    MFMA kernel (hmc_nuts_iters).  Diagonal targets are passed as dense precisions.
    `run(it0, it1)` advances every chain through iterations [it0, it1) in one launch; the
    tree workspace (live points, both ends, d_max+1 save slots per chain) stays on the device."""

    def __init__(self, target, n_chains, n_iter, warm_up, thin, d_max, dt, cov_p=None, rng="philox", seed=0,
                 fp_mode="fast", chain_offset=0, store_chain=True, store_energy=True, on_dmax="raise",
                 device=None, iters_per_call=None):
        # order_tiles=False: the NUTS kernel uses neither the tile order nor the gradient cache
        super().__init__(target, n_chains, n_iter, warm_up, thin, 5, 20, dt, cov_p=cov_p, rng=rng, seed=seed,
                         fp_mode=fp_mode, chain_offset=chain_offset, store_chain=store_chain,
                         store_energy=store_energy, n_save=0, device=device, dense=True, order_tiles=False,
                         random_ws=False)
        self._nuts_setup(d_max, on_dmax)
        # the Philox momenta drawn ahead are sized for the longest run() call (at most 32 iterations
        # are drawn per launch); replay tapes and a full cov_p draw in the kernel and need none
        self.iters_per_call = int(iters_per_call or n_iter)
        philox_mom = int(rng == "philox" and not self._full_mass)
        nbytes = H.lib().hmc_nuts_workspace_size_ex(self.D, self.N, self.d_max, max(1, self.iters_per_call),
                                                    philox_mom)
        if nbytes <= 0:
            raise NotImplementedError("NUTS kernel: d_max=%d not supported (1 <= d_max <= 30)" % self.d_max)
        self._alloc_ws(nbytes)

    def run(self, it0, it1):
        if it1 - it0 > self.iters_per_call:
            raise ValueError("NutsEngine.run: %d iterations in one call, the workspace is sized for %d "
                             "(iters_per_call)" % (it1 - it0, self.iters_per_call))
        # the sized entry checks the workspace against what this call needs (include/hmc.h)
        H.check(H.lib().hmc_nuts_iters_ws(self.T, self.K, self.schedule(it0, it1), self._replay, self.S,
                                          H.ptr(self.ws), self.ws.numel() * 8, self.stream()), "hmc_nuts_iters_ws")


# Targets that are not MVN and have kernels of their own (descriptors.KernelTarget): the one place
# that lists a target's arrays, for the device descriptor and for the checkpoint fingerprint alike.
_GLM_LIMITS = (("D", H.LOGIT_MAX_D), ("n", H.LOGIT_MAX_N))
_GLM_HEAD = lambda t: (t.D, t.n, t.D)       # noqa: E731  (D, n, ldx)
KERNEL_TARGETS = {
    MixtureTarget: Dsc.KernelTarget(
        "mixture", ("logw", "mu", "prec", "logdet_const"), (), H.Mixture, lambda t: (t.D, t.K),
        (("D", H.MIX_MAX_D), ("K", H.MIX_MAX_COMPONENTS)),
        "hmc_mix_chain_init", "hmc_mix_random_iters", "hmc_mix_leapfrog", "hmc_mix_energy", MixtureEngine, None),
    LogisticTarget: Dsc.KernelTarget(
        "logistic", ("X", "y", "prior_prec"), (), H.Logistic, _GLM_HEAD, _GLM_LIMITS,
        "hmc_logit_chain_init", "hmc_logit_random_iters", "hmc_logit_leapfrog", "hmc_logit_energy",
        LogisticEngine, None),
    GLMTarget: Dsc.KernelTarget(
        "GLM", ("X", "y", "prior_prec"), ("family_id",), H.GLM, _GLM_HEAD, _GLM_LIMITS,
        "hmc_glm_chain_init", "hmc_glm_random_iters", "hmc_glm_leapfrog", "hmc_glm_energy", GLMEngine,
        GLMNutsEngine),
}


def kernel_target(target):
    """The KERNEL_TARGETS row of `target`; None for an MVN target."""
    return next((row for cls, row in KERNEL_TARGETS.items() if isinstance(target, cls)), None)
