"""CPU model of the per-chain step-size adaptation (include/hmc.h: hmc_adapt), built on the oracle
(oracle/hmc_oracle.py, unchanged) for tests/test_adapt_host.py and tests/test_gpu_glm_adapt.py.

DualAverage restates the update rule in NumPy, independently of csrc/hmc_adapt.hpp.  nuts_adaptive
drives O.gen_sample_nuts one chain and one iteration at a time (Nchain = 1, Niter = 1, warm_up = 0,
thin = 1) with a RecordingCore whose dt is s * dt and a view that maps the call's (chain 0, iteration
1) onto the real (chain, iteration) of the draw source; energies[1] of a call is E_init, energies[2:]
are the tree's points, one per leapfrog.  random_adaptive writes the adaptive loop on HMCCore.leap_frog
/ .E with the row, E_chain, dE_chain and warm-up rules of O.gen_sample_random."""
import numpy as np

import glm_cases as G
from oracle import hmc_oracle as O

GAMMA, T0, KAPPA = 0.05, 10.0, 0.75
CLAMP = 20.0 * np.log(2.0)
SLOTS = ("log_s", "log_s_bar", "H_bar", "m", "mu", "sum_alpha_adapt", "sum_alpha_after", "n_after")


class DualAverage:
    """Hoffman & Gelman 2014, section 3.2, on log s with mu = log(s0); `clamped` records whether an
    update ever reached mu -+ 20 ln 2."""

    def __init__(self, s0=1.0, delta=0.8):
        self.delta = delta
        self.log_s = self.log_s_bar = self.mu = float(np.log(s0))
        self.H_bar = self.m = 0.0
        self.sum_adapt = self.sum_after = self.n_after = 0.0
        self.clamped = False

    def end_iteration(self, alpha, adapting):
        if not adapting:
            self.sum_after += alpha
            self.n_after += 1.0
            return
        self.sum_adapt += alpha
        self.m += 1.0
        m = self.m
        self.H_bar = (1.0 - 1.0 / (m + T0)) * self.H_bar + (self.delta - alpha) / (m + T0)
        raw = self.mu - np.sqrt(m) / GAMMA * self.H_bar
        self.log_s = float(np.clip(raw, self.mu - CLAMP, self.mu + CLAMP))
        self.clamped |= bool(self.log_s != raw)
        eta = m ** (-KAPPA)
        self.log_s_bar = eta * self.log_s + (1.0 - eta) * self.log_s_bar

    def scale(self, adapting):
        return float(np.exp(self.log_s if (adapting or self.m == 0.0) else self.log_s_bar))

    def slots(self):
        return np.array([self.log_s, self.log_s_bar, self.H_bar, self.m, self.mu, self.sum_adapt, self.sum_after,
                         self.n_after])


def point_alpha(E_init, E):
    """min(1, exp(E_init - E)); 0 for an energy, or a difference, that is not finite."""
    dE = E - E_init
    if not np.isfinite(E) or np.isnan(dE):
        return 0.0
    with np.errstate(over="ignore"):
        return float(min(1.0, np.exp(-dE)))


def _finish(out, das):
    out["state"] = np.stack([d.slots() for d in das])
    out["step_scale"] = np.exp(out["state"][:, 1])
    out["clamped"] = any(d.clamped for d in das)
    return out


class _OneIteration:
    """Draw source of one O.gen_sample_nuts call (chain 0, iterations 0 and 1) on the real draws'
    (chain m, iteration i).  The call's iteration-0 momentum only enters energies[0], which is dropped."""

    def __init__(self, draws, m, i, D):
        self.d, self.m, self.i, self.D = draws, m, i, D

    def p(self, m, i):
        return np.zeros(self.D) if i == 0 else self.d.p(self.m, self.i)

    def direction(self, m):
        return self.d.direction(self.m)

    def uniform(self, m):
        return self.d.uniform(self.m)


def nuts_adaptive(target, dt, cov_p, q_start, Niter, warm_up, thin, d_max, draws, adapt_end, delta=0.8, s0=None):
    """The adaptive NUTS run of every chain; O.gen_sample_nuts's result dict (on_dmax="break") plus
    state (N, 8), step_scale (N,), alpha (N, Niter) and clamped."""
    N, D = q_start.shape
    Lc = O.chain_len(Niter, warm_up, thin)
    out = dict(q_chain=np.zeros((N, Lc, D)), E_chain=np.zeros((N, Lc)), dE_chain=np.zeros((N, Lc)),
               alpha=np.zeros((N, Niter)), N_total_steps=0, n_leapfrog=0, n_unstable=0, n_dmax=0)
    s0 = np.broadcast_to(np.ones(N) if s0 is None else np.asarray(s0, float), (N,))
    das = [DualAverage(s0[m], delta) for m in range(N)]
    for m in range(N):
        q = q_start[m]
        out["q_chain"][m, 0] = q
        E_prev = O.HMCCore(target, dt, cov_p).E(q, draws.p(m, 0))
        out["E_chain"][m, 0] = E_prev
        out["N_total_steps"] += 1
        for i in range(1, Niter + 1):
            adapting = i < adapt_end
            core = G.RecordingCore(target, das[m].scale(adapting) * dt, cov_p)
            r = O.gen_sample_nuts(core, q[None, :], 1, 1, 0, 1, d_max, _OneIteration(draws, m, i, D), on_dmax="break")
            E_init, pts = core.energies[1], core.energies[2:]
            assert len(pts) == r["n_leapfrog"] >= 1
            alpha = float(np.mean([point_alpha(E_init, e) for e in pts]))
            out["alpha"][m, i - 1] = alpha
            das[m].end_iteration(alpha, adapting)
            q = r["q_chain"][0, 1]
            for k in ("n_leapfrog", "n_unstable", "n_dmax"):
                out[k] += r[k]
            out["N_total_steps"] += r["N_total_steps"] - 1          # the call's own initial energy
            if i >= warm_up:
                row = (i - warm_up) // thin
                out["E_chain"][m, row] = E_init
                out["dE_chain"][m, row] = E_init - E_prev
                out["q_chain"][m, row] = q
            E_prev = E_init
    return _finish(out, das)


def random_adaptive(target, dt, cov_p, q_start, Niter, warm_up, thin, L_low, L_high, draws, adapt_end, delta=0.8,
                    s0=None):
    """O.gen_sample_random (samplers.py:387-491) with the step of iteration i scaled by the chain's
    multiplier; its result dict plus state, step_scale, alpha, dE_prop (N, Niter) and clamped."""
    N, D = q_start.shape
    Lc = O.chain_len(Niter, warm_up, thin)
    q_chain, E_chain, dE_chain = np.zeros((N, Lc, D)), np.zeros((N, Lc)), np.zeros((N, Lc))
    alpha_all, dE_prop = np.zeros((N, Niter)), np.zeros((N, Niter))
    s0 = np.broadcast_to(np.ones(N) if s0 is None else np.asarray(s0, float), (N,))
    das = [DualAverage(s0[m], delta) for m in range(N)]
    acc = acc_wu = n_total = n_lf = 0
    core = O.HMCCore(target, dt, cov_p)
    for m in range(N):
        q_chain[m, 0] = q_start[m]
        q_tmp = q_start[m]
        E_prev = core.E(q_tmp, draws.p(m, 0))
        n_total += 1
        E_chain[m, 0] = E_prev
        for i in range(1, Niter + 1):
            adapting = i < adapt_end
            core.dt = das[m].scale(adapting) * dt
            q_initial = q_tmp
            p_tmp = draws.p(m, i)
            E_init = core.E(q_tmp, p_tmp)
            n_total += 1
            if i >= warm_up:
                r = (i - warm_up) // thin
                E_chain[m, r] = E_init
                dE_chain[m, r] = E_init - E_prev
            L = draws.L(m, i, L_low, L_high)
            for _ in range(1, L + 1):
                p_tmp, q_tmp = core.leap_frog(p_tmp, q_tmp)
                n_total += L * D
            n_lf += L
            E_final = core.E(q_tmp, p_tmp)
            n_total += 1
            dE = E_final - E_init
            E_prev = E_init
            lnu = draws.lnu(m, i)
            if (dE < 0) or (lnu < -dE):
                if i >= warm_up:
                    q_chain[m, (i - warm_up) // thin] = q_tmp
                    acc += 1
                else:
                    acc_wu += 1
            else:
                r = (i - warm_up) // thin
                assert r >= -Lc
                q_chain[m, r] = q_initial
                q_tmp = q_initial
            alpha_all[m, i - 1] = point_alpha(E_init, E_final)
            dE_prop[m, i - 1] = dE
            das[m].end_iteration(alpha_all[m, i - 1], adapting)
    out = dict(q_chain=q_chain, E_chain=E_chain, dE_chain=dE_chain, N_total_steps=n_total, n_leapfrog=n_lf,
               accept_count=acc, accept_count_warm_up=acc_wu, alpha=alpha_all, dE_prop=dE_prop,
               accept_R=acc / float(N * (Niter - warm_up + 1)),
               accept_R_warm_up=(acc_wu / float(N * warm_up)) if warm_up > 0 else None)
    return _finish(out, das)
