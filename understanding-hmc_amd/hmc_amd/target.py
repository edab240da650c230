"""Multivariate-normal target descriptors for the GPU engine.

The reference hands the sampler two opaque Python closures, V(q) and dVdq(q)
(samplers.py:310-311, :327-328), built by every driver as
    V(q)    = -normal_lnL(q, q0, cov0)          (case1-script.py:39-43, utils.py:213-218)
    dVdq(q) = np.dot(inv_cov0, q - q0)          (case1-script.py:45-49)
The GPU cannot call Python closures, so the engine needs the MVN parameters
explicitly.  Two ways in:
  * `MVNTarget(q0, cov0)` passed as HMC_sampler(..., target=...);
  * `probe_closures(D, V, dVdq)`: affine probing of the closures
    (dVdq(0) and dVdq(e_i) give P = inv(cov0) column by column and q0; V(q0)
    gives the constant), verified at random points before it is trusted.
    For q0 = 0 (every reference driver) the probe is exact to the bit.
Closures that are not MVN are rejected (no CPU fallback exists in the product).

One target that is not MVN has kernels of its own: `MixtureTarget(weights, mus, variances)`,
a mixture of K Gaussians with diagonal covariances (csrc/hmc_mix.hip), passed as
HMC_sampler(D, None, None, ..., target=MixtureTarget(...), sampler_type="Random").
One target is defined by data: `LogisticTarget(X, y, prior_var)`, the posterior of logistic-regression
coefficients under a normal prior (csrc/hmc_logit.hip), passed the same way.
"""
import numpy as np


class MVNTarget:
    """q0 (D,), precision P = inv(cov0) (D, D), constant D*log(2*pi) + log det(cov0)."""

    def __init__(self, q0, cov0=None, prec=None, logdet_const=None):
        self.q0 = np.ascontiguousarray(q0, dtype=np.float64).reshape(-1)
        D = self.q0.size
        if prec is None:
            cov0 = np.asarray(cov0, dtype=np.float64)
            prec = np.linalg.inv(cov0)                     # case1-script.py:36
        self.prec = np.ascontiguousarray(prec, dtype=np.float64)
        if self.prec.shape != (D, D):
            raise AssertionError("precision must be (D, D)")
        if logdet_const is None:
            if cov0 is None:
                cov0 = np.linalg.inv(self.prec)
            # scipy's logpdf constant (utils.py:218): rank*log(2 pi) + log pseudo-det, via eigh
            w = np.linalg.eigvalsh(np.asarray(cov0, dtype=np.float64))
            logdet_const = D * np.log(2 * np.pi) + np.sum(np.log(w))
        self.logdet_const = float(logdet_const)
        off = self.prec - np.diag(np.diag(self.prec))
        self.diagonal = not np.any(off)
        self.identity = self.diagonal and np.all(np.diag(self.prec) == 1.0)
        self.zero_mean = not np.any(self.q0)

    @property
    def D(self):
        return self.q0.size

    def V(self, q):
        x = np.asarray(q, dtype=np.float64) - self.q0
        return 0.5 * (self.logdet_const + x @ self.prec @ x)

    def dVdq(self, q):
        return np.dot(self.prec, np.asarray(q, dtype=np.float64) - self.q0)


class MixtureTarget:
    """Mixture of K Gaussians with diagonal covariances: weights (K,), mus (K, D), variances (K, D).

    V(q) = -log sum_k w_k N(q; mu_k, diag var_k).  The host V / dVdq below (logsumexp, NumPy) serve
    HMC_sampler.V / .dVdq and the plots; the chains run in csrc/hmc_mix.hip from the device
    descriptor's arrays logw, mu, prec = 1/var and logdet_const_k = D log(2 pi) + sum_d log var_kd.
    `q0` is the mixture mean (what the MVN targets call q0: where start points and plots centre)."""

    diagonal = True

    def __init__(self, weights, mus, variances):
        self.w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        self.mu = np.ascontiguousarray(mus, dtype=np.float64)
        self.variances = np.ascontiguousarray(variances, dtype=np.float64)
        K = self.w.size
        if self.mu.ndim != 2 or self.mu.shape[0] != K or self.variances.shape != self.mu.shape or self.mu.shape[1] < 1:
            raise AssertionError("MixtureTarget takes weights (K,), mus (K, D), variances (K, D)")
        if not (np.all(self.w > 0) and abs(self.w.sum() - 1.0) <= 1e-12):
            raise AssertionError("mixture weights must be positive and sum to 1 (within 1e-12)")
        if not np.all(self.variances > 0):
            raise AssertionError("mixture variances must be positive")
        self.logw = np.log(self.w)
        self.prec = 1.0 / self.variances
        self.logdet_const = self.D * np.log(2 * np.pi) + np.sum(np.log(self.variances), axis=1)
        self.q0 = self.mean()

    @property
    def D(self):
        return self.mu.shape[1]

    @property
    def K(self):
        return self.w.size

    def _log_terms(self, q):
        """l_k = log w_k + log N(q; mu_k, diag var_k) and x = q - mu, for q (..., D)."""
        x = np.asarray(q, dtype=np.float64)[..., None, :] - self.mu
        return self.logw - 0.5 * (self.logdet_const + np.sum(self.prec * x * x, axis=-1)), x

    def V(self, q):
        l, _ = self._log_terms(q)
        M = np.max(l, axis=-1)
        return -(M + np.log(np.sum(np.exp(l - M[..., None]), axis=-1)))

    def dVdq(self, q):
        l, x = self._log_terms(q)
        e = np.exp(l - np.max(l, axis=-1, keepdims=True))
        r = e / np.sum(e, axis=-1, keepdims=True)
        return np.sum(r[..., None] * (self.prec * x), axis=-2)

    def mean(self):
        """E[q_d] = sum_k w_k mu_kd."""
        return self.w @ self.mu

    def var(self):
        """Var[q_d] = sum_k w_k (var_kd + mu_kd^2) - mean_d^2."""
        return self.w @ (self.variances + self.mu ** 2) - self.mean() ** 2

    def sample(self, n, rng):
        """n exact draws from a np.random.RandomState (start points, tests)."""
        k = rng.choice(self.K, size=n, p=self.w)
        return self.mu[k] + np.sqrt(self.variances[k]) * rng.standard_normal((n, self.D))


class LogisticTarget:
    """Bayesian logistic regression: design matrix X (n, D), labels y (n,) in {0, 1}, independent
    zero-mean normal prior of variance prior_var (a scalar or (D,)).

    With z = X q and no normalising constants
        V(q)    = sum_j [softplus(z_j) - y_j z_j] + 0.5 sum_d q_d^2 / prior_var_d
        dV/dq   = X^T (sigma(z) - y) + q / prior_var
        softplus(z) = max(z, 0) + log1p(exp(-|z|)),  sigma(z) = 1/(1+e^-z) (z >= 0), e^z/(1+e^z) (z < 0):
    forms that never overflow.  The host V / dVdq below serve HMC_sampler.V / .dVdq and the plots,
    for one row or for batched (..., D) rows; the chains run in csrc/hmc_logit.hip from the device
    descriptor's arrays X, y and prior_prec = 1 / prior_var.  `q0` is the prior mean, zeros(D)
    (what the MVN targets call q0: where start points and plots centre)."""

    diagonal = True

    def __init__(self, X, y, prior_var=1.0):
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.X.ndim != 2 or self.X.shape[0] < 1 or self.X.shape[1] < 1:
            raise AssertionError("LogisticTarget takes X (n, D) with n >= 1 and D >= 1")
        if self.y.shape != (self.X.shape[0],):
            raise AssertionError("LogisticTarget takes y (n,) with one label per row of X")
        if not np.all((self.y == 0.0) | (self.y == 1.0)):
            raise AssertionError("logistic labels must be 0 or 1")
        pv = np.asarray(prior_var, dtype=np.float64)
        if pv.ndim == 0:
            pv = np.full(self.D, float(pv))
        self.prior_var = np.ascontiguousarray(pv)
        if self.prior_var.shape != (self.D,):
            raise AssertionError("prior_var must be a scalar or (D,)")
        if not np.all(self.prior_var > 0):
            raise AssertionError("prior_var must be positive")
        self.prior_prec = 1.0 / self.prior_var
        self.q0 = np.zeros(self.D)

    @property
    def D(self):
        return self.X.shape[1]

    @property
    def n(self):
        return self.X.shape[0]

    def V(self, q):
        q = np.asarray(q, dtype=np.float64)
        z = q @ self.X.T                                            # (..., n)
        softplus = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        return np.sum(softplus - self.y * z, axis=-1) + 0.5 * np.sum(q * q * self.prior_prec, axis=-1)

    def dVdq(self, q):
        q = np.asarray(q, dtype=np.float64)
        z = q @ self.X.T
        t = np.exp(-np.abs(z))
        sigma = np.where(z >= 0, 1.0, t) / (1.0 + t)
        return (sigma - self.y) @ self.X + q * self.prior_prec


class GLMTarget:
    """Posterior of the coefficients q of a generalized linear model: design matrix X (n, D),
    responses y (n,), linear predictor z = X q, and an independent zero-mean normal prior with
    variances prior_var (scalar or (D,)).  No normalising constants:
        family="poisson"    (log link, y = 0, 1, 2, ...)
            V(q)  = sum_j [exp(z_j) - y_j z_j] + 0.5 sum_d q_d^2 / prior_var_d
            dV/dq = X^T (exp(z) - y) + q / prior_var
            exp(z) overflows to inf from z ~ 709.78 on: V is then inf, which the samplers treat as any
            non-finite energy (Random rejects the proposal, NUTS counts the sub-tree unstable)
        family="bernoulli"  (logit link, y in {0, 1}): LogisticTarget's V and dV/dq, the same posterior
    Both samplers run on it: Random through csrc/hmc_logit.hip (the family is a template parameter of
    the logistic kernels), NUTS through csrc/hmc_glm_nuts.hip.  The host V / dVdq below serve
    HMC_sampler.V / .dVdq and the plots, for one row or for batched (..., D) rows.  `q0` is the prior
    mean, zeros(D)."""

    diagonal = True
    FAMILIES = {"bernoulli": 0, "poisson": 1}        # include/hmc.h HMC_GLM_BERNOULLI, HMC_GLM_POISSON

    def __init__(self, X, y, family="poisson", prior_var=1.0):
        if family not in self.FAMILIES:
            raise AssertionError("GLMTarget family must be one of %s" % sorted(self.FAMILIES))
        self.family = family
        self.family_id = self.FAMILIES[family]
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        if self.X.ndim != 2 or self.X.shape[0] < 1 or self.X.shape[1] < 1:
            raise AssertionError("GLMTarget takes X (n, D) with n >= 1 and D >= 1")
        if self.y.shape != (self.X.shape[0],):
            raise AssertionError("GLMTarget takes y (n,) with one response per row of X")
        if family == "bernoulli":
            if not np.all((self.y == 0.0) | (self.y == 1.0)):
                raise AssertionError("bernoulli responses must be 0 or 1")
        elif not (np.all(np.isfinite(self.y)) and np.all(self.y >= 0.0) and np.all(self.y == np.floor(self.y))):
            raise AssertionError("poisson responses must be non-negative integers")
        pv = np.asarray(prior_var, dtype=np.float64)
        if pv.ndim == 0:
            pv = np.full(self.D, float(pv))
        self.prior_var = np.ascontiguousarray(pv)
        if self.prior_var.shape != (self.D,):
            raise AssertionError("prior_var must be a scalar or (D,)")
        if not np.all(self.prior_var > 0):
            raise AssertionError("prior_var must be positive")
        self.prior_prec = 1.0 / self.prior_var
        self.q0 = np.zeros(self.D)

    @property
    def D(self):
        return self.X.shape[1]

    @property
    def n(self):
        return self.X.shape[0]

    def V(self, q):
        q = np.asarray(q, dtype=np.float64)
        z = q @ self.X.T                                            # (..., n)
        with np.errstate(over="ignore"):
            if self.family == "poisson":
                nll = np.exp(z)                                     # inf past ~709.78: V = inf
            else:
                nll = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
        return np.sum(nll - self.y * z, axis=-1) + 0.5 * np.sum(q * q * self.prior_prec, axis=-1)

    def dVdq(self, q):
        q = np.asarray(q, dtype=np.float64)
        z = q @ self.X.T
        with np.errstate(over="ignore"):
            if self.family == "poisson":
                mean = np.exp(z)
            else:
                t = np.exp(-np.abs(z))
                mean = np.where(z >= 0, 1.0, t) / (1.0 + t)
        return (mean - self.y) @ self.X + q * self.prior_prec


def probe_closures(D, V, dVdq, n_check=4, rtol=1e-9, seed=12345):
    """Recover an MVNTarget from the reference-style closures by affine probing."""
    z = np.zeros(D)
    g0 = np.asarray(dVdq(z), dtype=np.float64).reshape(-1)
    if g0.size != D:
        raise AssertionError("dVdq must return a length-D vector")
    cols = np.empty((D, D))
    for i in range(D):
        e = np.zeros(D)
        e[i] = 1.0
        cols[:, i] = np.asarray(dVdq(e), dtype=np.float64).reshape(-1) - g0
    P = cols
    if not np.any(g0):
        q0 = np.zeros(D)
    else:
        q0 = -np.linalg.solve(P, g0)
    logc = 2.0 * float(V(q0))
    t = MVNTarget(q0, prec=P, logdet_const=logc)
    rng = np.random.RandomState(seed)           # private stream: never touches the global np.random
    for _ in range(n_check):
        x = q0 + rng.standard_normal(D) * 1.7
        g_ref = np.asarray(dVdq(x), dtype=np.float64).reshape(-1)
        g = t.dVdq(x)
        if not np.allclose(g, g_ref, rtol=rtol, atol=rtol * (1 + np.abs(g_ref).max())):
            raise NotImplementedError("dVdq is not affine: the GPU engine supports multivariate-normal "
                                      "targets only (pass target=MVNTarget(q0, cov0))")
        v_ref = float(V(x))
        if not np.isclose(t.V(x), v_ref, rtol=rtol, atol=rtol * (1 + abs(v_ref))):
            raise NotImplementedError("V is not the MVN potential matching dVdq (pass target=MVNTarget)")
    return t
