"""Shared inputs of the GLM tests (tests/test_gpu_glm.py, tests/test_gpu_glm_nuts.py): the oracle
target, written here from the formulas of include/hmc.h and independently of hmc_amd.target, and the
input recipe.  oracle/hmc_oracle.py's HMCCore, gen_sample_random and gen_sample_nuts run the oracle
target unchanged.

    poisson    V(q) = sum_j [exp(z_j) - y_j z_j] + 0.5 sum_d q_d^2 / prior_var_d,   z = X q
               dV/dq = X^T (exp(z) - y) + q / prior_var
    bernoulli  V(q) = sum_j [softplus(z_j) - y_j z_j] + ...,  dV/dq = X^T (sigma(z) - y) + ...

Every input of a case is drawn from one RandomState(seed), in a fixed order (recipe)."""
import numpy as np

from oracle import hmc_oracle as O


class OracleGLM:
    def __init__(self, X, y, pv, family):
        self.X, self.y, self.pv = np.asarray(X, float), np.asarray(y, float), np.asarray(pv, float)
        self.family = family
        self.q0 = np.zeros(self.X.shape[1])          # HMCCore reads the dimension from q0

    def V(self, q):
        z = self.X @ q
        with np.errstate(over="ignore", invalid="ignore"):
            if self.family == "poisson":
                nll = np.exp(z)
            else:
                nll = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
            return np.sum(nll - self.y * z) + 0.5 * np.sum(q * q / self.pv)

    def dVdq(self, q):
        z = self.X @ q
        with np.errstate(over="ignore", invalid="ignore"):
            if self.family == "poisson":
                mean = np.exp(z)
            else:
                t = np.exp(-np.abs(z))
                mean = np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
            return self.X.T @ (mean - self.y) + q / self.pv


def recipe(family, D, n, N, cdt, seed, dtvec=False, covp=False, pvs=1.0):
    """X, beta, y, prior variances, start points, then the optional dt vector and cov_p; the draws of a
    sampler follow from the RandomState this returns (c["rs"]).
    poisson: X = 0.3 N(0, 1), beta = 2 N(0, 1) / sqrt(D) and y ~ Poisson(exp(X beta)), so that z stays
    moderate at every D (X beta has a standard deviation of 0.6);
    dt = cdt / sqrt(lambda_max(X^T W X + diag(1 / pv))) with W = diag(exp(X beta)) (poisson), I / 4
    (bernoulli: the logistic recipe of tests/test_gpu_logistic.py).
    pvs scales the prior variances pv = pvs U(0.5, 2) and, below 1, the start points with them: a
    tight prior brings the posterior's condition number down, so that a tree at a small d_max (7
    leapfrogs at d_max = 3) can reach its U-turn at a stable step."""
    rs = np.random.RandomState(seed)
    if family == "poisson":
        X = 0.3 * rs.standard_normal((n, D))
        beta = 2.0 * rs.standard_normal(D) / np.sqrt(D)
        y = rs.poisson(np.exp(X @ beta)).astype(float)
        W = np.exp(X @ beta)
    else:
        X = rs.standard_normal((n, D))
        beta = rs.standard_normal(D)
        y = (rs.random_sample(n) < 1 / (1 + np.exp(-X @ beta))).astype(float)
        W = np.full(n, 0.25)
    pv = pvs * rs.uniform(0.5, 2.0, D)
    lam = np.linalg.eigvalsh(X.T @ (W[:, None] * X) + np.diag(1 / pv)).max()
    dt = cdt / np.sqrt(lam)
    q_start = 0.5 * min(1.0, np.sqrt(pvs)) * rs.standard_normal((N, D))
    dt = dt * rs.uniform(0.7, 1.3, D) if dtvec else dt
    cov_p = np.diag(rs.uniform(0.9, 1.1, D)) if covp else None
    sd = np.sqrt(np.diag(cov_p)) if covp else 1.0
    return dict(family=family, D=D, n=n, N=N, dt=dt, cov_p=cov_p, X=X, y=y, pv=pv, q_start=q_start, sd=sd,
                seed=seed, rs=rs)


def oracle_target(c):
    return OracleGLM(c["X"], c["y"], c["pv"], c["family"])


def glm_target(c):
    from hmc_amd.target import GLMTarget
    return GLMTarget(c["X"], c["y"], c["family"], c["pv"])


class RecordingCore(O.HMCCore):
    """HMCCore that keeps every energy it returns."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.energies = []

    def E(self, q, p):
        e = super().E(q, p)
        self.energies.append(e)
        return e


class TreeShape:
    """Mixin for an oracle draw source: per (chain, iteration) the uniforms each sub-tree consumed, in
    order.  A sub-tree of 2^j points that runs to its end takes 2^j uniforms (2^j - 1 progressive ones
    and the acceptance's); one that is rejected (unstable or U-turn) takes fewer.  shapes[m][i - 1] is
    the list for iteration i, its length the tree depth."""

    def _init_shapes(self, N):
        self.shapes = [[] for _ in range(N)]

    def p(self, m, i):
        if i >= 1:
            self.shapes[m].append([])
        return super().p(m, i)

    def direction(self, m):
        self.shapes[m][-1].append(0)
        return super().direction(m)

    def uniform(self, m):
        self.shapes[m][-1][-1] += 1
        return super().uniform(m)


class TapeDraws(TreeShape, O.ReplayDraws):
    def __init__(self, p0, P, tape):
        O.ReplayDraws.__init__(self, p0, P, tape=tape.copy())
        self._init_shapes(p0.shape[0])


def tree_stats(shapes):
    """(depths (N, Niter), number of iterations whose last sub-tree was rejected)."""
    depth = np.array([[len(it) for it in ch] for ch in shapes])
    rejected = sum(1 for ch in shapes for it in ch if it and it[-1] < (1 << (len(it) - 1)))
    return depth, rejected
