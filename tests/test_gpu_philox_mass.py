"""Philox momenta under a mass matrix other than the identity, pinned to host-regenerated draws.

With rng="philox" and cov_p != I every kernel family builds its momentum its own way: a diagonal
cov_p scales z by sqrt(diag cov_p) (hmc_kinetic.p_scale), a full one forms p = C z with
C = chol(cov_p) passed transposed (hmc_kinetic.p_chol_t):
  Random, dense target  D <= 128   hmc_dense.hip   per-lane matvec over p_chol_t (iteration 0: a scalar loop)
  Random, dense target  D > 128    hmc_big.hip     z into a workspace vector, then a block GEMM
  Random, diagonal target          hmc_wave.hip / hmc_big.hip   p_scale only
  NUTS  D <= 128                   hmc_nuts.hip    matvec behind a ballot of the lanes starting an iteration
  NUTS  128 < D <= 320             hmc_nuts_lock.hip   block GEMM over transposed fragments
  NUTS  D > 320                    hmc_nuts_big.hip    one GEMV per chain
The replay-mode tests feed p itself, so none of them sees z -> p.  Here the production surface runs
with rng="philox"; z, L, log u and the NUTS directions / uniforms are regenerated on the host
(tests/philox_host.py) and replayed through the oracle with HMCCore(target, dt, cov_p).

Every parity case has a nonzero chain_offset, a chain count that is no multiple of 16 and at
least two launches.  Assertions (the tolerances of tests/test_gpu_philox_parity.py): identical
counters, q_chain within rtol = atol = 1e-9, E_chain within rtol = 1e-10.

The kinetic identity runs whole blocks: for p = C z, K = p.inv(cov_p).p / 2 = z.z / 2 exactly, so
each chain's K at every iteration start, recovered from the stored rows as E - V(q), must equal
half the squared norm of the host's z.  No oracle trajectory is needed.
"""
import functools

import numpy as np
import pytest

import make_golden_shapes as S
from oracle import hmc_oracle as O
from philox_host import PhiloxNutsDraws, dense_momenta, host_L_lnu, pair_p0, wave_momenta

gpu = pytest.mark.gpu


class FastMVN(O.MVNTarget):
    """V = 0.5 (logdet const + x.P.x) instead of scipy's eigh-based logpdf (same value to ~1e-14)."""

    def __init__(self, q0, cov0):
        super().__init__(q0, cov0)
        D = self.q0.size
        self.c = D * np.log(2 * np.pi) + np.linalg.slogdet(self.cov0)[1]

    def V(self, q):
        x = q - self.q0
        return 0.5 * (self.c + x @ (self.inv_cov0 @ x))


class DiagMVN:
    """MVNTarget for a diagonal covariance `var` (D,), without the D x D arrays (D = 2050)."""

    def __init__(self, q0, var):
        self.q0, self.prec = np.asarray(q0, np.float64), 1.0 / np.asarray(var, np.float64)
        self.c = self.q0.size * np.log(2 * np.pi) + np.sum(np.log(var))

    def V(self, q):
        x = q - self.q0
        return 0.5 * (self.c + x @ (self.prec * x))

    def dVdq(self, q):
        return self.prec * (q - self.q0)


class DiagCore(O.HMCCore):
    """HMCCore (samplers.py:811-839) for a diagonal cov_p `var_p` (D,): np.dot(diag(a), g) == a * g,
    so K and the half kicks are written elementwise (test_diag_core_is_hmccore pins it to HMCCore)."""

    def __init__(self, target, dt, var_p):
        self.t, self.dt, self.minv = target, dt, 1.0 / np.asarray(var_p, np.float64)

    def K(self, p):
        return np.dot(p, self.minv * p) / 2.

    def leap_frog(self, p_old, q_old):
        p_half = p_old - self.dt * (self.minv * self.t.dVdq(q_old)) / 2.
        q_new = q_old + self.dt * p_half
        p_new = p_half - self.dt * (self.minv * self.t.dVdq(q_new)) / 2.
        return p_new, q_new


def kinetic_from_rows(q_chain, E_chain, V):
    """K of every chain at every iteration start from the rows a run with warm_up = 0, thin = 1
    stores: E_chain[m, r] is E = V + K at the start of iteration r (r = 0: the initial draw,
    samplers.py:415-420), taken at q_chain[m, r - 1], the state iteration r - 1 left (q_chain[m, 0]
    for r = 0 and r = 1).  V: (n, D) -> (n,).  Returns (K, V at those q), each (N, rows)."""
    N, rows, D = q_chain.shape
    src = np.concatenate([q_chain[:, :1], q_chain[:, :-1]], axis=1)
    Vq = V(src.reshape(-1, D)).reshape(N, rows)
    return E_chain - Vq, Vq


def mvn_V(prec, c):
    """Vectorised V of a zero-mean MVN: rows of x -> 0.5 (c + x.P.x)."""
    return lambda x: 0.5 * (c + np.einsum("nd,nd->n", x @ prec, x))


# ------------------------------------------------------------------ host-only checks of the helpers
class _RecordingLiveDraws(O.LiveDraws):
    def __init__(self, D, cov_p):
        super().__init__(D, cov_p)
        self.rec = {}

    def p(self, m, i):
        self.rec[(m, i)] = super().p(m, i)
        return self.rec[(m, i)]


@pytest.mark.parametrize("sampler", ["random", "nuts"])
def test_kinetic_from_rows_on_oracle(sampler):
    """The row convention of kinetic_from_rows, fixed on the CPU: applied to an oracle run on
    np.random draws with a full cov_p it returns core.K(p) of every (chain, iteration) to 1e-12."""
    D, N, Niter = 5, 4, 3
    cov, cov_p = O.mvn_cov(D, 0.6), S.dense_cov_p(D)
    tgt = FastMVN(np.zeros(D), cov)
    core = O.HMCCore(tgt, 0.2, cov_p)
    np.random.seed(77)
    q_start = np.random.standard_normal((N, D))
    draws = _RecordingLiveDraws(D, cov_p)
    if sampler == "random":
        ref = O.gen_sample_random(core, q_start, N, Niter, 0, 1, 5, 13, draws)
    else:
        ref = O.gen_sample_nuts(core, q_start, N, Niter, 0, 1, 8, draws, on_dmax="break")
    K, _ = kinetic_from_rows(ref["q_chain"], ref["E_chain"], mvn_V(tgt.inv_cov0, tgt.c))
    want = np.array([[core.K(draws.rec[(m, i)]) for i in range(Niter + 1)] for m in range(N)])
    assert K.shape == want.shape
    np.testing.assert_allclose(K, want, rtol=0, atol=1e-12)
    if sampler == "random":                      # some rejected, so the rows really differ in what they hold
        assert 0 < ref["accept_count"] < N * Niter


def test_diag_core_is_hmccore():
    """DiagMVN / DiagCore (the D = 2050 case's oracle arithmetic) equal MVNTarget / HMCCore."""
    D = 9
    rs = np.random.RandomState(1)
    var, var_p, q0 = rs.uniform(0.5, 2, D), rs.uniform(0.5, 2, D), rs.standard_normal(D)
    a = O.HMCCore(FastMVN(q0, np.diag(var)), 0.3, np.diag(var_p))
    b = DiagCore(DiagMVN(q0, var), 0.3, var_p)
    p, q = rs.standard_normal(D), rs.standard_normal(D)
    for _ in range(5):
        np.testing.assert_allclose(b.E(q, p), a.E(q, p), rtol=1e-14)
        (pa, qa), (pb, qb) = a.leap_frog(p, q), b.leap_frog(p, q)
        np.testing.assert_allclose(pb, pa, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(qb, qa, rtol=1e-14, atol=1e-15)
        p, q = pa, qa


def test_dense_momenta_chain_ids():
    """The helpers key draws by the global chain id: a shard's rows are the whole batch's rows,
    above 2^32 too; dims h + 4m read slot h + 4 (m - (m & 1)), half m & 1."""
    seed, D = 0x51, 21
    gcs = np.array([0, 5, (1 << 33) + 2], dtype=np.uint64)
    p0, P = dense_momenta(seed, gcs, D, 2)
    for j, g in enumerate(gcs):
        q0, Q = dense_momenta(seed, np.array([g], dtype=np.uint64), D, 2)
        assert np.array_equal(q0[0], p0[j]) and np.array_equal(Q[0], P[j])
    assert not np.array_equal(P[0], P[2])
    # slot 1 holds dims 1 and 5, slot 9 dims 9 and 13, slot 16 dims 16 and 20
    from philox_host import bm_pair, words
    for slot, (d0, d1) in {1: (1, 5), 9: (9, 13), 16: (16, 20)}.items():
        z0, z1 = bm_pair(words(slot, 0, gcs[1], seed))
        assert p0[1, d0] == z0 and p0[1, d1] == z1
    assert np.array_equal(dense_momenta(seed, gcs, D, 1, pair0=True)[0], pair_p0(seed, gcs, D))
    assert np.array_equal(pair_p0(seed, np.arange(40, 43), D), wave_momenta(seed, 3, D, 1, chain0=40)[0])


# ------------------------------------------------------------------ value parity, Random sampler
L_LOW, L_HIGH = 5, 13            # L in 5..12 (high exclusive, samplers.py:441)
BIG_OFFSET = (1 << 33) + 7       # a chain id with a nonzero high word


def _mass(mass, D, rs):
    return S.dense_cov_p(D) if mass == "full" else np.diag(rs.uniform(0.5, 2.0, D))


def _apply_mass(z, cov_p, mass):
    """p from the unit normals z (..., D): C z with C = chol(cov_p), or z sqrt(diag cov_p)."""
    return z @ np.linalg.cholesky(cov_p).T if mass == "full" else z * np.sqrt(np.diag(cov_p))


# kernel, target, cov_p, D, N, rho, dt.  dt = 0.02 with a full cov_p; the diagonal cases' dt chosen
# on the oracle so that some proposals are accepted and some rejected (the reference drifts by p,
# not inv(cov_p) p (Q3), so with cov_p != I the acceptance falls quickly with dt: 0.2 .. 0.7 here).
RANDOM_CASES = [
    ("dense", "dense", "full", 37, 24, 0.5, 0.02),
    ("dense", "dense", "diag", 37, 24, 0.5, 0.02),
    ("dense", "dense", "full", 100, 40, 0.9, 0.02),
    ("dense", "dense", "diag", 100, 40, 0.9, 0.01),
    ("dense", "dense", "full", 128, 20, 0.6, 0.02),
    ("dense", "dense", "diag", 128, 20, 0.6, 0.01),
    ("big", "dense", "full", 129, 20, 0.5, 0.02),
    ("big", "dense", "diag", 129, 20, 0.5, 0.02),
    ("big", "dense", "full", 300, 20, 0.5, 0.02),
    ("big", "dense", "diag", 300, 20, 0.5, 0.01),
    ("wave", "diag", "diag", 100, 20, 0.0, 0.02),
    ("wave", "diag", "diag", 129, 20, 0.0, 0.02),
    ("wave", "diag", "diag", 300, 20, 0.0, 0.01),
    ("bigdiag", "diag", "diag", 2050, 20, 0.0, 0.005),
]
# fp_mode="exact" once per kernel family
RANDOM_EXACT = {("dense", "full", 37), ("big", "full", 129), ("wave", "diag", 129), ("bigdiag", "diag", 2050)}
RANDOM_PARAMS = [pytest.param(c, m, id="%s_D%d_%s_%s" % (c[0], c[3], c[2], m))
                 for c in RANDOM_CASES for m in ("fast", "exact")
                 if m == "fast" or (c[0], c[2], c[3]) in RANDOM_EXACT]
NITER_R, WU_R, PER_LAUNCH_R = 5, 2, 2          # launches of 2, 2 and 1 iterations


@functools.lru_cache(maxsize=None)
def _random_reference(case, offset):
    kernel, target, mass, D, N, rho, dt = case
    rs = np.random.RandomState(4000 + 3 * D + (mass == "full"))
    seed = 0xA55_0000 + D
    cov_p = _mass(mass, D, rs)
    if target == "dense":
        var = None
        cov = O.mvn_cov(D, rho)
        q_start = rs.standard_normal((N, D)) @ np.linalg.cholesky(cov).T
    else:
        var = rs.uniform(0.5, 2.0, D)
        cov = None
        q_start = rs.standard_normal((N, D)) * np.sqrt(var)
    gcs = offset + np.arange(N, dtype=np.uint64)
    if kernel == "dense":
        z0, Z = dense_momenta(seed, gcs, D, NITER_R)
    else:                                       # hmc_wave.hip, hmc_big.hip: pair k holds dims 2k, 2k+1
        z0, Z = wave_momenta(seed, N, D, NITER_R, chain0=offset)
    p0, P = _apply_mass(z0, cov_p, mass), _apply_mass(Z, cov_p, mass)
    L, lnu = host_L_lnu(seed, gcs, NITER_R, L_LOW, L_HIGH)
    if D > 1024:                                # diagonal everything: elementwise oracle arithmetic
        tgt = DiagMVN(np.zeros(D), var)
        core = DiagCore(tgt, dt, np.diag(cov_p))
    else:
        tgt = FastMVN(np.zeros(D), cov if cov is not None else np.diag(var))
        core = O.HMCCore(tgt, dt, cov_p)
    ref = O.gen_sample_random(core, q_start, N, NITER_R, WU_R, 1, L_LOW, L_HIGH, O.ReplayDraws(p0, P, L, lnu))
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(ref=ref, seed=seed, cov_p=cov_p, cov=cov, var=var, c=tgt.c, q_start=q_start, L=L)


def _offset(case_key, fp_mode):
    return BIG_OFFSET if fp_mode == "exact" else 1_000_003 + 16 * case_key


@pytest.mark.parametrize("case", RANDOM_CASES, ids=["%s_D%d_%s" % (c[0], c[3], c[2]) for c in RANDOM_CASES])
def test_random_reference_accepts_and_rejects(case):
    """The condition every Random parity case stands on, on the reference's own numbers: in the
    oracle run some proposals are accepted and some rejected, after and during warm-up."""
    N = case[4]
    assert N % 16 != 0
    ref = _random_reference(case, _offset(case[3], "fast"))["ref"]
    assert 0 < ref["accept_R"] < 1, ref["accept_R"]
    assert 0 < ref["accept_count"] + ref["accept_count_warm_up"] < N * NITER_R


@gpu
@pytest.mark.parametrize("case,fp_mode", RANDOM_PARAMS)
def test_random_philox_mass_vs_oracle(case, fp_mode):
    """HMC_sampler(sampler_type="Random", rng="philox", cov_p != I) vs the oracle on the host's draws."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    kernel, target, mass, D, N, rho, dt = case
    offset = _offset(D, fp_mode)
    r = _random_reference(case, offset)
    ref = r["ref"]
    assert 0 < ref["accept_R"] < 1
    if target == "dense":
        tgt = MVNTarget(np.zeros(D), r["cov"], logdet_const=r["c"])
    else:
        tgt = MVNTarget(np.zeros(D), prec=np.diag(1.0 / r["var"]), logdet_const=r["c"])
    h = HMC_sampler(D, None, None, Nchain=N, Niter=NITER_R, sampler_type="Random", L_low=L_LOW, L_high=L_HIGH, dt=dt,
                    warm_up_num=WU_R, cov_p=r["cov_p"], target=tgt, rng="philox", seed=r["seed"], fp_mode=fp_mode,
                    chain_offset=offset, iters_per_launch=PER_LAUNCH_R)
    h.gen_sample(r["q_start"], verbose=False)
    assert h.n_leapfrog == ref["n_leapfrog"] == int(r["L"].sum())
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)


# ------------------------------------------------------------------ value parity, NUTS
# kernel, D, N, rho, Niter, dt, d_max, cov_p
NUTS_CASES = [
    ("tree", 12, 24, 0.6, 5, 0.15, 9, "full"),
    ("tree", 12, 24, 0.6, 5, 0.15, 9, "diag"),
    ("tree", 100, 20, 0.9, 4, 0.1, 8, "full"),
    ("tree", 100, 20, 0.9, 4, 0.1, 8, "diag"),
    ("lock", 129, 18, 0.5, 3, 0.15, 7, "full"),
    ("lock", 129, 18, 0.5, 3, 0.15, 7, "diag"),
    ("lock", 144, 40, 0.8, 3, 0.2, 6, "full"),       # slots take two chains: the chains of one block
    ("lock", 144, 40, 0.8, 3, 0.2, 6, "diag"),       # start their iterations at different block steps
    ("lock", 300, 18, 0.5, 3, 0.15, 7, "full"),      # the kLockJ instance
    ("lock", 300, 18, 0.5, 3, 0.15, 7, "diag"),
    ("lock", 320, 3, 0.5, 3, 0.15, 7, "full"),       # upper bound of the lockstep range
    ("lock", 320, 3, 0.5, 3, 0.15, 7, "diag"),
    ("perchain", 321, 3, 0.5, 3, 0.15, 7, "full"),
    ("perchain", 330, 3, 0.5, 3, 0.15, 7, "full"),
]
NUTS_EXACT = {("tree", 100, "full"), ("lock", 320, "full"), ("perchain", 321, "full")}
NUTS_PARAMS = [pytest.param(c, m, id="%s_D%d_%s_%s" % (c[0], c[1], c[7], m))
               for c in NUTS_CASES for m in ("fast", "exact")
               if m == "fast" or (c[0], c[1], c[7]) in NUTS_EXACT]
WU_N, PER_LAUNCH_N = 1, 2
# Philox seeds are 0xB660000 + D + (bump << 12).  The oracle run of a parity case should reach d_max
# nowhere; with bump = 0 two rows did in a few trees, and these bumps are the first without one.
NUTS_SEED_BUMP = {(129, "full"): 21, (330, "full"): 1}
# Rows whose oracle run reaches d_max whatever the seed (trees that break at d_max out of
# N * Niter = 120, over 3 start seeds x 4 start scales, and 60 Philox seeds for the diagonal row:
# D = 12 full 2 .. 13, D = 144 full 10 .. 42, D = 144 diagonal 0 once in 72 runs, else 1 .. 15): at
# these D, dt and d_max a tenth of the trees is still open after d_max doublings.  The shapes are
# kept as they are and the d_max counter is compared exactly, like every other counter.
NUTS_DMAX_ROWS = {(12, "full"), (144, "full"), (144, "diag")}


@functools.lru_cache(maxsize=None)
def _nuts_reference(case, offset):
    kernel, D, N, rho, Niter, dt, d_max, mass = case
    rs = np.random.RandomState(5000 + 3 * D + (mass == "full"))
    seed = 0xB66_0000 + D + (NUTS_SEED_BUMP.get((D, mass), 0) << 12)
    cov, cov_p = O.mvn_cov(D, rho), _mass(mass, D, rs)
    q_start = rs.standard_normal((N, D)) * 1.2           # (the start of tests/test_gpu_nuts_big.py)
    gcs = offset + np.arange(N, dtype=np.uint64)
    z0, Z = dense_momenta(seed, gcs, D, Niter, pair0=D > 128)
    p0, P = _apply_mass(z0, cov_p, mass), _apply_mass(Z, cov_p, mass)
    tgt = FastMVN(np.zeros(D), cov)
    ref = O.gen_sample_nuts(O.HMCCore(tgt, dt, cov_p), q_start, N, Niter, WU_N, 1, d_max,
                            PhiloxNutsDraws(seed, p0, P, gcs), on_dmax="break")
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dict(ref=ref, seed=seed, cov=cov, cov_p=cov_p, c=tgt.c, q_start=q_start)


@pytest.mark.parametrize("case", NUTS_CASES, ids=["%s_D%d_%s" % (c[0], c[1], c[7]) for c in NUTS_CASES])
def test_nuts_reference_is_stable_below_dmax(case):
    """The condition every NUTS parity case stands on: the oracle run has no unstable sub-tree and
    never reaches d_max (NUTS_DMAX_ROWS: in fewer than half of its trees), and its trees are deep
    enough to check U-turns (> 3 leapfrogs each)."""
    N, Niter = case[2], case[4]
    assert N % 16 != 0
    ref = _nuts_reference(case, _offset(case[1], "fast"))["ref"]
    assert ref["n_unstable"] == 0
    if (case[1], case[7]) in NUTS_DMAX_ROWS:
        assert 2 * ref["n_dmax"] < N * Niter
    else:
        assert ref["n_dmax"] == 0
    assert ref["n_leapfrog"] > 3 * N * Niter


@gpu
@pytest.mark.parametrize("case,fp_mode", NUTS_PARAMS)
def test_nuts_philox_mass_vs_oracle(case, fp_mode):
    """HMC_sampler(sampler_type="NUTS", rng="philox", cov_p != I) vs the oracle on the host's draws."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    kernel, D, N, rho, Niter, dt, d_max, mass = case
    offset = _offset(D, fp_mode)
    r = _nuts_reference(case, offset)
    ref = r["ref"]
    assert ref["n_unstable"] == 0 and (ref["n_dmax"] == 0 or (D, mass) in NUTS_DMAX_ROWS)
    h = HMC_sampler(D, None, None, Nchain=N, Niter=Niter, warm_up_num=WU_N, sampler_type="NUTS", dt=dt, d_max=d_max,
                    cov_p=r["cov_p"], target=MVNTarget(np.zeros(D), r["cov"], logdet_const=r["c"]), rng="philox",
                    seed=r["seed"], fp_mode=fp_mode, chain_offset=offset, iters_per_launch=PER_LAUNCH_N)
    h.gen_sample_NUTS(r["q_start"], 0, False, on_dmax="break")
    assert h.n_leapfrog == ref["n_leapfrog"]
    assert h.n_unstable == ref["n_unstable"]
    assert h.n_dmax == ref["n_dmax"]
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)


# ------------------------------------------------------------------ kinetic identity at block occupancy
# sampler, D, N: whole blocks of chains in differing states, plus a ragged tail
KINETIC_CASES = [("random", 100, 1007), ("random", 136, 1007), ("nuts", 100, 1007), ("nuts", 136, 1007),
                 ("nuts", 300, 1007), ("nuts", 330, 67)]


@gpu
@pytest.mark.parametrize("sampler,D,N", KINETIC_CASES, ids=["%s_D%d" % c[:2] for c in KINETIC_CASES])
def test_kinetic_identity_full_cov_p(sampler, D, N):
    """K = z.z / 2 for p = C z, per chain and iteration start (iteration 0, the initial draw,
    included), at N = 1000 + 7 chains (64 + 3 for the per-chain NUTS kernel): K recovered from the
    stored rows (kinetic_from_rows) against the host's z, within the project's relative E
    tolerance 1e-10 applied to both terms of the subtraction E - V."""
    from hmc_amd.engine import NutsEngine, RandomEngine
    from hmc_amd.target import MVNTarget
    import torch
    Niter, seed, offset = 3, 0xC77_0000 + D, 2_000_003 + D
    rs = np.random.RandomState(6000 + D)
    cov, cov_p = O.mvn_cov(D, 0.5), S.dense_cov_p(D)
    q_start = rs.standard_normal((N, D)) @ np.linalg.cholesky(cov).T
    ftgt = FastMVN(np.zeros(D), cov)
    tgt = MVNTarget(np.zeros(D), cov, logdet_const=ftgt.c)
    gcs = offset + np.arange(N, dtype=np.uint64)
    if sampler == "random":
        eng = RandomEngine(tgt, N, Niter, 0, 1, L_LOW, L_HIGH, 0.02, cov_p=cov_p, rng="philox", seed=seed,
                           fp_mode="fast", chain_offset=offset)
        if D <= 128:
            z0, Z = dense_momenta(seed, gcs, D, Niter)
        else:
            z0, Z = wave_momenta(seed, N, D, Niter, chain0=offset)
    else:
        eng = NutsEngine(tgt, N, Niter, 0, 1, 7, 0.15, cov_p=cov_p, rng="philox", seed=seed, fp_mode="fast",
                         chain_offset=offset, on_dmax="break")
        z0, Z = dense_momenta(seed, gcs, D, Niter, pair0=D > 128)
    eng.init(q_start)
    eng.run(1, 3)
    eng.run(3, Niter + 1)
    torch.cuda.synchronize()
    q_chain, E = eng.q_chain.cpu().numpy(), eng.E_chain.cpu().numpy()
    assert np.isfinite(q_chain).all() and np.isfinite(E).all()
    assert not np.array_equal(q_chain[:, -1], q_chain[:, 0])
    K, Vq = kinetic_from_rows(q_chain, E, mvn_V(ftgt.inv_cov0, ftgt.c))
    z = np.concatenate([z0[:, None, :], Z], axis=1)
    want = 0.5 * np.einsum("nid,nid->ni", z, z)
    err, bound = np.abs(K - want), 1e-10 * (np.abs(E) + np.abs(Vq))
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert np.all(err <= bound), "chain %d iteration %d: K %.15g, z.z/2 %.15g, bound %.3g" % (
        worst[0], worst[1], K[worst], want[worst], bound[worst])
