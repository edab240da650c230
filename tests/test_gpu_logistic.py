"""Bayesian logistic-regression target on the GPU (csrc/hmc_logit.hip) against the CPU oracle.

The oracle target (`OracleLogistic`) is written here, directly from
    V(q) = sum_j [softplus(z_j) - y_j z_j] + 0.5 sum_d q_d^2 / prior_var_d,   z = X q
    softplus(z) = max(z, 0) + log1p(exp(-|z|))
    dV/dq = X^T (sigma(z) - y) + q / prior_var,   sigma(z) = 1/(1+e^-z) (z >= 0), e^z/(1+e^z) (z < 0)
and independently of hmc_amd.target.LogisticTarget; oracle/hmc_oracle.py's HMCCore and
gen_sample_random run it unchanged.

Every parity case first asserts, on the oracle alone, conditions on its INPUTS (not tolerances on the
kernel): (1) no Metropolis decision is within 1e-4 of flipping, (2) the oracle rerun from
q_start (1 + 1e-13) moves q_chain by at most 1e-11, and (3) at least 2 and at most 60 % of the
proposals are rejected.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hmc_oracle as O
from philox_host import dense_momenta, host_L_lnu

pytestmark = pytest.mark.gpu


class OracleLogistic:
    def __init__(self, X, y, pv):
        self.X, self.y, self.pv = np.asarray(X, float), np.asarray(y, float), np.asarray(pv, float)
        self.q0 = np.zeros(self.X.shape[1])          # HMCCore reads the dimension from q0

    def V(self, q):
        z = self.X @ q
        return np.sum(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) - self.y * z) + 0.5 * np.sum(q * q / self.pv)

    def dVdq(self, q):
        z = self.X @ q
        t = np.exp(-np.abs(z))
        sigma = np.where(z >= 0, 1.0 / (1.0 + t), t / (1.0 + t))
        return self.X.T @ (sigma - self.y) + q / self.pv


class RecordingCore(O.HMCCore):
    """HMCCore that keeps every energy it returns: gen_sample_random asks for one per chain start and
    then (E_init, E_final) per iteration, which gives each proposal's dE."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.energies = []

    def E(self, q, p):
        e = super().E(q, p)
        self.energies.append(e)
        return e


#        D    n    N  Niter wu thin L_low L_high c   seed dt_vec cov_p
CASES = {
    "A": (2, 20, 5, 12, 4, 1, 5, 20, 1.5, 11, False, False),       # D < 4, ragged row tile
    "B": (37, 100, 4, 40, 7, 2, 5, 20, 0.7, 2, True, True),        # every option at once
    "C": (16, 16, 17, 20, 0, 1, 5, 20, 1.1, 3, False, False),      # exact tiles in D and n; one chain over a tile
    "D": (17, 17, 16, 20, 5, 3, 5, 20, 1.2, 4, False, False),      # one over in D and n; exactly one chain tile
    "E": (1, 1, 6, 40, 0, 1, 1, 6, 1.5, 5, False, False),          # D = 1, n = 1, L from 1
    "F": (64, 250, 4, 20, 3, 1, 5, 20, 0.9, 6, False, False),
    "G": (65, 33, 33, 12, 3, 1, 5, 20, 0.6, 7, False, True),       # three chain tiles, last with one chain
    "H": (128, 1000, 3, 10, 0, 1, 5, 12, 0.7, 8, False, False),    # ABI limit in D
    "I": (25, 1000, 4, 20, 2, 1, 5, 20, 1.1, 9, False, False),     # a realistic shape
}

# warm_up = 16 > L_chain * thin = 5: the reference raises IndexError (test_out_of_range_rejections_and_L_tallies);
# 19 chains are two tiles, the second with three
OOB_CASE = (3, 8, 19, 20, 16, 1, 5, 20, 1.5, 12, False, False)


def recipe(name, N=None, Niter=None):
    """The shared input recipe, every draw from one RandomState(seed) in this order: X, beta, y,
    prior variances, start points, Z0, Z, L, log u, then the optional dt vector and cov_p."""
    D, n, N_, Niter_, wu, thin, Llo, Lhi, cdt, seed, dtvec, covp = OOB_CASE if name == "oob" else CASES[name]
    N, Niter = N or N_, Niter or Niter_
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, D))
    beta = rs.standard_normal(D)
    y = (rs.random_sample(n) < 1 / (1 + np.exp(-X @ beta))).astype(float)
    pv = rs.uniform(0.5, 2.0, D)
    lam = np.linalg.eigvalsh(X.T @ X / 4 + np.diag(1 / pv)).max()
    dt = cdt / np.sqrt(lam)
    q_start = 0.5 * rs.standard_normal((N, D))
    Z0 = rs.standard_normal((N, D))
    Z = rs.standard_normal((N, Niter, D))
    L = rs.randint(Llo, Lhi, size=(N, Niter)).astype(np.int32)
    lnu = np.log(rs.random_sample((N, Niter)))
    dt = dt * rs.uniform(0.7, 1.3, D) if dtvec else dt
    cov_p = np.diag(rs.uniform(0.9, 1.1, D)) if covp else None
    sd = np.sqrt(np.diag(cov_p)) if covp else 1.0
    return dict(D=D, n=n, N=N, Niter=Niter, wu=wu, thin=thin, Llo=Llo, Lhi=Lhi, dt=dt, cov_p=cov_p, X=X, y=y, pv=pv,
                q_start=q_start, p0=Z0 * sd, P=Z * sd, L=L, lnu=lnu, sd=sd, seed=seed)


def oracle_run(c, q_start=None, n_save=0):
    core = RecordingCore(OracleLogistic(c["X"], c["y"], c["pv"]), c["dt"], c["cov_p"])
    out = O.gen_sample_random(core, c["q_start"] if q_start is None else q_start, c["N"], c["Niter"], c["wu"],
                              c["thin"], c["Llo"], c["Lhi"], O.ReplayDraws(c["p0"], c["P"], c["L"], c["lnu"]),
                              n_save_chain0=n_save)
    E = np.asarray(core.energies).reshape(c["N"], 1 + 2 * c["Niter"])
    out["dE_prop"] = E[:, 2::2] - E[:, 1::2]          # (N, Niter): E_final - E_init of every proposal
    return out


def check_input_conditions(c, ref):
    """The conditions of the module docstring; prints each figure before asserting it."""
    dE, lnu = ref["dE_prop"], c["lnu"]
    up = dE >= 0
    margin = np.abs(lnu + dE)[up].min() if up.any() else np.inf
    pert = oracle_run(c, q_start=c["q_start"] * (1 + 1e-13))
    sens = np.abs(pert["q_chain"] - ref["q_chain"]).max()
    rejected = int(np.sum(~((dE < 0) | (lnu < -dE))))
    print("margin %.3g  sensitivity %.3g  rejected %d/%d" % (margin, sens, rejected, dE.size))
    assert margin >= 1e-4
    assert sens <= 1e-11
    assert rejected >= 2
    assert rejected <= 0.60 * dE.size


@functools.lru_cache(maxsize=None)
def case(name):
    c = recipe(name)
    return c, oracle_run(c)


def target_of(c, y=None):
    from hmc_amd.target import LogisticTarget
    return LogisticTarget(c["X"], c["y"] if y is None else y, c["pv"])


def sampler(c, rng="replay", **kw):
    from hmc_amd.samplers import HMC_sampler
    args = dict(Nchain=c["N"], Niter=c["Niter"], thin_rate=c["thin"], warm_up_num=c["wu"], cov_p=c["cov_p"],
                sampler_type="Random", dt=c["dt"], L_low=c["Llo"], L_high=c["Lhi"], target=target_of(c), rng=rng)
    args.update(kw)
    h = HMC_sampler(c["D"], None, None, **args)
    if rng == "replay":
        h.set_random_replay(c["p0"], c["P"], c["L"], c["lnu"])
    return h


def assert_run_matches(h, ref):
    """The bounds of the existing FAST-mode parity tests (test_gpu_mixture.py::assert_run_matches)."""
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.n_leapfrog == ref["n_leapfrog"] and h.N_total_steps == ref["N_total_steps"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)
    np.testing.assert_allclose(h.dE_chain[:, :, 0], ref["dE_chain"], rtol=1e-8, atol=1e-10)
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]


OUTPUTS = ("q_chain", "E_chain", "dE_chain", "_acc", "_acc_wu", "n_leapfrog", "N_total_steps")


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", sorted(CASES))
def test_primitives_vs_oracle(name):
    """hmc_logit_energy / hmc_logit_leapfrog on 64 rows: 56 at 0.5 N(0, I) and 8 at +-1e3 (1 + 0.1 u)
    per coordinate, where exp(-|z|) underflows and both sides must stay finite."""
    c = recipe(name)
    D = c["D"]
    rs = np.random.RandomState(1000 + c["seed"])
    q = 0.5 * rs.standard_normal((64, D))
    q[56:] = 1e3 * np.where(rs.random_sample((8, D)) < 0.5, -1.0, 1.0) * (1.0 + 0.1 * rs.random_sample((8, D)))
    p = rs.standard_normal((64, D)) * c["sd"]
    h = sampler(c)
    core = O.HMCCore(OracleLogistic(c["X"], c["y"], c["pv"]), c["dt"], c["cov_p"])
    E = h.E(q, p)
    E_ref = np.array([core.E(q[i], p[i]) for i in range(64)])
    assert np.all(np.isfinite(E)) and np.all(np.isfinite(E_ref))
    np.testing.assert_allclose(E, E_ref, rtol=1e-10, atol=1e-12)
    pn, qn = h.leap_frog(p, q)
    ref = [core.leap_frog(p[i], q[i]) for i in range(64)]
    assert np.all(np.isfinite(pn)) and np.all(np.isfinite(qn))
    np.testing.assert_allclose(pn, [r[0] for r in ref], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(qn, [r[1] for r in ref], rtol=1e-10, atol=1e-12)
    e1, (p1, q1) = h.E(q[3], p[3]), h.leap_frog(p[3], q[3])          # single rows keep their shape
    assert np.ndim(e1) == 0 and p1.shape == (D,) and q1.shape == (D,)
    assert e1 == E[3] and np.array_equal(p1, pn[3]) and np.array_equal(q1, qn[3])


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", sorted(CASES))
def test_replay_parity(name):
    c, ref = case(name)
    check_input_conditions(c, ref)
    h = sampler(c, fp_mode="fast")
    h.gen_sample(c["q_start"], verbose=False)
    assert_run_matches(h, ref)
    if name == "D":                                   # one arithmetic: fp_mode changes nothing
        g = sampler(c, fp_mode="exact")
        g.gen_sample(c["q_start"], verbose=False)
        for a in OUTPUTS:
            assert np.array_equal(getattr(g, a), getattr(h, a)), a


# ------------------------------------------------------------------------------------------ 3
def test_chain0_capture():
    c, _ = case("A")
    ref = oracle_run(c, n_save=8)
    h = sampler(c)
    h.gen_sample(c["q_start"], N_save_chain0=8, verbose=False)
    assert_run_matches(h, ref)
    assert np.array_equal(h.decision_chain[:, 0], ref["decision_chain"])
    assert len(h.phi_q) == len(ref["phi_q"]) == 8
    for a, b in zip(h.phi_q, ref["phi_q"]):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------------------------------ 4
def philox_streams(c, seed, chain0=0):
    """The draws the kernel makes, regenerated on the host (tests/philox_host.py): the dense Random
    kernel's momenta (dims h + 4m) and block (0x80000000, it, chain) for (L, log u)."""
    N, D, Niter = c["N"], c["D"], c["Niter"]
    gcs = np.arange(chain0, chain0 + N, dtype=np.uint64)
    p0, P = dense_momenta(seed, gcs, D, Niter)
    L, lnu = host_L_lnu(seed, gcs, Niter, c["Llo"], c["Lhi"])
    return dict(c, p0=p0 * c["sd"], P=P * c["sd"], L=L, lnu=lnu)


def test_philox_parity():
    seed = 22
    c = philox_streams(recipe("B", N=48, Niter=20), seed)
    ref = oracle_run(c)
    check_input_conditions(c, ref)
    h = sampler(c, rng="philox", seed=seed, fp_mode="fast")
    h.gen_sample(c["q_start"], verbose=False)
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 5
def test_layout_and_launch_invariance():
    """One launch against launches of 7 iterations, and shards [0, 40) + [40, 96): 40 is not a multiple
    of 16, so the second shard's chains sit in other tile columns than in the single run."""
    c = recipe("F", N=96)

    def run(q_start, **kw):
        h = sampler(dict(c, N=len(q_start)), rng="philox", seed=5, **kw)
        h.gen_sample(q_start, verbose=False)
        return h

    one = run(c["q_start"])
    split = run(c["q_start"], iters_per_launch=7)
    for a in OUTPUTS:
        assert np.array_equal(getattr(one, a), getattr(split, a)), a
    lo, hi = run(c["q_start"][:40], chain_offset=0), run(c["q_start"][40:], chain_offset=40)
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(one, a), np.concatenate([getattr(lo, a), getattr(hi, a)])), a
    for a in ("_acc", "_acc_wu", "n_leapfrog"):
        assert getattr(one, a) == getattr(lo, a) + getattr(hi, a), a


# ------------------------------------------------------------------------------------------ 6
def logistic_engine(c, Niter, wu, **kw):
    from hmc_amd.engine import LogisticEngine
    y = kw.pop("y", None)
    return LogisticEngine(target_of(c, y), c["N"], Niter, wu, 1, 5, 20, c["dt"], rng="philox", seed=11, **kw)


def test_window_storage():
    """Every row into a circular window of R rows over 5 launches of 8 iterations (bench.py's storage
    path): the window holds the last R rows of a stored run, bitwise."""
    c = recipe("C", N=24)
    S, launches, R = 8, 5, 8
    Niter, wu = S * launches, S + 1
    full = logistic_engine(c, Niter, wu, store_chain=True)
    full.init(c["q_start"])
    full.run(1, Niter + 1)
    eng = logistic_engine(c, Niter, wu, store_chain=False)
    win = torch.zeros((c["N"], R, c["D"]), dtype=torch.float64, device=eng.device)
    eng.set_chain_window(win, 0)
    eng.init(c["q_start"])
    for k in range(launches):
        eng.run(1 + k * S, 1 + (k + 1) * S)
    torch.cuda.synchronize()
    rows = full.q_chain.shape[1]
    assert rows % R == 0 and rows > R
    assert torch.equal(win, full.q_chain[:, rows - R:])
    assert torch.equal(eng.E_chain, full.E_chain) and torch.equal(eng.q, full.q)
    assert np.array_equal(eng.read_counters(), full.read_counters())


# ------------------------------------------------------------------------------------------ 7
def test_streaming_diagnostics_match_stored_chain():
    c = recipe("B", N=8, Niter=120)
    c = dict(c, wu=20, thin=1)
    out = []
    for store in (True, False):
        h = sampler(c, rng="philox", seed=21, store_chain=store)
        h.gen_sample(c["q_start"], verbose=False)
        h.compute_convergence_stats()
        out.append(h)
    full, st = out
    assert st.q_chain is None and st.stream_info["truncated_dims"] == 0
    assert st._acc == full._acc and st.n_leapfrog == full.n_leapfrog
    np.testing.assert_allclose(st.R_q, full.R_q, rtol=1e-10)           # tests/test_gpu_exact_ess.py's bounds
    np.testing.assert_allclose(st.n_eff_q, full.n_eff_q, rtol=1e-8)


# ------------------------------------------------------------------------------------------ 8
def test_checkpoint(tmp_path):
    """save after iteration 9 of 20, restore into a fresh engine, run to the end: bitwise the
    uninterrupted run.  The checkpoint fingerprints the data: one flipped label refuses it."""
    c = recipe("D")
    Niter, wu = 20, 5
    whole = logistic_engine(c, Niter, wu)
    whole.init(c["q_start"])
    whole.run(1, Niter + 1)
    first = logistic_engine(c, Niter, wu)
    first.init(c["q_start"])
    first.run(1, 10)
    path = str(tmp_path / "logit.npz")
    first.save(path, 10)
    second = logistic_engine(c, Niter, wu)
    it = second.restore(path)
    assert it == 10
    second.run(it, Niter + 1)
    torch.cuda.synchronize()
    for a in ("q", "E_prev", "q_chain", "E_chain", "dE_chain"):
        assert torch.equal(getattr(second, a), getattr(whole, a)), a
    assert np.array_equal(second.read_counters(), whole.read_counters())
    y = c["y"].copy()
    y[3] = 1.0 - y[3]
    with pytest.raises(AssertionError):
        logistic_engine(c, Niter, wu, y=y).restore(path)


# ------------------------------------------------------------------------------------------ 9
def test_stationarity_from_exact_posterior_draws():
    """16,384 chains start at exact posterior draws (rejection from the prior); HMC leaves the
    posterior invariant, so the final rows are exact draws too and, for any density ~ exp(-V),
    E[dV/dq_d] = 0 and E[q_d dV/dq_d] = 1: both within 5 standard errors, taken from the start sample."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import LogisticTarget
    N, Niter = 16384, 30
    rs = np.random.RandomState(2025)
    X = rs.standard_normal((6, 3))
    y = (rs.random_sample(6) < 0.5).astype(float)
    cand = rs.standard_normal((4000000, 3))
    z = cand @ X.T
    nll = np.sum(np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) - y * z, axis=1)
    keep = np.log(rs.random_sample(len(cand))) < -nll
    print("rejection sampler kept %d of %d" % (keep.sum(), len(cand)))
    assert keep.sum() >= N
    q_start = cand[keep][:N]
    h = HMC_sampler(3, None, None, Nchain=N, Niter=Niter, sampler_type="Random", L_low=5, L_high=20, dt=0.3,
                    target=LogisticTarget(X, y, 1.0), rng="philox", seed=9)
    h.gen_sample(q_start, verbose=False)
    assert h.accept_R > 0
    x = h.q_chain[:, -1, :]
    assert not np.array_equal(x, q_start)
    oracle = OracleLogistic(X, y, np.ones(3))

    def moments(rows):
        g = np.array([oracle.dVdq(r) for r in rows])
        return g, rows * g

    g0, qg0 = moments(q_start)
    g1, qg1 = moments(x)
    z1 = g1.mean(axis=0) / (g0.std(axis=0, ddof=1) / np.sqrt(N))
    z2 = (qg1.mean(axis=0) - 1.0) / (qg0.std(axis=0, ddof=1) / np.sqrt(N))
    print("z-scores  E[g]:", z1, " E[q g] - 1:", z2)
    assert np.all(np.abs(z1) <= 5) and np.all(np.abs(z2) <= 5)


# ------------------------------------------------------------------------------------------ 10
def test_non_finite_chain_is_rejected_and_isolated():
    """Case A's first four chains with and without a fifth at 1e200 in their tile."""
    c = recipe("A")
    good = c["q_start"][:4]
    bad = np.full((1, c["D"]), 1e200)
    runs = []
    for qs in (good, np.concatenate([good, bad])):
        h = sampler(dict(c, N=len(qs)), rng="philox", seed=3)
        h.gen_sample(qs, verbose=False)
        runs.append(h)
    ok, mixed = runs
    assert np.array_equal(mixed.q_chain[:4], ok.q_chain) and np.array_equal(mixed.E_chain[:4], ok.E_chain)
    assert np.array_equal(mixed.dE_chain[:4], ok.dE_chain)
    assert np.all(mixed.q_chain[4] == 1e200)
    assert (mixed._acc, mixed._acc_wu) == (ok._acc, ok._acc_wu)        # every proposal of the bad chain rejected
    assert not np.any(np.isfinite(mixed.E_chain[4]))


# ------------------------------------------------------------------------------------------ 11
def test_refusals_and_neighbours_unchanged():
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import LogisticTarget, MixtureTarget, MVNTarget
    c = recipe("A")
    t = target_of(c)
    kw = dict(Nchain=2, Niter=10, dt=0.1, target=t)
    with pytest.raises(NotImplementedError):
        HMC_sampler(2, None, None, sampler_type="NUTS", d_max=5, **kw)
    with pytest.raises(NotImplementedError):
        HMC_sampler(2, None, None, sampler_type="Random", L_low=5, L_high=20,
                    cov_p=np.array([[1.0, 0.2], [0.2, 1.0]]), **kw)
    with pytest.raises(NotImplementedError):
        HMC_sampler(129, None, None, sampler_type="Random", L_low=5, L_high=20, Nchain=2, Niter=10, dt=0.1,
                    target=LogisticTarget(np.zeros((2, 129)), np.array([0.0, 1.0])))
    n = (1 << 20) + 1
    with pytest.raises(NotImplementedError):
        HMC_sampler(1, None, None, sampler_type="Random", L_low=5, L_high=20, Nchain=2, Niter=10, dt=0.1,
                    target=LogisticTarget(np.zeros((n, 1)), np.zeros(n)))

    def mvn():
        D = 10
        h = HMC_sampler(D, None, None, Nchain=16, Niter=20, sampler_type="Random", L_low=5, L_high=20, dt=0.1,
                        target=MVNTarget(np.zeros(D), np.diag(np.linspace(0.5, 2.0, D))), rng="philox", seed=4,
                        fp_mode="fast")
        h.gen_sample(np.random.RandomState(0).standard_normal((16, D)), verbose=False)
        return h

    def mixture():
        rs = np.random.RandomState(1)
        mix = MixtureTarget([0.4, 0.6], rs.standard_normal((2, 5)), rs.uniform(0.5, 2.0, (2, 5)))
        h = HMC_sampler(5, None, None, Nchain=16, Niter=20, sampler_type="Random", L_low=5, L_high=20, dt=0.3,
                        target=mix, rng="philox", seed=6)
        h.gen_sample(rs.standard_normal((16, 5)), verbose=False)
        return h

    before = mvn(), mixture()
    m = sampler(c, rng="philox", seed=1)
    m.gen_sample(c["q_start"], verbose=False)
    after = mvn(), mixture()
    for b, a_ in zip(before, after):
        for a in ("q_chain", "E_chain", "dE_chain", "_acc", "n_leapfrog"):
            assert np.array_equal(getattr(b, a), getattr(a_, a)), a


# ------------------------------------------------------------------------------------------ 12
def test_out_of_range_rejections_and_L_tallies():
    """A rejection at i < i_oob = warm_up - L_chain * thin = 11 writes q_chain row
    (i - warm_up) // thin < -L_chain in the reference (samplers.py:471), an IndexError.  The tallies
    of k_logit_iters over two launches, [1, 9) and [9, 21): the rejections before i_oob (from the
    oracle's replay of the same draws with warm_up = 1; the decisions do not depend on warm_up), sum L
    and sum L^2 equal the reference's, and HMC_sampler raises the reference's error."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import LogisticEngine
    c = recipe("oob")
    i_oob = c["wu"] - O.chain_len(c["Niter"], c["wu"], c["thin"])
    assert i_oob == 11
    dE = oracle_run(dict(c, wu=1))["dE_prop"][:, :i_oob - 1]
    n_oob = int(np.sum(~((dE < 0) | (c["lnu"][:, :i_oob - 1] < -dE))))
    assert 0 < n_oob < dE.size                          # the reference rejects there, but not always
    with pytest.raises(IndexError):
        oracle_run(c)
    eng = LogisticEngine(target_of(c), c["N"], c["Niter"], c["wu"], c["thin"], c["Llo"], c["Lhi"], c["dt"],
                         rng="replay")
    eng.set_replay(c["p0"], c["P"], c["L"], c["lnu"])
    eng.init(c["q_start"])
    eng.run(1, 9)
    eng.run(9, c["Niter"] + 1)
    torch.cuda.synchronize()
    cnt = eng.read_counters()
    L = c["L"].astype(np.int64)
    assert int(cnt[H.CNT_OOB_REJECT]) == n_oob
    assert int(cnt[H.CNT_LEAPFROG]) == int(L.sum()) and int(cnt[H.CNT_LEAPFROG_SQ]) == int((L * L).sum())
    with pytest.raises(IndexError):
        sampler(c).gen_sample(c["q_start"], verbose=False)
