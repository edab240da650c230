"""GLM targets on the GPU with the Random-trajectory sampler (csrc/hmc_logit.hip with the family as a
template parameter, the hmc_glm_* entries) against the CPU oracle.

The oracle target is tests/glm_cases.py::OracleGLM, written from the formulas and independent of
hmc_amd.target.  Every Poisson parity case first asserts, on the oracle alone, the conditions on its
INPUTS that tests/test_gpu_logistic.py sets (not tolerances on the kernel): (1) no Metropolis decision
within 1e-4 of flipping, (2) the oracle rerun from q_start (1 + 1e-13) moves q_chain by at most 1e-11,
(3) at least 2 and at most 60 % of the proposals rejected.  The seeds were chosen on the CPU so that the
oracle meets them."""
import functools

import numpy as np
import pytest
import torch

import glm_cases as G
from oracle import hmc_oracle as O
from philox_host import dense_momenta, host_L_lnu

pytestmark = pytest.mark.gpu

#        D    n    N  Niter wu thin L_low L_high c   seed dt_vec cov_p
CASES = {
    "A": (1, 1, 6, 30, 0, 1, 1, 6, 1.5, 1, False, False),           # D = 1, n = 1, L from 1
    "B": (2, 20, 5, 16, 4, 1, 5, 20, 1.3, 1, False, False),         # D < 4, ragged row tile
    "C": (17, 17, 16, 16, 5, 3, 5, 20, 1.1, 1, False, False),       # one over in D and n; exactly one chain tile
    "D": (37, 100, 4, 30, 7, 2, 5, 20, 0.8, 1, True, True),         # a dt vector and a diagonal cov_p
    "E": (65, 33, 33, 10, 3, 1, 5, 20, 0.8, 1, False, False),       # three chain tiles, last with one chain
    "F": (128, 100, 3, 10, 0, 1, 5, 12, 0.8, 1, False, False),      # ABI limit in D
}

# warm_up = 16 > L_chain * thin = 5: the reference raises IndexError
# (test_poisson_out_of_range_rejections_and_L_tallies); 19 chains are two tiles, the second with three
OOB_CASE = (3, 8, 19, 20, 16, 1, 5, 20, 1.5, 1, False, False)


def recipe(name, family="poisson", N=None, Niter=None):
    D, n, N_, Niter_, wu, thin, Llo, Lhi, cdt, seed, dtvec, covp = OOB_CASE if name == "oob" else CASES[name]
    N, Niter = N or N_, Niter or Niter_
    c = G.recipe(family, D, n, N, cdt, seed, dtvec=dtvec, covp=covp)
    rs = c["rs"]
    Z0 = rs.standard_normal((N, D))
    Z = rs.standard_normal((N, Niter, D))
    L = rs.randint(Llo, Lhi, size=(N, Niter)).astype(np.int32)
    lnu = np.log(rs.random_sample((N, Niter)))
    c.update(Niter=Niter, wu=wu, thin=thin, Llo=Llo, Lhi=Lhi, p0=Z0 * c["sd"], P=Z * c["sd"], L=L, lnu=lnu)
    return c


def oracle_run(c, q_start=None):
    core = G.RecordingCore(G.oracle_target(c), c["dt"], c["cov_p"])
    out = O.gen_sample_random(core, c["q_start"] if q_start is None else q_start, c["N"], c["Niter"], c["wu"],
                              c["thin"], c["Llo"], c["Lhi"], O.ReplayDraws(c["p0"], c["P"], c["L"], c["lnu"]))
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


def sampler(c, rng="replay", **kw):
    from hmc_amd.samplers import HMC_sampler
    args = dict(Nchain=c["N"], Niter=c["Niter"], thin_rate=c["thin"], warm_up_num=c["wu"], cov_p=c["cov_p"],
                sampler_type="Random", dt=c["dt"], L_low=c["Llo"], L_high=c["Lhi"], target=G.glm_target(c), rng=rng)
    args.update(kw)
    h = HMC_sampler(c["D"], None, None, **args)
    if rng == "replay":
        h.set_random_replay(c["p0"], c["P"], c["L"], c["lnu"])
    return h


def assert_run_matches(h, ref):
    """The bounds of tests/test_gpu_logistic.py::assert_run_matches."""
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.n_leapfrog == ref["n_leapfrog"] and h.N_total_steps == ref["N_total_steps"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)
    np.testing.assert_allclose(h.dE_chain[:, :, 0], ref["dE_chain"], rtol=1e-8, atol=1e-10)
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]


OUTPUTS = ("q_chain", "E_chain", "dE_chain", "_acc", "_acc_wu", "n_leapfrog", "N_total_steps")


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", ["B", "D", "G"])
def test_bernoulli_is_bit_identical_to_the_logistic_entries(name):
    """hmc_glm_* with family = BERNOULLI against hmc_logit_* on cases B, D and G of the logistic recipe
    (tests/test_gpu_logistic.py): the sampler's outputs and counters, the engine's raw counter block,
    and the two row-wise entries, all with array_equal."""
    import test_gpu_logistic as TL
    from hmc_amd.target import GLMTarget
    c = TL.recipe(name)
    runs = []
    for target in (TL.target_of(c), GLMTarget(c["X"], c["y"], "bernoulli", c["pv"])):
        h = TL.sampler(c, target=target)
        h.gen_sample(c["q_start"], verbose=False)
        runs.append(h)
    logit, glm = runs
    assert type(logit.engine).__name__ == "LogisticEngine" and type(glm.engine).__name__ == "GLMEngine"
    for a in OUTPUTS + ("accept_R", "accept_R_warm_up"):
        assert np.array_equal(getattr(glm, a), getattr(logit, a)), a
    assert torch.equal(glm.engine.counters, logit.engine.counters)
    assert torch.equal(glm.engine.q, logit.engine.q) and torch.equal(glm.engine.E_prev, logit.engine.E_prev)
    rs = np.random.RandomState(5)
    q, p = 0.5 * rs.standard_normal((40, c["D"])), rs.standard_normal((40, c["D"]))
    assert np.array_equal(glm.E(q, p), logit.E(q, p))
    for x, y in zip(glm.leap_frog(p, q), logit.leap_frog(p, q)):
        assert np.array_equal(x, y)
    ph = [TL.sampler(c, rng="philox", seed=8, target=t) for t in (TL.target_of(c),
                                                                   GLMTarget(c["X"], c["y"], "bernoulli", c["pv"]))]
    for h in ph:
        h.gen_sample(c["q_start"], verbose=False)
    for a in OUTPUTS:
        assert np.array_equal(getattr(ph[1], a), getattr(ph[0], a)), a


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("name", sorted(CASES))
def test_poisson_replay_parity(name):
    c, ref = case(name)
    check_input_conditions(c, ref)
    h = sampler(c, fp_mode="fast")
    h.gen_sample(c["q_start"], verbose=False)
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name", sorted(CASES))
def test_poisson_primitives_vs_oracle(name):
    """hmc_glm_energy / hmc_glm_leapfrog on 64 rows at 0.5 N(0, I), rtol 1e-10."""
    c = recipe(name)
    D = c["D"]
    rs = np.random.RandomState(1000 + D)
    q = 0.5 * rs.standard_normal((64, D))
    p = rs.standard_normal((64, D)) * c["sd"]
    h = sampler(c)
    core = O.HMCCore(G.oracle_target(c), c["dt"], c["cov_p"])
    E = h.E(q, p)
    E_ref = np.array([core.E(q[i], p[i]) for i in range(64)])
    np.testing.assert_allclose(E, E_ref, rtol=1e-10, atol=1e-12)
    pn, qn = h.leap_frog(p, q)
    ref = [core.leap_frog(p[i], q[i]) for i in range(64)]
    np.testing.assert_allclose(pn, [r[0] for r in ref], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(qn, [r[1] for r in ref], rtol=1e-10, atol=1e-12)
    e1, (p1, q1) = h.E(q[3], p[3]), h.leap_frog(p[3], q[3])          # single rows keep their shape
    assert np.ndim(e1) == 0 and p1.shape == (D,) and q1.shape == (D,)
    assert e1 == E[3] and np.array_equal(p1, pn[3]) and np.array_equal(q1, qn[3])


# ------------------------------------------------------------------------------------------ 4
def test_poisson_philox_parity():
    """The draws the kernel makes, regenerated on the host (tests/philox_host.py): the dense Random
    kernel's momenta (dims h + 4m) and block (0x80000000, it, chain) for (L, log u)."""
    seed, chain0 = 22, 5
    c = recipe("D", N=40, Niter=16)
    gcs = np.arange(chain0, chain0 + c["N"], dtype=np.uint64)
    p0, P = dense_momenta(seed, gcs, c["D"], c["Niter"])
    L, lnu = host_L_lnu(seed, gcs, c["Niter"], c["Llo"], c["Lhi"])
    c = dict(c, p0=p0 * c["sd"], P=P * c["sd"], L=L, lnu=lnu)
    ref = oracle_run(c)
    check_input_conditions(c, ref)
    h = sampler(c, rng="philox", seed=seed, chain_offset=chain0, fp_mode="fast")
    h.gen_sample(c["q_start"], verbose=False)
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 5
def test_poisson_layout_and_launch_invariance():
    """One launch against three, and shards [0, 40) + [40, 72): 40 is not a multiple of 16, so the
    second shard's chains sit in other tile columns than in the single run."""
    c = recipe("C", N=72, Niter=12)

    def run(q_start, **kw):
        h = sampler(dict(c, N=len(q_start)), rng="philox", seed=5, **kw)
        h.gen_sample(q_start, verbose=False)
        return h

    one = run(c["q_start"])
    split = run(c["q_start"], iters_per_launch=4)
    for a in OUTPUTS:
        assert np.array_equal(getattr(one, a), getattr(split, a)), a
    lo, hi = run(c["q_start"][:40], chain_offset=0), run(c["q_start"][40:], chain_offset=40)
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(one, a), np.concatenate([getattr(lo, a), getattr(hi, a)])), a
    for a in ("_acc", "_acc_wu", "n_leapfrog"):
        assert getattr(one, a) == getattr(lo, a) + getattr(hi, a), a


# ------------------------------------------------------------------------------------------ 6
def test_one_overflowing_chain_is_rejected_and_isolated():
    """Case B's chains with and without a sixteenth whose start has z > 709 in a data row: its
    exp(z) is +inf, so every energy of it is non-finite, every proposal is rejected and it stays put;
    its 15 neighbours in the tile equal the run without it, bit for bit."""
    c = recipe("B", N=15)
    good = c["q_start"]
    j = int(np.argmax(np.abs(c["X"][:, 0])))
    bad = np.zeros((1, c["D"]))
    bad[0, 0] = 800.0 / c["X"][j, 0]                      # z_j = 800
    assert (c["X"] @ bad[0]).max() > 709.78
    runs = []
    for qs in (good, np.concatenate([good, bad])):
        h = sampler(dict(c, N=len(qs)), rng="philox", seed=3)
        h.gen_sample(qs, verbose=False)
        runs.append(h)
    ok, mixed = runs
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(mixed, a)[:15], getattr(ok, a)), a
    assert np.all(mixed.q_chain[15] == bad[0])
    assert (mixed._acc, mixed._acc_wu) == (ok._acc, ok._acc_wu)        # every proposal of the bad chain rejected
    assert not np.any(np.isfinite(mixed.E_chain[15]))


# ------------------------------------------------------------------------------------------ 7
def test_poisson_out_of_range_rejections_and_L_tallies():
    """A rejection at i < i_oob = warm_up - L_chain * thin = 11 writes q_chain row
    (i - warm_up) // thin < -L_chain in the reference (samplers.py:471), an IndexError.  The tallies
    of the Poisson instance of k_logit_iters over two launches, [1, 9) and [9, 21): the rejections
    before i_oob (from the oracle's replay of the same draws with warm_up = 1; the decisions do not
    depend on warm_up), sum L and sum L^2 equal the reference's, and HMC_sampler raises the reference's
    error."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import GLMEngine
    c = recipe("oob")
    i_oob = c["wu"] - O.chain_len(c["Niter"], c["wu"], c["thin"])
    assert i_oob == 11
    dE = oracle_run(dict(c, wu=1))["dE_prop"][:, :i_oob - 1]
    n_oob = int(np.sum(~((dE < 0) | (c["lnu"][:, :i_oob - 1] < -dE))))
    assert 0 < n_oob < dE.size                          # the reference rejects there, but not always
    with pytest.raises(IndexError):
        oracle_run(c)
    eng = GLMEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["Llo"], c["Lhi"], c["dt"],
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
