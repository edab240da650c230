"""NUTS on GLM targets on the GPU (csrc/hmc_glm_nuts.hip, hmc_glm_nuts_iters) against the CPU oracle,
for both families.

The reference consumes its NUTS draws in a data-dependent order, so replay parity runs an explicit
per-chain tape drawn as in tests/test_gpu_nuts.py::test_nuts_matches_oracle, and Philox parity drives
the oracle with the host-regenerated streams of tests/philox_host.py.  The oracle target is
tests/glm_cases.py::OracleGLM, independent of hmc_amd.target.

Every parity case first asserts, on the oracle alone and before any GPU call, conditions on its INPUTS
(not tolerances on the kernel), and prints the figures:
  (a) rerunning from q_start (1 +- 1e-9) leaves n_leapfrog, n_unstable and n_dmax equal and moves
      q_chain by at most 1e-6: no tree decision sits within the kernel's error of flipping;
  (b) a (1 + 1e-13) perturbation moves q_chain by at most 1e-11;
  (c) at least one sub-tree rejected by a U-turn, and two different tree depths among the chains of one
      tile in one iteration;
  (d) no d_max hit, except in the cases built for it (compared exactly, on_dmax="break").
The seeds, step factors and prior scales were chosen on the CPU so that the oracle meets them."""
import functools

import numpy as np
import pytest
import torch

import glm_cases as G
from oracle import hmc_oracle as O
from philox_host import PhiloxNutsDraws, dense_momenta

pytestmark = pytest.mark.gpu

#  D    n    N  d_max Niter wu thin options (dt vector + diagonal cov_p)
SHAPES = {
    "D1": (1, 1, 5, 4, 12, 0, 1, False),
    "D2": (2, 20, 17, 5, 12, 4, 1, False),             # ragged last tile
    "D17": (17, 17, 16, 5, 10, 3, 2, False),           # one over a tile in D and n, exactly one chain tile
    "D37": (37, 100, 33, 6, 8, 2, 1, True),
    "D64": (64, 40, 4, 4, 6, 0, 1, False),             # exact tiles in D
    "D65": (65, 33, 18, 4, 6, 0, 1, False),
    "D128": (128, 100, 3, 3, 5, 0, 1, False),
}
# (family, shape) -> (prior scale pvs, step factor c, seed); glm_cases.recipe
TUNING = {
    ("poisson", "D1"): (1.0, 0.8, 1),
    ("poisson", "D2"): (1.0, 0.8, 2),
    ("poisson", "D17"): (0.2, 0.8, 5),
    ("poisson", "D37"): (0.2, 0.8, 2),
    ("poisson", "D64"): (0.2, 1.6, 3),
    ("poisson", "D65"): (0.03, 0.8, 7),
    ("poisson", "D128"): (0.01, 2.0, 1),
    ("bernoulli", "D1"): (1.0, 1.6, 2),
    ("bernoulli", "D2"): (1.0, 1.8, 1),
    ("bernoulli", "D17"): (0.2, 1.2, 3),
    ("bernoulli", "D37"): (1.0, 1.8, 3),
    ("bernoulli", "D64"): (0.2, 1.8, 1),
    ("bernoulli", "D65"): (0.03, 1.2, 2),
    ("bernoulli", "D128"): (0.03, 2.4, 1),
}
DMAX_CASES = ()          # (family, shape) whose oracle run hits d_max: compared with on_dmax="break"
FAMILIES = ("poisson", "bernoulli")


def nuts_case(family, name, N=None, Niter=None, d_max=None, cdt=None):
    """glm_cases.recipe, then p0, P and the tape from the same RandomState.  int(v) of a tape entry is a
    direction, v itself a uniform, as in tests/test_gpu_nuts.py."""
    D, n, N_, d_max_, Niter_, wu, thin, opts = SHAPES[name]
    pvs, c_, seed = TUNING[family, name]
    N, Niter, d_max = N or N_, Niter or Niter_, d_max or d_max_
    c = G.recipe(family, D, n, N, cdt or c_, seed, dtvec=opts, covp=opts, pvs=pvs)
    rs = c["rs"]
    c.update(d_max=d_max, Niter=Niter, wu=wu, thin=thin)
    c["p0"] = rs.standard_normal((N, D)) * c["sd"]
    c["P"] = rs.standard_normal((N, Niter, D)) * c["sd"]
    c["tape"] = rs.uniform(0.0, 2.0, (N, Niter * 2 * (2 ** d_max + d_max + 2)))
    return c


def oracle_run(c, q_start=None, draws=None, on_dmax="break"):
    core = O.HMCCore(G.oracle_target(c), c["dt"], c["cov_p"])
    dr = draws() if draws else G.TapeDraws(c["p0"], c["P"], c["tape"])
    out = O.gen_sample_nuts(core, c["q_start"] if q_start is None else q_start, c["N"], c["Niter"], c["wu"],
                            c["thin"], c["d_max"], dr, on_dmax=on_dmax)
    out["depth"], out["rejected"] = G.tree_stats(dr.shapes)
    return out


def counts(r):
    return r["n_leapfrog"], r["n_unstable"], r["n_dmax"]


def check_input_conditions(c, ref, draws=None, dmax_case=False):
    """(a)-(d) of the module docstring; prints each figure before asserting it."""
    moved = 0.0
    for s in (1 + 1e-9, 1 - 1e-9):
        r = oracle_run(c, c["q_start"] * s, draws)
        assert counts(r) == counts(ref), (s, counts(r), counts(ref))
        moved = max(moved, np.abs(r["q_chain"] - ref["q_chain"]).max())
    sens = np.abs(oracle_run(c, c["q_start"] * (1 + 1e-13), draws)["q_chain"] - ref["q_chain"]).max()
    uturn = ref["rejected"] - ref["n_unstable"]
    dep = ref["depth"]
    mixed = any(len(set(dep[t:t + 16, i])) > 1 for t in range(0, c["N"], 16) for i in range(dep.shape[1]))
    print("counts %s  moved(1e-9) %.3g  sensitivity(1e-13) %.3g  U-turn rejections %d  depths %d..%d mixed %s"
          % (counts(ref), moved, sens, uturn, dep.min(), dep.max(), mixed))
    assert moved <= 1e-6
    assert sens <= 1e-11
    assert uturn >= 1 and mixed
    assert (ref["n_dmax"] > 0) == dmax_case


@functools.lru_cache(maxsize=None)
def case(family, name):
    c = nuts_case(family, name)
    return c, oracle_run(c)


def sampler(c, rng="replay", **kw):
    from hmc_amd.samplers import HMC_sampler
    args = dict(Nchain=c["N"], Niter=c["Niter"], thin_rate=c["thin"], warm_up_num=c["wu"], cov_p=c["cov_p"],
                sampler_type="NUTS", dt=c["dt"], d_max=c["d_max"], target=G.glm_target(c), rng=rng)
    args.update(kw)
    h = HMC_sampler(c["D"], None, None, **args)
    if rng == "replay":
        h.set_nuts_replay(c["p0"], c["P"], c["tape"])
    return h


def assert_run_matches(h, ref):
    """Exact counts; the array bounds of tests/test_gpu_nuts.py::test_nuts_matches_oracle."""
    assert (h.n_leapfrog, h.n_unstable, h.n_dmax) == counts(ref)
    assert h.N_total_steps == ref["N_total_steps"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(h.dE_chain[:, :, 0], ref["dE_chain"], rtol=1e-8, atol=1e-9)
    assert h.accept_R == 1.0


OUTPUTS = ("q_chain", "E_chain", "dE_chain", "n_leapfrog", "n_unstable", "n_dmax", "N_total_steps")


# ------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("family", FAMILIES)
def test_replay_parity(family, name):
    c, ref = case(family, name)
    dmax_case = (family, name) in DMAX_CASES
    check_input_conditions(c, ref, dmax_case=dmax_case)
    h = sampler(c)
    h.gen_sample_NUTS(c["q_start"], 0, False, on_dmax="break" if dmax_case else "raise")
    assert_run_matches(h, ref)
    from hmc_amd import _lib as H
    cnt = h.engine.read_counters()
    assert cnt[H.CNT_HANDOFF_GIVEUP] == 0 and cnt[H.CNT_ENERGY_EVALS] == cnt[H.CNT_LEAPFROG]
    assert 0 < cnt[H.CNT_LEAPFROG] <= 16 * cnt[H.CNT_LEAPFROG_SQ]       # wave steps: lane utilisation <= 1


# ------------------------------------------------------------------------------------------ 2
PHILOX_SEEDS = {("poisson", "D2"): 31, ("poisson", "D37"): 33, ("poisson", "D65"): 35,
                ("bernoulli", "D2"): 31, ("bernoulli", "D37"): 35, ("bernoulli", "D65"): 31}


@pytest.mark.parametrize("name", ["D2", "D37", "D65"])
@pytest.mark.parametrize("family", FAMILIES)
def test_philox_parity(family, name):
    """HMC_sampler(rng="philox") against the oracle driven by PhiloxNutsDraws + dense_momenta: a
    non-zero chain_offset, a ragged N and three launches."""
    seed, chain0 = PHILOX_SEEDS[family, name], 7
    c = nuts_case(family, name, Niter=6)
    gcs = np.arange(chain0, chain0 + c["N"], dtype=np.uint64)
    p0, P = dense_momenta(seed, gcs, c["D"], c["Niter"])
    c = dict(c, p0=p0 * c["sd"], P=P * c["sd"])

    class Draws(G.TreeShape, PhiloxNutsDraws):
        def __init__(self):
            PhiloxNutsDraws.__init__(self, seed, c["p0"], c["P"], gcs)
            self._init_shapes(c["N"])

    ref = oracle_run(c, draws=Draws)
    check_input_conditions(c, ref, draws=Draws)
    h = sampler(c, rng="philox", seed=seed, chain_offset=chain0, iters_per_launch=2)
    h.gen_sample(c["q_start"], verbose=False)
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("family", FAMILIES)
def test_launch_shard_and_neighbour_invariance(family):
    """Bit-identical: iters_per_launch 1 against all; two shards [0, 24) + [24, 40) against one call (24
    is no multiple of 16: the second shard's chains sit in other tile columns); and chain 19's results
    with 15 other neighbours, itself in column 9 instead of 3."""
    c = nuts_case(family, "D17", N=40, Niter=6, d_max=8)     # Philox draws: room above the tuned d_max

    def run(q_start, **kw):
        h = sampler(dict(c, N=len(q_start)), rng="philox", seed=5, **kw)
        h.gen_sample(q_start, verbose=False)
        return h

    one = run(c["q_start"])
    split = run(c["q_start"], iters_per_launch=1)
    for a in OUTPUTS:
        assert np.array_equal(getattr(one, a), getattr(split, a)), a
    lo, hi = run(c["q_start"][:24], chain_offset=0), run(c["q_start"][24:], chain_offset=24)
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(one, a), np.concatenate([getattr(lo, a), getattr(hi, a)])), a
    for a in ("n_leapfrog", "n_unstable", "n_dmax"):
        assert getattr(one, a) == getattr(lo, a) + getattr(hi, a), a
    # global chain 19 (column 3 of the second tile above) as local chain 9 of a tile of global chains
    # 10 .. 25 whose 15 other start points are new
    other = 0.5 * np.random.RandomState(8).standard_normal((16, c["D"])) * np.sqrt(c["pv"])
    other[9] = c["q_start"][19]
    moved = run(other, chain_offset=10)
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(moved, a)[9], getattr(one, a)[19]), a
        assert not np.array_equal(getattr(moved, a)[8], getattr(one, a)[18]), a


# ------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("family", FAMILIES)
def test_unstable_step(family):
    """A dt large enough that the oracle reports n_unstable > 0 (|E - E_init| > 1000): counts equal."""
    c = nuts_case(family, "D17", N=8, Niter=5, cdt={"poisson": 1.8, "bernoulli": 6.0}[family])
    ref = oracle_run(c)
    print("counts", counts(ref))
    assert ref["n_unstable"] > 0
    h = sampler(c)
    assert np.all(np.isfinite(ref["q_chain"])) and np.all(np.isfinite(ref["E_chain"]))
    h.gen_sample_NUTS(c["q_start"], 0, False, on_dmax="break")
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("family", FAMILIES)
def test_d_max_reached(family):
    """d_max = 2 with a small step: on_dmax="raise" -> AssertionError after the run, "break" -> the
    count equals the oracle's and the chains keep their current samples."""
    c = nuts_case(family, "D2", N=6, Niter=5, d_max=2, cdt=0.2)
    ref = oracle_run(c)
    assert ref["n_dmax"] > 0
    with pytest.raises(AssertionError):
        O.gen_sample_nuts(O.HMCCore(G.oracle_target(c), c["dt"], c["cov_p"]), c["q_start"], c["N"], c["Niter"],
                          c["wu"], c["thin"], c["d_max"], O.ReplayDraws(c["p0"], c["P"], tape=c["tape"].copy()))
    with pytest.raises(AssertionError):
        sampler(c).gen_sample_NUTS(c["q_start"], 0, False, on_dmax="raise")
    h = sampler(c)
    h.gen_sample_NUTS(c["q_start"], 0, False, on_dmax="break")
    assert_run_matches(h, ref)


# ------------------------------------------------------------------------------------------ 6
def test_tape_exhaustion_and_replay_without_a_tape():
    c, _ = case("poisson", "D2")
    h = sampler(dict(c, tape=c["tape"][:, :3]))
    with pytest.raises(IndexError):
        h.gen_sample(c["q_start"], verbose=False)
    from hmc_amd.samplers import HMC_sampler
    g = HMC_sampler(c["D"], None, None, Nchain=c["N"], Niter=c["Niter"], sampler_type="NUTS", dt=c["dt"],
                    d_max=8, target=G.glm_target(c), rng="replay")
    np.random.seed(4)
    with pytest.warns(UserWarning, match="set_nuts_replay"):
        g.gen_sample(c["q_start"], verbose=False)
    assert g.n_leapfrog > 0 and np.all(np.isfinite(g.q_chain))


# ------------------------------------------------------------------------------------------ 7
def glm_nuts_engine(c, **kw):
    from hmc_amd.engine import GLMNutsEngine
    return GLMNutsEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["d_max"], c["dt"],
                         cov_p=c["cov_p"], rng="philox", seed=11, **kw)


def test_window_storage_and_store_chain_false():
    """Every row into a circular window of R rows over 4 launches: the window holds the last R rows of
    a stored run, bitwise; without a q_chain (q_chain == NULL) the final q is the stored run's last row."""
    c = nuts_case("poisson", "D17", N=24, Niter=12, d_max=8)
    c = dict(c, wu=1, thin=1)
    R = 4
    full = glm_nuts_engine(c)
    full.init(c["q_start"])
    full.run(1, c["Niter"] + 1)
    eng = glm_nuts_engine(c, store_chain=False)
    win = torch.zeros((c["N"], R, c["D"]), dtype=torch.float64, device=eng.device)
    eng.set_chain_window(win, 0)
    eng.init(c["q_start"])
    for k in range(4):
        eng.run(1 + 3 * k, 4 + 3 * k)
    bare = glm_nuts_engine(c, store_chain=False)
    bare.init(c["q_start"])
    bare.run(1, c["Niter"] + 1)
    torch.cuda.synchronize()
    rows = full.q_chain.shape[1]
    assert rows == 12 and rows % R == 0
    assert torch.equal(win, full.q_chain[:, rows - R:])
    assert torch.equal(eng.E_chain, full.E_chain) and torch.equal(eng.q, full.q)
    assert np.array_equal(eng.read_counters()[[2, 5, 6, 7]], full.read_counters()[[2, 5, 6, 7]])
    assert bare.q_chain is None and torch.equal(bare.q, full.q_chain[:, -1])
    assert torch.equal(bare.E_chain, full.E_chain)


def test_sampler_store_chain_false():
    c = nuts_case("bernoulli", "D2", Niter=24, d_max=8)
    out = []
    for store in (True, False):
        h = sampler(dict(c, wu=4), rng="philox", seed=22, store_chain=store, iters_per_launch=6)
        h.gen_sample(c["q_start"], verbose=False)
        out.append(h)
    full, st = out
    assert st.q_chain is None and st.n_leapfrog == full.n_leapfrog
    assert np.array_equal(st.q_device.cpu().numpy(), full.q_chain[:, -1])


# ------------------------------------------------------------------------------------------ 8
def test_non_finite_poisson_chain_is_unstable_and_isolated():
    """D = 1, n = 1, sixteen chains in one tile.  Chain 9 starts at z = x q = -1000 with, in every
    iteration, a momentum that moves z by about +900 per leapfrog, and a tape that sends its first
    doubling to the left (a finite point, refused by a uniform >= 1) and its second to the right: that
    sub-tree's first point (z ~ -135) is finite, its second has z ~ 806 > 709.78, exp(z) = +inf and
    V = +inf, which |E - E_init| > 1000 counts as unstable.  The chain keeps its sample in every
    iteration, and its 15 neighbours equal a run with a tame chain 9 in its place, bit for bit."""
    c = nuts_case("poisson", "D1", N=16, Niter=6)
    x, dt = c["X"][0, 0], c["dt"]
    core = O.HMCCore(G.oracle_target(c), dt, None)
    q0, pbig = np.array([-1000.0 / x]), np.array([580.0 / (x * dt)])
    p1, q1 = core.leap_frog(pbig, q0)
    p2, q2 = core.leap_frog(p1, q1)
    pl, ql = core.leap_frog(-pbig, q0)
    print("z:", x * q0, x * q1, x * q2, "left", x * ql, "E:", core.E(q0, pbig), core.E(q1, p1), core.E(q2, p2))
    assert x * q1[0] < -30 and np.isfinite(core.E(q1, p1)) and np.isfinite(core.E(ql, pl))
    assert x * q2[0] > 720 and core.E(q2, p2) == np.inf
    qs, P, tape = c["q_start"].copy(), c["P"].copy(), c["tape"].copy()
    qs[9], P[9] = q0, pbig
    tape[9] = np.tile([1.5, 1.5, 0.5], tape.shape[1] // 3 + 1)[:tape.shape[1]]    # left, refuse, right
    bad = dict(c, q_start=qs, P=P, tape=tape)
    ref, ref_ok = oracle_run(bad), oracle_run(c)
    print("counts", counts(ref), "with a tame chain 9", counts(ref_ok))
    assert ref["n_dmax"] == ref_ok["n_dmax"] == 0
    assert ref["n_unstable"] == ref_ok["n_unstable"] + c["Niter"]           # once per iteration
    assert np.all(ref["q_chain"][9] == q0) and np.all(np.isfinite(ref["E_chain"][9]))
    runs = []
    for cc in (c, bad):
        h = sampler(cc)
        h.gen_sample_NUTS(cc["q_start"], 0, False, on_dmax="raise")
        runs.append(h)
    ok, mixed = runs
    keep = np.arange(16) != 9
    for a in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(mixed, a)[keep], getattr(ok, a)[keep]), a
    assert np.all(mixed.q_chain[9] == q0)
    assert_run_matches(mixed, ref)


# ------------------------------------------------------------------------------------------ 9
def test_small_ensemble_against_the_oracle():
    """Poisson, D = 2, n = 20.  GPU Philox NUTS: 8,192 chains, 20 iterations (40 take the oracle side
    16 s on the CPU, 20 take 7 s), last sample per chain; oracle gen_sample_nuts with LiveDraws: 512
    chains, the same settings.  Per-dimension means agree
    within 5 sd sqrt(1/512 + 1/8192), sd from the GPU sample: a two-sample 5-sigma bound."""
    NG, NO, Niter = 8192, 512, ENSEMBLE_NITER
    c = nuts_case("poisson", "D2")
    rs = np.random.RandomState(77)
    qg, qo = 0.5 * rs.standard_normal((NG, 2)), 0.5 * rs.standard_normal((NO, 2))
    h = sampler(dict(c, N=NG, Niter=Niter, wu=0, d_max=8), rng="philox", seed=3)
    h.gen_sample(qg, verbose=False)
    assert h.n_dmax == 0
    x = h.q_chain[:, -1]
    np.random.seed(12)
    ref = O.gen_sample_nuts(O.HMCCore(G.oracle_target(c), c["dt"], None), qo, NO, Niter, 0, 1, 8,
                            O.LiveDraws(2, np.eye(2)))
    y = ref["q_chain"][:, -1]
    sd = x.std(axis=0, ddof=1)
    z = (x.mean(axis=0) - y.mean(axis=0)) / (sd * np.sqrt(1 / NO + 1 / NG))
    print("means GPU", x.mean(axis=0), "oracle", y.mean(axis=0), "sd", sd, "z", z)
    assert np.all(np.abs(z) <= 5)


ENSEMBLE_NITER = 20
