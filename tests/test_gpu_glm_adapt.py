"""Per-chain step-size adaptation on the GLM targets on the GPU (the ADAPT forms of the kernels of
csrc/hmc_logit.hip and csrc/hmc_glm_nuts.hip behind hmc_glm_random_iters_adapt /
hmc_glm_nuts_iters_adapt) against the plain entries and against the CPU model tests/adapt_model.py.

  frozen identity   step_scale0 = 1 without adapt_step, and adapt_step with warm_up_num 0 and 1 (no
                    iteration adapts), through the _adapt entries against the plain entries: bitwise.
  replay parity     adaptive runs against the model, with the exact counts and the array bounds of the
                    plain parity tests, step_scale and state slots 0-3 to rtol 1e-9.
  Philox parity     the same against the model driven by the host-regenerated Philox streams.
  invariance        launch split, shards, tile column / neighbours, save and restore inside warm-up:
                    bitwise, step_scale and the state array included.
  ensemble          8,192 GPU chains against 128 model chains: means of log(step_scale) and of the
                    post-warm-up acceptance statistic within a two-sample 5-sigma bound.

Every parity case first asserts, on the model alone and before any GPU call, conditions on its INPUTS
(not tolerances on the kernel), and prints the figures:
  (a) q_chain is finite;
  (b) rerunning from q_start (1 +- 1e-9) leaves the counts equal and moves q_chain by at most 1e-6;
  (c) a (1 + 1e-13) start moves q_chain by at most 1e-11 and step_scale by at most 1e-11;
  (d) NUTS: at least one sub-tree rejected by a U-turn and two tree depths within one tile;
  (e) the clamp of log_s is never reached;
  (f) step_scale ends outside [0.9, 1.1] for at least half the chains: the adaptation did something.
The seeds, step factors and prior scales were chosen on the CPU so that the model meets them."""
import functools

import numpy as np
import pytest
import torch

import adapt_model as A
import glm_cases as G
import test_gpu_glm as TG
import test_gpu_glm_nuts as TN
from oracle import hmc_oracle as O
from philox_host import PhiloxNutsDraws, dense_momenta, host_L_lnu

pytestmark = pytest.mark.gpu

FAMILIES = ("poisson", "bernoulli")
KINDS = ("NUTS", "Random")
DELTA = 0.8
WU, DMAX, LLO, LHI = 8, 7, 5, 20
# Random: 15 iterations, not 12.  The reference writes a proposal rejected in warm-up iteration i to row
# (i - warm_up) // thin < 0 of q_chain and raises IndexError when that is below -L_chain (Q5): with
# warm_up = 8, L_chain = 1 + (Niter - 8) // thin must be at least 7 (thin 1) or 4 (thin 2) for any
# rejection in iteration 1 to be legal, and the adaptation's first steps are where rejections are.
NITER = {"NUTS": 12, "Random": 15}
#        D    n    N  thin  dt vector + diagonal cov_p
SHAPES = {
    "D1": (1, 1, 5, 1, False),
    "D17": (17, 17, 16, 2, False),            # exactly one chain tile; thin = 2
    "D37": (37, 100, 8, 1, True),             # the multiplier composes with a dt vector and a cov_p
    "D65": (65, 33, 18, 1, False),            # ragged chain tile
    "D128": (128, 100, 3, 1, False),          # the spilling MT = 8 instance
}
# (kind, family, shape) -> (prior scale pvs, step factor c, seed); glm_cases.recipe
TUNING = {
    ("NUTS", "poisson", "D1"): (1.0, 0.5, 4),
    ("NUTS", "poisson", "D17"): (0.2, 0.5, 1),
    ("NUTS", "poisson", "D37"): (0.2, 0.5, 3),
    ("NUTS", "poisson", "D65"): (0.03, 0.5, 1),
    ("NUTS", "poisson", "D128"): (0.01, 0.5, 2),
    ("NUTS", "bernoulli", "D1"): (1.0, 0.25, 2),
    ("NUTS", "bernoulli", "D17"): (0.2, 0.5, 1),
    ("NUTS", "bernoulli", "D37"): (0.01, 0.5, 4),
    ("NUTS", "bernoulli", "D65"): (0.03, 0.5, 1),
    ("NUTS", "bernoulli", "D128"): (0.03, 0.5, 1),
    ("Random", "poisson", "D1"): (1.0, 0.5, 1),
    ("Random", "poisson", "D17"): (0.06, 2.2, 3),
    ("Random", "poisson", "D37"): (0.2, 0.5, 2),
    ("Random", "poisson", "D65"): (0.03, 0.5, 4),
    ("Random", "poisson", "D128"): (0.01, 0.5, 2),
    ("Random", "bernoulli", "D1"): (1.0, 0.5, 2),
    ("Random", "bernoulli", "D17"): (0.2, 0.5, 6),
    ("Random", "bernoulli", "D37"): (1.0, 0.5, 1),
    ("Random", "bernoulli", "D65"): (0.009, 0.7, 6),
    ("Random", "bernoulli", "D128"): (0.03, 0.5, 1),
}


def make_case(kind, family, name, N=None, Niter=None, wu=WU, tuning=None, d_max=DMAX):
    D, n, N_, thin, opts = SHAPES[name]
    pvs, cdt, seed = tuning or TUNING[kind, family, name]
    N, Niter = N or N_, Niter or NITER[kind]
    c = G.recipe(family, D, n, N, cdt, seed, dtvec=opts, covp=opts, pvs=pvs)
    rs = c["rs"]
    c.update(kind=kind, d_max=d_max, Niter=Niter, wu=wu, thin=thin, Llo=LLO, Lhi=LHI)
    c["p0"] = rs.standard_normal((N, D)) * c["sd"]
    c["P"] = rs.standard_normal((N, Niter, D)) * c["sd"]
    if kind == "NUTS":
        c["tape"] = rs.uniform(0.0, 2.0, (N, Niter * 2 * (2 ** d_max + d_max + 2)))
    else:
        c["L"] = rs.randint(LLO, LHI, size=(N, Niter)).astype(np.int32)
        c["lnu"] = np.log(rs.random_sample((N, Niter)))
    return c


def model_run(c, q_start=None, draws=None, s0=None, adapt_end=None):
    qs = c["q_start"] if q_start is None else q_start
    adapt_end = c["wu"] if adapt_end is None else adapt_end
    if c["kind"] == "NUTS":
        dr = draws() if draws else G.TapeDraws(c["p0"], c["P"], c["tape"])
        out = A.nuts_adaptive(G.oracle_target(c), c["dt"], c["cov_p"], qs, c["Niter"], c["wu"], c["thin"], c["d_max"],
                              dr, adapt_end, DELTA, s0)
        out["depth"], out["rejected"] = G.tree_stats(dr.shapes)
        out["accept_R"] = 1.0
        return out
    dr = draws() if draws else O.ReplayDraws(c["p0"], c["P"], c["L"], c["lnu"])
    return A.random_adaptive(G.oracle_target(c), c["dt"], c["cov_p"], qs, c["Niter"], c["wu"], c["thin"], c["Llo"],
                             c["Lhi"], dr, adapt_end, DELTA, s0)


def counts(c, r):
    if c["kind"] == "NUTS":
        return r["n_leapfrog"], r["n_unstable"], r["n_dmax"]
    return r["accept_count"], r["accept_count_warm_up"], r["n_leapfrog"]


def input_figures(c, ref, draws=None):
    """The figures of conditions (a)-(f) of the module docstring, on the model alone."""
    f = dict(finite=bool(np.all(np.isfinite(ref["q_chain"])) and np.all(np.isfinite(ref["state"]))))
    f["moved"], f["counts_equal"] = 0.0, True
    for s in (1 + 1e-9, 1 - 1e-9):
        r = model_run(c, c["q_start"] * s, draws)
        f["counts_equal"] &= counts(c, r) == counts(c, ref)
        f["moved"] = max(f["moved"], np.abs(r["q_chain"] - ref["q_chain"]).max())
    r = model_run(c, c["q_start"] * (1 + 1e-13), draws)
    f["sens"] = np.abs(r["q_chain"] - ref["q_chain"]).max()
    f["sens_scale"] = np.abs(r["step_scale"] - ref["step_scale"]).max()
    if c["kind"] == "NUTS":
        dep = ref["depth"]
        f["uturn"] = ref["rejected"] - ref["n_unstable"]
        f["mixed"] = any(len(set(dep[t:t + 16, i])) > 1 for t in range(0, c["N"], 16) for i in range(dep.shape[1]))
    f["clamped"] = ref["clamped"]
    f["adapted"] = float(np.mean((ref["step_scale"] < 0.9) | (ref["step_scale"] > 1.1)))
    return f


def check_input_conditions(c, ref, draws=None):
    f = input_figures(c, ref, draws)
    print("counts %s  %s  step_scale %.3g..%.3g" % (counts(c, ref), f, ref["step_scale"].min(),
                                                    ref["step_scale"].max()))
    assert f["finite"]
    assert f["counts_equal"] and f["moved"] <= 1e-6
    assert f["sens"] <= 1e-11 and f["sens_scale"] <= 1e-11
    if c["kind"] == "NUTS":
        assert f["uturn"] >= 1 and f["mixed"]
    assert not f["clamped"]
    assert f["adapted"] >= 0.5


def sampler(c, rng="replay", **kw):
    """tests/test_gpu_glm_nuts.py::sampler / tests/test_gpu_glm.py::sampler on the case's streams."""
    return (TN.sampler if c["kind"] == "NUTS" else TG.sampler)(c, rng=rng, **kw)


def run(c, q_start=None, rng="replay", **kw):
    h = sampler(c, rng=rng, **kw)
    qs = c["q_start"] if q_start is None else q_start
    if c["kind"] == "NUTS":
        h.gen_sample_NUTS(qs, 0, False, on_dmax="break")
    else:
        h.gen_sample(qs, verbose=False)
    return h


def assert_run_matches(c, h, ref):
    """The exact counts and array bounds of the plain parity tests, then the adaptation's own outputs."""
    (TN if c["kind"] == "NUTS" else TG).assert_run_matches(h, ref)
    print("step_scale GPU %s\n           model %s" % (h.step_scale, ref["step_scale"]))
    np.testing.assert_allclose(h.step_scale, ref["step_scale"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(h.adapt_state[:, :4], ref["state"][:, :4], rtol=1e-9, atol=0)
    assert np.array_equal(h.adapt_state[:, 3], ref["state"][:, 3]) and np.array_equal(h.adapt_state[:, 7],
                                                                                       ref["state"][:, 7])
    np.testing.assert_allclose(h.adapt_state[:, 4:7], ref["state"][:, 4:7], rtol=1e-9, atol=1e-12)
    n_ad, n_af = ref["state"][:, 3].sum(), ref["state"][:, 7].sum()
    np.testing.assert_allclose(h.accept_stat_warm_up, ref["state"][:, 5].sum() / n_ad, rtol=1e-9)
    np.testing.assert_allclose(h.accept_stat, ref["state"][:, 6].sum() / n_af, rtol=1e-9)


OUTPUTS = {"NUTS": TN.OUTPUTS, "Random": TG.OUTPUTS}


def assert_bitwise(kind, a, b, adapt=True, same_launches=True):
    for name in OUTPUTS[kind] + (("step_scale", "adapt_state") if adapt else ()):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.q_device, b.q_device)
    ca, cb = a.engine.read_counters(), b.engine.read_counters()
    if kind == "NUTS" and not same_launches:       # LEAPFROG_SQ counts the NUTS kernel's wave steps, which
        ca[3] = cb[3] = 0                          # depend on the launch split (include/hmc.h); no result does
    assert np.array_equal(ca, cb)


# ------------------------------------------------------------------------------------------ c
def frozen_case(kind, family, name):
    """The plain NUTS parity case of that shape; for the Random sampler the same inputs with a
    trajectory-length and a log-uniform stream."""
    c = TN.nuts_case(family, name)
    c["kind"] = kind
    if kind == "Random":
        rs = np.random.RandomState(7)
        c.update(Llo=LLO, Lhi=LHI, L=rs.randint(LLO, LHI, size=(c["N"], c["Niter"])).astype(np.int32),
                 lnu=np.log(rs.random_sample((c["N"], c["Niter"]))))
    return c


@pytest.mark.parametrize("name", ["D1", "D17", "D65", "D128"])
@pytest.mark.parametrize("rng", ["replay", "philox"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_identity(kind, family, rng, name):
    c = frozen_case(kind, family, name)
    kw = dict(seed=9, chain_offset=3) if rng == "philox" else {}
    plain = run(c, rng=rng, **kw)
    assert plain.step_scale is None and plain.adapt_state is None
    frozen = run(c, rng=rng, step_scale0=1.0, **kw)
    assert type(frozen.engine) is type(plain.engine) and frozen.engine._adapt is not None
    assert_bitwise(kind, frozen, plain, adapt=False)
    assert np.all(frozen.step_scale == 1.0) and np.all(frozen.adapt_state[:, :5] == 0.0)
    assert np.all(frozen.adapt_state[:, 7] == c["Niter"]) and frozen.accept_stat_warm_up is None
    assert 0.0 < frozen.accept_stat <= 1.0
    for wu in (0, 1):                                   # adapt_step with no iteration 1 <= i < warm_up
        cw = dict(c, wu=wu)
        base = plain if wu == c["wu"] else run(cw, rng=rng, **kw)
        ad = run(cw, rng=rng, adapt_step=True, **kw)
        assert ad.engine._adapt.adapt_end == wu
        assert_bitwise(kind, ad, base, adapt=False)
        assert np.all(ad.step_scale == 1.0) and np.all(ad.adapt_state[:, 3] == 0.0)


# ------------------------------------------------------------------------------------------ d
@functools.lru_cache(maxsize=None)
def parity_case(kind, family, name):
    c = make_case(kind, family, name)
    return c, model_run(c)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_replay_parity(kind, family, name):
    """12 (NUTS) or 15 (Random) iterations, warm_up_num 8, d_max 7, launches of 5: the adaptation ends
    inside the second."""
    c, ref = parity_case(kind, family, name)
    check_input_conditions(c, ref)
    h = run(c, adapt_step=True, adapt_delta=DELTA, iters_per_launch=5)
    assert_run_matches(c, h, ref)
    assert np.all(h.adapt_state[:, 3] == WU - 1) and np.all(h.adapt_state[:, 7] == NITER[kind] - WU + 1)


# ------------------------------------------------------------------------------------------ e
# (kind, family) -> (prior scale, step factor, recipe seed, Philox seed)
PHILOX_TUNING = {
    ("NUTS", "poisson"): (0.06, 0.5, 1, 31),
    ("NUTS", "bernoulli"): (0.03, 0.45, 1, 31),
    ("Random", "poisson"): (0.2, 0.5, 1, 31),
    ("Random", "bernoulli"): (1.0, 0.5, 1, 31),
}


PHILOX_CHAIN0 = 7


def philox_case(kind, family, tuning):
    """The D37 case with the draws the kernels make for global chains 7 .. 7 + N - 1 under Philox seed
    `seed`, regenerated on the host; (case, draw-source factory or None)."""
    pvs, cdt, case_seed, seed = tuning
    c = make_case(kind, family, "D37", tuning=(pvs, cdt, case_seed))
    gcs = np.arange(PHILOX_CHAIN0, PHILOX_CHAIN0 + c["N"], dtype=np.uint64)
    p0, P = dense_momenta(seed, gcs, c["D"], c["Niter"])
    c = dict(c, p0=p0 * c["sd"], P=P * c["sd"], philox_seed=seed)
    if kind == "Random":
        L, lnu = host_L_lnu(seed, gcs, c["Niter"], c["Llo"], c["Lhi"])
        return dict(c, L=L, lnu=lnu), None

    class Draws(G.TreeShape, PhiloxNutsDraws):
        def __init__(self):
            PhiloxNutsDraws.__init__(self, seed, c["p0"], c["P"], gcs)
            self._init_shapes(c["N"])
    return c, Draws


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_philox_parity(kind, family):
    """D37 against the model driven by the host-regenerated streams (tests/philox_host.py): a non-zero
    chain_offset and three launches."""
    c, Draws = philox_case(kind, family, PHILOX_TUNING[kind, family])
    seed, chain0 = c["philox_seed"], PHILOX_CHAIN0
    ref = model_run(c, draws=Draws)
    check_input_conditions(c, ref, draws=Draws)
    h = run(c, rng="philox", seed=seed, chain_offset=chain0, adapt_step=True, adapt_delta=DELTA, iters_per_launch=5)
    assert_run_matches(c, h, ref)


# ------------------------------------------------------------------------------------------ f
def invariance_case(kind, family):
    """40 chains at D17, warm_up_num 7; 10 iterations (NUTS) or 14 (Random: L_chain = 8, so that a
    rejection in the first warm-up iteration is a legal row of the reference, see NITER)."""
    c = TN.nuts_case(family, "D17", N=40, Niter={"NUTS": 10, "Random": 14}[kind], d_max=8)   # d_max: room for Philox draws
    return dict(c, kind=kind, wu=7, thin=1, Llo=LLO, Lhi=LHI)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_launch_shard_and_neighbour_invariance(kind, family):
    """Bit-identical, step_scale and the state array included: iters_per_launch 1 against one launch;
    two shards [0, 24) + [24, 40) against one call; and global chain 19 with 15 other neighbours, in
    tile column 9 instead of 3."""
    c = invariance_case(kind, family)

    def go(q_start, **kw):
        return run(dict(c, N=len(q_start)), q_start, rng="philox", seed=5, adapt_step=True, **kw)

    one = go(c["q_start"])
    assert np.all(one.step_scale != 1.0) and np.all(one.adapt_state[:, 3] == c["wu"] - 1)   # every chain adapted
    assert_bitwise(kind, go(c["q_start"], iters_per_launch=1), one, same_launches=False)
    lo, hi = go(c["q_start"][:24], chain_offset=0), go(c["q_start"][24:], chain_offset=24)
    for a in ("q_chain", "E_chain", "dE_chain", "step_scale", "adapt_state"):
        assert np.array_equal(getattr(one, a), np.concatenate([getattr(lo, a), getattr(hi, a)])), a
    assert one.n_leapfrog == lo.n_leapfrog + hi.n_leapfrog
    other = 0.5 * np.random.RandomState(8).standard_normal((16, c["D"])) * np.sqrt(c["pv"])
    other[9] = c["q_start"][19]
    moved = go(other, chain_offset=10)
    for a in ("q_chain", "E_chain", "dE_chain", "step_scale", "adapt_state"):
        assert np.array_equal(getattr(moved, a)[9], getattr(one, a)[19]), a
        assert not np.array_equal(getattr(moved, a)[8], getattr(one, a)[18]), a


def engine(c, **kw):
    from hmc_amd.engine import GLMEngine, GLMNutsEngine
    common = dict(cov_p=c["cov_p"], rng="philox", seed=11, adapt_step=True, adapt_delta=DELTA, **kw)
    if c["kind"] == "NUTS":
        return GLMNutsEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["d_max"], c["dt"], **common)
    return GLMEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["Llo"], c["Lhi"], c["dt"], **common)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_save_and_restore_inside_warm_up(kind, family, tmp_path):
    """Checkpoint after iteration 3 of 7 adapting ones, restore into a fresh engine, continue: the
    chains, the energies, the counters and the state array equal the uninterrupted run's, bitwise."""
    c = invariance_case(kind, family)
    full = engine(c)
    full.init(c["q_start"])
    full.run(1, c["Niter"] + 1)
    first = engine(c)
    first.init(c["q_start"])
    first.run(1, 4)
    path = str(tmp_path / "ckpt.npz")
    first.save(path, 4)
    mid = first.adapt_state.clone()
    second = engine(c)
    assert second.restore(path) == 4
    assert torch.equal(second.adapt_state, mid) and torch.all(mid[:, 3] == 3)
    second.run(4, c["Niter"] + 1)
    torch.cuda.synchronize()
    for a in ("q", "q_chain", "E_chain", "dE_chain", "adapt_state", "step_scale"):
        assert torch.equal(getattr(second, a), getattr(full, a)), a
    keep = [i for i in range(9) if not (kind == "NUTS" and i == 3)]     # NUTS LEAPFROG_SQ: wave steps, per launch
    assert np.array_equal(second.read_counters()[keep], full.read_counters()[keep])
    assert not torch.equal(full.adapt_state[:, :3], mid[:, :3])
    from hmc_amd.engine import GLMEngine, GLMNutsEngine      # a checkpoint of an adaptive run needs one
    plain = (GLMNutsEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["d_max"], c["dt"],
                           cov_p=c["cov_p"], rng="philox", seed=11) if kind == "NUTS" else
             GLMEngine(G.glm_target(c), c["N"], c["Niter"], c["wu"], c["thin"], c["Llo"], c["Lhi"], c["dt"],
                       cov_p=c["cov_p"], rng="philox", seed=11))
    with pytest.raises(AssertionError):
        plain.restore(path)


# ------------------------------------------------------------------------------------------ g
ENSEMBLE_ADAPT, ENSEMBLE_AFTER = 32, 8


def test_ensemble_against_the_model():
    """Bernoulli (its energies cannot overflow), D = 2, n = 20, NUTS, d_max 8.  GPU Philox: 8,192
    chains, 32 adapting iterations and 8 more (40 and 10 take the model side 19 s on the CPU, these
    15 s); model with LiveDraws: 128 chains, the same settings; both sides keep the current sample
    where a tree reaches d_max (0.4 % of the model's trees).
    The means of log(step_scale) agree within 5 sd sqrt(1/128 + 1/8192), sd from the GPU sample, and so
    do the means of the post-warm-up acceptance statistic: two-sample bounds, both sides from one dt."""
    NG, NO = 8192, 128
    wu, Niter = ENSEMBLE_ADAPT + 1, ENSEMBLE_ADAPT + ENSEMBLE_AFTER
    c = TN.nuts_case("bernoulli", "D2")
    c = dict(c, kind="NUTS", Niter=Niter, wu=wu, thin=1, d_max=8)
    rs = np.random.RandomState(78)
    qg, qo = 0.5 * rs.standard_normal((NG, 2)), 0.5 * rs.standard_normal((NO, 2))
    h = sampler(dict(c, N=NG), rng="philox", seed=4, adapt_step=True, adapt_delta=DELTA)
    h.gen_sample_NUTS(qg, 0, False, on_dmax="break")
    np.random.seed(13)
    ref = A.nuts_adaptive(G.oracle_target(c), c["dt"], None, qo, Niter, wu, 1, 8, O.LiveDraws(2, np.eye(2)), wu,
                          DELTA)
    print("n_dmax: GPU %d of %d trees, model %d of %d" % (h.n_dmax, NG * Niter, ref["n_dmax"], NO * Niter))
    assert not ref["clamped"] and np.all(np.isfinite(h.step_scale))
    assert np.all(h.adapt_state[:, 3] == ENSEMBLE_ADAPT) and np.all(h.adapt_state[:, 7] == ENSEMBLE_AFTER)
    for name, x, y in (("log step_scale", np.log(h.step_scale), np.log(ref["step_scale"])),
                       ("post-warm-up alpha", h.adapt_state[:, 6] / h.adapt_state[:, 7],
                        ref["state"][:, 6] / ref["state"][:, 7])):
        sd = x.std(ddof=1)
        z = (x.mean() - y.mean()) / (sd * np.sqrt(1 / NO + 1 / NG))
        print("%s: GPU mean %.4f  model mean %.4f  sd %.4f  z %.2f" % (name, x.mean(), y.mean(), sd, z))
        assert abs(z) <= 5
    np.testing.assert_allclose(h.accept_stat, (h.adapt_state[:, 6] / h.adapt_state[:, 7]).mean(), rtol=1e-12)
