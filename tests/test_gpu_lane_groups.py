"""Every layout of the lane-group Random kernel (csrc/hmc_random.hip::k_random_iters<K, ...>, all
diagonal targets with D <= 64) against the oracle.

choose_layout gives each (D, L_low, L_high) a triple (K coordinate pairs per lane, lpc lanes per
chain, cpw chains per wave); over D = 1..64 and all trajectory-length ranges it takes 36 of them
(tests/test_layout_query.py holds the table and asserts, without a GPU, that the case lists below
reach every one).  What differs between layouts: the shuffle tree of group_sum (guarded by
s + off < lpc), the idle tail lanes of a wave (lpc = 7: 63 lanes used), the pv[j] slot mask (at
D = 25 the last lane's second slot is past npairs, at D = 27 it is not), the half pair of an odd D,
and in Philox mode the (L, log u) cache: lane s of a group draws iteration it + s once per lpc
iterations, read back by shuffle and restarted at every launch.

References: oracle/hmc_oracle.py (gen_sample_random on ReplayDraws) and, for Philox mode, the draws
regenerated on the host (tests/philox_host.py: group_momenta, host_L_lnu).  Tolerances are the
project's contracts:
  * replay, EXACT: q_chain bit-identical, E_chain rtol 1e-12, dE_chain rtol 1e-8 / atol 1e-10;
  * replay FAST and Philox: q within 1e-9 (rtol and atol), E rtol 1e-10;
  * always exact: both accept counters and rates, n_leapfrog, N_total_steps.
Every case runs cpw + 2 chains: one full wave and a ragged second one.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import hmc_oracle as O
from philox_host import group_momenta, host_L_lnu

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------- case lists
# (D, L_low, L_high).  tests/test_layout_query.py imports these lists.
# a. unit target: every D with L in [3, 9); constant L = 7 reaches K = 4, 5 (3..5 lanes), 8;
#    L in [5, 20) at D = 19, 20 reaches (1, 10, 6)
REPLAY_CASES = ([(D, 3, 9) for D in range(1, 65)]
                + [(D, 7, 8) for D in (21, 22, 24, 29, 30, 37, 40, 43, 48, 49, 50, 51, 56)]
                + [(D, 5, 20) for D in (19, 20)])
# b. general diagonal target (GEN = true), one odd D per K with more than one lane per chain:
#    (D, L_low, L_high, thin, warm_up)
GEN_CASES = [(13, 3, 9, 1, 3), (25, 3, 9, 2, 0), (27, 3, 9, 1, 3), (63, 3, 9, 2, 0),
             (21, 7, 8, 1, 3), (29, 7, 8, 2, 0), (43, 7, 8, 1, 3)]
# c. Philox mode, one case per layout, odd D wherever the layout has one: (K, lpc, cpw) -> (D, L_low, L_high)
PHILOX_CASES = {
    (1, 1, 64): (1, 3, 9), (1, 2, 32): (3, 3, 9), (1, 3, 21): (5, 3, 9), (1, 4, 16): (7, 3, 9),
    (1, 7, 9): (13, 3, 9), (1, 8, 8): (15, 3, 9), (1, 9, 7): (17, 3, 9), (1, 10, 6): (19, 5, 20),
    (1, 11, 5): (21, 3, 9), (1, 12, 5): (23, 3, 9), (1, 15, 4): (29, 3, 9), (1, 16, 4): (31, 3, 9),
    (1, 19, 3): (37, 3, 9), (1, 20, 3): (39, 3, 9), (1, 21, 3): (41, 3, 9), (1, 25, 2): (49, 3, 9),
    (1, 26, 2): (51, 3, 9), (1, 27, 2): (53, 3, 9), (1, 28, 2): (55, 3, 9), (1, 29, 2): (57, 3, 9),
    (1, 30, 2): (59, 3, 9), (1, 31, 2): (61, 3, 9), (1, 32, 2): (63, 3, 9),
    (2, 3, 21): (11, 3, 9), (2, 7, 9): (27, 3, 9), (2, 9, 7): (35, 3, 9), (2, 11, 5): (43, 3, 9),
    (2, 12, 5): (47, 3, 9),
    (4, 3, 21): (21, 7, 8), (4, 7, 9): (53, 7, 8),
    (5, 1, 64): (9, 3, 9), (5, 2, 32): (19, 3, 9), (5, 3, 21): (29, 7, 8), (5, 4, 16): (39, 7, 8),
    (5, 5, 12): (49, 7, 8),
    (8, 3, 21): (45, 7, 8),
}
PHILOX_GEN_CASES = [(13, 3, 9), (25, 3, 9)]          # p_scale != 1
SHARD_CASE = (13, 3, 9)                              # d.
CAPTURE_CASE = (13, 3, 9)                            # e.
WINDOW_CASE = (26, 3, 9)                             # e. (K = 2)


def all_cases():
    """(D, L_low, L_high) of every GPU case of this file."""
    return (REPLAY_CASES + [c[:3] for c in GEN_CASES] + sorted(PHILOX_CASES.values()) + PHILOX_GEN_CASES
            + [SHARD_CASE, CAPTURE_CASE, WINDOW_CASE])


def layout(D, lo, hi):
    """(K, lpc, cpw) hmc_random_iters takes (host query of the real choose_layout)."""
    from hmc_amd import _lib as H
    K, lpc, cpw, wave = H.random_layout(D, lo, hi)
    assert wave == 0, "D = %d does not run the lane-group kernel" % D
    return K, lpc, cpw


# ---------------------------------------------------------------------------------- references
def _problem(D, gen, rs):
    """Unit target, dt = 0.1; or q0 != 0, diagonal cov0 and cov_p, vector dt."""
    if not gen:
        return dict(q0=np.zeros(D), cov0=np.eye(D), cov_p=None, dt=0.1, sd=1.0)
    q0 = rs.standard_normal(D) * 0.5
    cov0 = np.diag(rs.uniform(0.5, 2.0, D))
    cov_p = np.diag(rs.uniform(0.8, 1.3, D))
    return dict(q0=q0, cov0=cov0, cov_p=cov_p, dt=rs.uniform(0.05, 0.15, D), sd=np.sqrt(np.diag(cov_p)))


def _oracle(c, n_save=0):
    core = O.HMCCore(O.MVNTarget(c["q0"], c["cov0"]), c["dt"], c["cov_p"])
    return O.gen_sample_random(core, c["q_start"], c["N"], c["Niter"], c["wu"], c["thin"], c["lo"], c["hi"],
                               O.ReplayDraws(c["p0"], c["P"], c["L"], c["lnu"]), n_save_chain0=n_save)


@functools.lru_cache(maxsize=None)
def replay_case(D, lo, hi, gen=False, thin=1, wu=3, n_save=0):
    """Inputs, recorded draw streams and the oracle's run of them (computed once, never modified)."""
    Niter = 8
    N = layout(D, lo, hi)[2] + 2
    rs = np.random.RandomState(100000 * int(gen) + 1000 * D + 10 * lo + hi)
    c = _problem(D, gen, rs)
    c.update(D=D, N=N, Niter=Niter, wu=wu, thin=thin, lo=lo, hi=hi, offset=0,
             q_start=c["q0"] + rs.standard_normal((N, D)),
             p0=rs.standard_normal((N, D)) * c["sd"], P=rs.standard_normal((N, Niter, D)) * c["sd"],
             L=rs.randint(lo, hi, size=(N, Niter)).astype(np.int32), lnu=np.log(rs.random_sample((N, Niter))))
    return c, _oracle(c, n_save)


def philox_inputs(D, lo, hi, gen, N, Niter, offset, seed, wu=2):
    """A Philox-mode run's inputs with its draws regenerated on the host for global chains
    offset .. offset + N - 1."""
    rs = np.random.RandomState(200000 * int(gen) + 1000 * D + 10 * lo + hi)
    c = _problem(D, gen, rs)
    gcs = np.arange(offset, offset + N, dtype=np.uint64)
    p0, P = group_momenta(seed, gcs, D, Niter)
    L, lnu = host_L_lnu(seed, gcs, Niter, lo, hi)
    c.update(D=D, N=N, Niter=Niter, wu=wu, thin=1, lo=lo, hi=hi, offset=offset, seed=seed,
             q_start=c["q0"] + rs.standard_normal((N, D)), p0=p0 * c["sd"], P=P * c["sd"], L=L, lnu=lnu)
    return c


@functools.lru_cache(maxsize=None)
def philox_case(D, lo, hi, gen=False):
    """Niter = 2 lpc + 3: the (L, log u) cache refills twice and ends mid-block; the first chain's
    global id is not a multiple of cpw."""
    K, lpc, cpw = layout(D, lo, hi)
    c = philox_inputs(D, lo, hi, gen, N=cpw + 2, Niter=2 * lpc + 3, offset=3 * cpw + 1, seed=0x5EED0000 + 977 * D + hi)
    return c, _oracle(c)


def run(c, fp_mode, rng="replay", n_save=0, rows=slice(None), **kw):
    """HMC_sampler on the case's inputs (chains `rows` of it)."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    q_start = c["q_start"][rows]
    h = HMC_sampler(c["D"], None, None, Nchain=len(q_start), Niter=c["Niter"], thin_rate=c["thin"],
                    warm_up_num=c["wu"], cov_p=c["cov_p"], sampler_type="Random", L_low=c["lo"], L_high=c["hi"],
                    dt=c["dt"], target=MVNTarget(c["q0"], c["cov0"]), rng=rng, fp_mode=fp_mode, **kw)
    if rng == "replay":
        h.set_random_replay(c["p0"][rows], c["P"][rows], c["L"][rows], c["lnu"][rows])
    h.gen_sample(q_start, N_save_chain0=n_save, verbose=False)
    return h


def run_philox(c, rows=slice(None), **kw):
    kw.setdefault("chain_offset", c["offset"])
    return run(c, "fast", rng="philox", seed=c["seed"], rows=rows, **kw)


def check(h, ref, exact):
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]
    assert h.n_leapfrog == ref["n_leapfrog"] and h.N_total_steps == ref["N_total_steps"]
    if exact:
        assert np.array_equal(h.q_chain, ref["q_chain"]), "q_chain not bit-identical to the oracle"
        np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-12)
        np.testing.assert_allclose(h.dE_chain[:, :, 0], ref["dE_chain"], rtol=1e-8, atol=1e-10)
    else:
        np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)


# ------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("fp_mode", ["exact", "fast"])
@pytest.mark.parametrize("D,lo,hi", REPLAY_CASES)
def test_replay_parity_every_D(D, lo, hi, fp_mode):
    """Unit target, dt = 0.1, 8 iterations, warm-up 3, cpw + 2 chains, replayed draws."""
    c, ref = replay_case(D, lo, hi)
    check(run(c, fp_mode), ref, exact=fp_mode == "exact")


# ------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("fp_mode", ["exact", "fast"])
@pytest.mark.parametrize("D,lo,hi,thin,wu", GEN_CASES)
def test_general_diagonal_replay(D, lo, hi, thin, wu, fp_mode):
    """GEN = true (q0 != 0, diagonal cov0 and cov_p, vector dt) on the multi-lane layouts of every K,
    with thinning and without warm-up in some."""
    assert layout(D, lo, hi)[1] > 1
    c, ref = replay_case(D, lo, hi, gen=True, thin=thin, wu=wu)
    check(run(c, fp_mode), ref, exact=fp_mode == "exact")


# ------------------------------------------------------------------------------------------ c
def _philox_fused_and_split(c, ref, lpc):
    one = run_philox(c)
    split = run_philox(c, iters_per_launch=lpc + 1)       # every launch restarts the (L, log u) cache
    for a in ("q_chain", "E_chain", "dE_chain", "_acc", "_acc_wu", "n_leapfrog", "N_total_steps"):
        assert np.array_equal(getattr(one, a), getattr(split, a)), a
    assert one.n_leapfrog == int(c["L"].sum())
    check(one, ref, exact=False)
    check(split, ref, exact=False)


@pytest.mark.parametrize("lay", sorted(PHILOX_CASES), ids=lambda l: "K%d-lpc%d" % l[:2])
def test_philox_parity_every_layout(lay):
    """In-kernel Philox draws of every layout against the oracle on the host-regenerated draws, as
    one fused launch and in launches of lpc + 1 iterations (bit-identical to each other)."""
    D, lo, hi = PHILOX_CASES[lay]
    assert layout(D, lo, hi) == lay
    c, ref = philox_case(D, lo, hi)
    _philox_fused_and_split(c, ref, lay[1])


@pytest.mark.parametrize("D,lo,hi", PHILOX_GEN_CASES)
def test_philox_parity_general_diagonal(D, lo, hi):
    """GEN = true with p_scale != 1: the host draw times sqrt(diag cov_p)."""
    c, ref = philox_case(D, lo, hi, gen=True)
    assert np.all(c["sd"] != 1.0)
    _philox_fused_and_split(c, ref, layout(D, lo, hi)[1])


# ------------------------------------------------------------------------------------------ d
def test_shard_invariance_in_lane_groups():
    """2 cpw + 3 chains as one call and as two shards split inside a wave's second lane group
    (chain 10, cpw = 9): results depend on the global chain id only."""
    D, lo, hi = SHARD_CASE
    cpw = layout(D, lo, hi)[2]
    assert cpw == 9
    N, cut = 2 * cpw + 3, 10
    c = philox_inputs(D, lo, hi, False, N=N, Niter=17, offset=0, seed=0xD13)
    one = run_philox(c)
    a = run_philox(c, rows=slice(0, cut), chain_offset=0)
    b = run_philox(c, rows=slice(cut, N), chain_offset=cut)
    for k in ("q_chain", "E_chain", "dE_chain"):
        assert np.array_equal(getattr(one, k), np.concatenate([getattr(a, k), getattr(b, k)])), k
    for k in ("_acc", "_acc_wu", "n_leapfrog"):
        assert getattr(one, k) == getattr(a, k) + getattr(b, k), k
    check(one, _oracle(c), exact=False)


# ------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("fp_mode", ["exact", "fast"])
def test_chain0_capture_on_a_multi_lane_layout(fp_mode):
    """phi_q (q[:2] at the start and after every leapfrog step of chain 0's first 4 iterations) and
    decision_chain from the 7-lane layout equal the oracle's."""
    D, lo, hi = CAPTURE_CASE
    assert layout(D, lo, hi)[:2] == (1, 7)
    n_save = 4
    c, ref = replay_case(D, lo, hi, n_save=n_save)
    h = run(c, fp_mode, n_save=n_save)
    check(h, ref, exact=fp_mode == "exact")
    assert np.array_equal(h.decision_chain[:, 0], ref["decision_chain"])
    assert len(h.phi_q) == len(ref["phi_q"]) == n_save
    for i, (got, want) in enumerate(zip(h.phi_q, ref["phi_q"])):
        assert got.shape == want.shape == (c["L"][0, i] + 1, 2)
        if fp_mode == "exact":
            assert np.array_equal(got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)


def test_circular_window_on_a_k2_layout():
    """Every row into a circular window of 4 rows (row r at slot r % 4) over 3 launches on the
    (2, 7, 9) layout, Philox: the window then holds the oracle's last 4 rows."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    D, lo, hi = WINDOW_CASE
    K, lpc, cpw = layout(D, lo, hi)
    assert (K, lpc) == (2, 7)
    S, launches, R = 4, 3, 4
    Niter = S * launches
    c = philox_inputs(D, lo, hi, False, N=cpw + 2, Niter=Niter, offset=0, seed=0x26, wu=S + 1)
    eng = RandomEngine(MVNTarget(c["q0"], c["cov0"]), c["N"], Niter, c["wu"], 1, lo, hi, c["dt"], rng="philox",
                       seed=c["seed"], fp_mode="fast", store_chain=False)
    win = torch.zeros((c["N"], R, D), dtype=torch.float64, device=eng.device)
    eng.set_chain_window(win, 0)
    eng.init(c["q_start"])
    for k in range(launches):
        eng.run(1 + k * S, 1 + (k + 1) * S)
    torch.cuda.synchronize()
    ref = _oracle(c)
    rows = ref["q_chain"].shape[1]
    assert rows % R == 0 and rows > R
    np.testing.assert_allclose(win.cpu().numpy(), ref["q_chain"][:, rows - R:], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)
    cnt = eng.read_counters()
    assert int(cnt[H.CNT_ACCEPT]) == ref["accept_count"] and int(cnt[H.CNT_ACCEPT_WU]) == ref["accept_count_warm_up"]
    assert int(cnt[H.CNT_LEAPFROG]) == ref["n_leapfrog"] == int(c["L"].sum())


# ------------------------------------------------------------------------------------------ f
@functools.lru_cache(maxsize=None)
def oob_case():
    """warm_up = 16 > L_chain * thin = 5 on the (1, 2, 32) layout: 37 chains are a full wave and five
    chains of a second one.  A rejection at i < i_oob = warm_up - L_chain * thin = 11 writes q_chain
    row (i - warm_up) // thin < -L_chain in the reference (samplers.py:471), an IndexError.  dt = 1.3
    makes the unit target reject often.  Returns the inputs and the (N, Niter) rejections, read from the
    oracle's replay of the same draws with warm_up = 1, which stores every iteration (a rejected
    iteration stores the point before it again, bit for bit; the decisions do not depend on warm_up)."""
    D, lo, hi, N, Niter = 3, 3, 9, 37, 20
    assert layout(D, lo, hi) == (1, 2, 32)
    rs = np.random.RandomState(3037)
    c = dict(_problem(D, False, rs), dt=1.3)
    c.update(D=D, N=N, Niter=Niter, wu=16, thin=1, lo=lo, hi=hi, offset=0, q_start=rs.standard_normal((N, D)),
             p0=rs.standard_normal((N, D)), P=rs.standard_normal((N, Niter, D)),
             L=rs.randint(lo, hi, size=(N, Niter)).astype(np.int32), lnu=np.log(rs.random_sample((N, Niter))))
    qc = _oracle(dict(c, wu=1))["q_chain"]
    return c, np.all(qc == np.concatenate([c["q_start"][:, None], qc[:, :-1]], axis=1), axis=2)


@pytest.mark.parametrize("fp_mode", ["exact", "fast"])
def test_out_of_range_rejections_and_L_tallies(fp_mode):
    """The tallies of k_random_iters over two launches, [1, 9) and [9, 21): the rejections before
    i_oob, sum L and sum L^2 equal the reference's, and HMC_sampler raises the reference's error."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    c, rej = oob_case()
    i_oob = c["wu"] - O.chain_len(c["Niter"], c["wu"], 1)
    assert i_oob == 11
    n_oob = int(rej[:, :i_oob - 1].sum())
    assert 0 < n_oob < rej[:, :i_oob - 1].size          # the reference rejects there, but not always
    with pytest.raises(IndexError):
        _oracle(c)
    eng = RandomEngine(MVNTarget(c["q0"], c["cov0"]), c["N"], c["Niter"], c["wu"], 1, c["lo"], c["hi"], c["dt"],
                       rng="replay", fp_mode=fp_mode)
    eng.set_replay(c["p0"], c["P"], c["L"], c["lnu"])
    eng.init(c["q_start"])
    eng.run(1, 9)
    eng.run(9, c["Niter"] + 1)
    torch.cuda.synchronize()
    cnt = eng.read_counters()
    L = c["L"].astype(np.int64)
    assert int(cnt[H.CNT_OOB_REJECT]) == n_oob
    assert int(cnt[H.CNT_LEAPFROG]) == int(L.sum()) and int(cnt[H.CNT_LEAPFROG_SQ]) == int((L * L).sum())
    if fp_mode == "fast":
        with pytest.raises(IndexError):
            run(c, fp_mode)
