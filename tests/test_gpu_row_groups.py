"""Four chains per wavefront (hmc_rows.hip, 97 <= D <= 112): `k_rows_iters<7>` pinned to the oracle
on host-regenerated Philox draws, to the wave-per-chain kernel inside one library, and to itself
under sharding.

The first cases run N = 6 chains with L in 5..20: wave 0 is full (chains 0..3, one per 16-lane row)
and wave 1 is half empty (chains 4, 5).  The later ones cover what those leave out: every D over a
whole period of the momentum ring, every wave of a block and a second and third block, ragged last
waves of one and three rows, a 64-bit chain offset, trajectories of one step and of thousands, the
L^2 and out-of-range tallies, and a sample window that starts at a later row.  The draws are
regenerated on the host (tests/philox_host.py, as tests/test_gpu_philox_parity.py does) and
replayed through oracle/hmc_oracle.py.  Every case that is meant for the four-chain kernel asserts
from the host queries that its launches take it (`_assert_rows`).
Tolerances: q to 1e-9 (FAST integrator against the reference's arithmetic), E to 1e-10 relative
(FAST mode's contract), accept and leapfrog counts exact.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import hmc_oracle as O
from philox_host import host_L_lnu, wave_momenta

N, L_LOW, L_HIGH = 6, 5, 20
gpu = pytest.mark.gpu


def _q_start(D, n=N):
    return np.random.RandomState(1000 + D).standard_normal((n, D)) * np.sqrt(2.0)


def _core(D, dt, hi):
    """The oracle's primitives on the unit MVN.  Trajectories of thousands of steps take the form
    without the D x D products by the identity (tests/test_gpu_philox_parity.py::UnitCore: the same
    arithmetic, np.dot(I, g) == g exactly), which keeps them to a second or two."""
    if hi <= 64:
        return O.HMCCore(O.MVNTarget(np.zeros(D), np.eye(D)), dt)
    from test_gpu_philox_parity import UnitCore, UnitMVN
    return UnitCore(UnitMVN(D), dt)


@functools.lru_cache(maxsize=None)
def _reference(D, niter, wu, thin, dt, seed, n=N, chain0=0, lo=L_LOW, hi=L_HIGH):
    """The oracle's run of global chains chain0 .. chain0 + n - 1 on the host-regenerated draws
    (computed once per case, never written to).  Chain by chain, so that `_first` can take the run
    of the first chains out of it: `accept` and `accept_wu` hold the counts per chain, "L" the
    trajectory lengths (n, niter)."""
    p0, P = wave_momenta(seed, n, D, niter, chain0=chain0)
    L, lnu = host_L_lnu(seed, np.arange(chain0, chain0 + n, dtype=np.uint64), niter, lo, hi)
    core, qs = _core(D, dt, hi), _q_start(D, n)
    per = [O.gen_sample_random(core, qs[m:m + 1], 1, niter, wu, thin, lo, hi,
                               O.ReplayDraws(p0[m:m + 1], P[m:m + 1], L[m:m + 1], lnu[m:m + 1])) for m in range(n)]
    ref = {k: np.concatenate([r[k] for r in per]) for k in ("q_chain", "E_chain", "dE_chain")}
    ref["accept"] = np.array([r["accept_count"] for r in per])
    ref["accept_wu"] = np.array([r["accept_count_warm_up"] for r in per])
    ref["N_total_steps"] = sum(r["N_total_steps"] for r in per)
    ref["L"], ref["sched"] = L, (niter, wu)
    return _totals(ref)


def _totals(ref):
    L = ref["L"].astype(np.int64)
    n, (niter, wu) = L.shape[0], ref["sched"]
    ref["accept_count"], ref["accept_count_warm_up"] = int(ref["accept"].sum()), int(ref["accept_wu"].sum())
    ref["accept_R"] = ref["accept_count"] / float(n * (niter - wu + 1))
    ref["n_leapfrog"] = ref["L_sum"] = int(L.sum())
    ref["L_sq"] = int((L * L).sum())
    return ref


def _first(ref, n):
    """The reference run of the first n chains of `ref` (chains do not interact, and a chain's
    draws are keyed by its global id)."""
    out = {k: ref[k][:n] for k in ("q_chain", "E_chain", "dE_chain", "accept", "accept_wu", "L")}
    out["sched"] = ref["sched"]
    return _totals(out)


def _engine(D, niter, wu, thin, dt, seed, n=N, chain_offset=0, lo=L_LOW, hi=L_HIGH, **kw):
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    return RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), n, niter, wu, thin, lo, hi, dt, rng="philox",
                        seed=seed, fp_mode="fast", chain_offset=chain_offset, **kw)


def _routing(eng):
    """(leapfrog form, layout) the host answers for this engine's launches."""
    from hmc_amd import _lib as H
    S = eng.schedule(1, eng.n_iter + 1)
    out = (ctypes.c_int32 * 4)()
    H.check(H.lib().hmc_random_layout_ex(ctypes.byref(eng.T), ctypes.byref(eng.K), ctypes.byref(S), ctypes.byref(out)))
    return H.lib().hmc_random_leapfrog_form(ctypes.byref(eng.T), ctypes.byref(eng.K), ctypes.byref(S)), tuple(out)


def _assert_rows(eng):
    """The launches of `eng` take the four-chain kernel: its layout and the three-term form for the
    engine's own descriptors, and no chain-0 capture (which the wave-per-chain kernel serves)."""
    from hmc_amd import _lib as H
    assert H.random_layout(eng.D, eng.L_low, eng.L_high) == (4, 16, 4, 0)
    assert _routing(eng) == (1, (4, 16, 4, 0))
    assert eng.n_save == 0 and eng.rng == "philox" and eng.fp_mode == "fast"


def _run(eng, q_start, cuts):
    eng.init(q_start)
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.run(a, b)
    torch.cuda.synchronize()


def _check_counts(eng, ref):
    from hmc_amd import _lib as H
    c = eng.read_counters()
    assert int(c[H.CNT_ACCEPT]) == ref["accept_count"]
    assert int(c[H.CNT_ACCEPT_WU]) == ref["accept_count_warm_up"]
    assert int(c[H.CNT_LEAPFROG]) == ref["n_leapfrog"] == ref["L_sum"]
    assert int(c[H.CNT_LEAPFROG_SQ]) == ref["L_sq"]      # feeds N_total_steps (Q13)
    return c


def _check_chain(eng, ref):
    """q rows and the final state to 1e-9, E rows to 1e-10 relative: the file's tolerances."""
    np.testing.assert_allclose(eng.q_chain.cpu().numpy(), ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.q.cpu().numpy(), ref["q_chain"][:, -1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)


def test_layout_and_form_queries(monkeypatch):
    """Host only: D = 97..112 answers 16 lanes per chain, 4 chains per wave, not the wave flag (7
    coordinates per lane are reported as 4 pairs); D = 96 and 113 keep the wave-per-chain answer;
    the leapfrog form at D = 100 is still the three-term one."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    assert H.random_layout(96, L_LOW, L_HIGH) == (1, 64, 1, 1)
    assert H.random_layout(97, L_LOW, L_HIGH) == (4, 16, 4, 0)
    assert H.random_layout(112, L_LOW, L_HIGH) == (4, 16, 4, 0)
    assert H.random_layout(113, L_LOW, L_HIGH) == (1, 64, 1, 1)
    T = H.Target(100, H.HMC_TARGET_DIAG, None, None, 0.0)
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    S = H.Schedule(4, 0, 10, 0, 1, 11, L_LOW, L_HIGH, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 10, 0, 0)
    assert H.lib().hmc_random_leapfrog_form(ctypes.byref(T), ctypes.byref(K), ctypes.byref(S)) == 1


@gpu
@pytest.mark.parametrize("split", [False, True], ids=["fused", "17+18"])
@pytest.mark.parametrize("D", [97, 100, 112])
def test_rows_vs_oracle(D, split):
    """35 iterations (two parked E batches of 16 plus three), one launch or launches of 17 + 18."""
    niter, wu, dt, seed = 35, 1, 0.1, 0xF0_0000 + D
    ref = _reference(D, niter, wu, 1, dt, seed)
    eng = _engine(D, niter, wu, 1, dt, seed)
    _run(eng, _q_start(D), [1, 18, 36] if split else [1, 36])
    _check_counts(eng, ref)
    np.testing.assert_allclose(eng.q_chain.cpu().numpy(), ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.q.cpu().numpy(), ref["q_chain"][:, -1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)


def _rejections(ref):
    """(N, niter - 1) booleans for iterations 2..niter of a thin = 1, warm_up = 1 reference run: a
    rejected iteration stores the row before it again (the restored start point, bit for bit)."""
    qc = ref["q_chain"]
    return np.all(qc[:, 1:] == qc[:, :-1], axis=2)


@functools.lru_cache(maxsize=None)
def _mixed_dt(D, niter, seed):
    """The first step size of a fixed ladder at which the reference run accepts between 0.2 and 0.8
    of the proposals and some iteration both accepts and rejects among chains 0..3 (one wave)."""
    for dt in (0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.2):
        ref = _reference(D, niter, 1, 1, dt, seed)
        rej = _rejections(ref)[:4]
        if 0.2 <= ref["accept_R"] <= 0.8 and np.any(rej.any(axis=0) & ~rej.all(axis=0)):
            return dt
    raise AssertionError("no step size of the ladder gives mixed decisions")


@gpu
def test_rows_mixed_decisions_in_a_wave():
    """Rows of one wave that accept next to rows that reject: the restore runs under the rejecting
    rows' EXEC mask only."""
    D, niter, seed = 100, 35, 0xF1_0000
    dt = _mixed_dt(D, niter, seed)
    ref = _reference(D, niter, 1, 1, dt, seed)
    eng = _engine(D, niter, 1, 1, dt, seed)
    _run(eng, _q_start(D), [1, 36])
    _check_counts(eng, ref)
    np.testing.assert_allclose(eng.q_chain.cpu().numpy(), ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)


@gpu
def test_rows_thinning_window_warmup():
    """thin = 2, a circular window of 3 rows, and the warm-up boundary (iteration 6) inside the first
    of two launches: the window holds the oracle's last three rows, E_chain every row."""
    D, niter, wu, thin, dt, seed, R = 100, 24, 6, 2, 0.1, 0xF2_0000, 3
    ref = _reference(D, niter, wu, thin, dt, seed)
    eng = _engine(D, niter, wu, thin, dt, seed, store_chain=False)
    win = torch.zeros((N, R, D), dtype=torch.float64, device=eng.device)
    eng.set_chain_window(win, 0)
    _run(eng, _q_start(D), [1, 10, 25])
    _check_counts(eng, ref)
    rows = ref["q_chain"].shape[1]
    assert rows == 10
    w = win.cpu().numpy()
    for r in range(rows - R, rows):
        np.testing.assert_allclose(w[:, r % R], ref["q_chain"][:, r], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.q.cpu().numpy(), ref["q_chain"][:, -1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)
    np.testing.assert_allclose(eng.dE_chain.cpu().numpy(), ref["dE_chain"], rtol=0,
                               atol=1e-10 * np.abs(ref["E_chain"]).max())


@gpu
@pytest.mark.parametrize("D", [97, 100, 112])
def test_rows_equal_wave_kernel(D):
    """One library, the same job twice: with chain-0 capture requested the wave-per-chain kernel
    runs, without it the four-chain kernel.  q and the q rows are bitwise equal (the same FMAs in
    the same order per coordinate); E differs only by the order of the energy sums."""
    from hmc_amd import _lib as H
    niter, wu, dt, seed = 35, 3, 0.1, 0xF3_0000 + D
    out = []
    for n_save in (3, 0):
        eng = _engine(D, niter, wu, 1, dt, seed, n_save=n_save)
        _run(eng, _q_start(D), [1, 20, 36])
        out.append((eng.q.clone(), eng.q_chain.clone(), eng.E_chain.clone(), eng.read_counters()))
    (qw, qcw, Ew, cw), (qr, qcr, Er, cr) = out
    assert torch.equal(qw, qr) and torch.equal(qcw, qcr)
    torch.testing.assert_close(Er, Ew, rtol=1e-12, atol=0)
    for k in (H.CNT_ACCEPT, H.CNT_ACCEPT_WU, H.CNT_LEAPFROG):
        assert cw[k] == cr[k]


@gpu
def test_rows_shard_invariance():
    """Chains 0..5 in one launch and as two shards of 3 (chain_offset): everything bitwise equal, E
    included (a row's sum order does not depend on which row of the wave it is)."""
    D, niter, wu, dt, seed = 100, 20, 2, 0.1, 0xF4_0000
    qs = _q_start(D)

    def run(lo, hi):
        eng = _engine(D, niter, wu, 1, dt, seed, n=hi - lo, chain_offset=lo)
        _run(eng, qs[lo:hi], [1, niter + 1])
        return eng.q.clone(), eng.q_chain.clone(), eng.E_chain.clone(), eng.dE_chain.clone(), eng.read_counters()

    whole, a, b = run(0, N), run(0, 3), run(3, N)
    for k in range(4):
        assert torch.equal(torch.cat([a[k], b[k]]), whole[k]), k
    assert np.array_equal(a[4] + b[4], whole[4])


# ---- every D over a whole period of the momentum ring
# A chain's read position in its ring moves 16 npairs bytes per iteration modulo 1280: it comes back
# after 80 iterations for odd npairs (D = 97/98, 101/102, 105/106, 109/110), after 40 at D = 107/108,
# 20 at D = 103/104, and sooner for the rest.  81 iterations visit every read offset of every D,
# those that run into the mirrored chunk included.
RING_ITERS = 81


def _ring_case(D):
    return D, RING_ITERS, 1, 1, 0.1, 0xF5_0000 + D


@gpu
@pytest.mark.parametrize("D", range(97, 113))
def test_rows_every_D_full_ring_period(D):
    """All sixteen D (npairs 49..56, the masked pair of odd D, the lanes that own slot 6), 81
    iterations in one launch."""
    ref = _reference(*_ring_case(D))
    eng = _engine(*_ring_case(D))
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, RING_ITERS + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


@gpu
@pytest.mark.parametrize("D", [97, 110])
def test_rows_ring_period_cut_launches(D):
    """The same runs in launches of 29 + 52 iterations: the ring restarts at a launch boundary, and
    29 is no multiple of 16, so a partial batch of parked E values is flushed there."""
    ref = _reference(*_ring_case(D))
    eng = _engine(*_ring_case(D))
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, 30, RING_ITERS + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


# ---- every wave of a block, later blocks, ragged last waves
GEOM_ITERS, GEOM_N = 20, 71


def _geom_case(D, n=GEOM_N):
    return D, GEOM_ITERS, 1, 1, 0.1, 0xF6_0000 + D, n


@gpu
@pytest.mark.parametrize("n", [71, 37, 33])
@pytest.mark.parametrize("D", [100, 97])
def test_rows_block_and_wave_geometry(D, n):
    """A block holds 8 waves x 4 chains, each chain with a ring of its own behind the tables.
    N = 71: two full blocks (every wave index 0..7) and a third with one full wave and one of three
    rows; N = 37 and N = 33: a second block whose last wave has one valid row (wave 1, wave 0).
    Every chain against the oracle (the reference of the first n chains of the 71)."""
    ref = _first(_reference(*_geom_case(D)), n)
    eng = _engine(*_geom_case(D, n))
    _assert_rows(eng)
    _run(eng, _q_start(D, n), [1, GEOM_ITERS + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


@gpu
def test_rows_chain_offset_past_32_bits():
    """Nine chains at global ids 2^33 + 5 ..: the chain id enters the Philox counter as two words,
    and the offset is no multiple of the four chains of a wave."""
    D, niter, dt, seed, n, off = 100, 20, 0.1, 0xF7_0000, 9, (1 << 33) + 5
    ref = _reference(D, niter, 1, 1, dt, seed, n, off)
    eng = _engine(D, niter, 1, 1, dt, seed, n=n, chain_offset=off)
    _assert_rows(eng)
    _run(eng, _q_start(D, n), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    # the draws do depend on the high word: another reference, not the same one under another name
    assert not np.array_equal(ref["L"], _reference(D, niter, 1, 1, dt, seed, n, 5)["L"])


# ---- trajectory lengths
@gpu
def test_rows_single_step_trajectories():
    """L_high = L_low + 1 = 2: every L is 1, no row has a paired step and the loop is skipped."""
    D, niter, dt, seed, lo, hi = 100, 35, 0.1, 0xF8_0000, 1, 2
    ref = _reference(D, niter, 1, 1, dt, seed, N, 0, lo, hi)
    assert ref["L"].min() == ref["L"].max() == 1
    eng = _engine(D, niter, 1, 1, dt, seed, lo=lo, hi=hi)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


@gpu
def test_rows_short_mixed_trajectories():
    """L in 1..4: rows without a paired step (L = 1) beside rows with one or two in the same wave,
    both parities of L."""
    D, niter, dt, seed, lo, hi = 100, 35, 0.1, 0xF9_0000, 1, 5
    ref = _reference(D, niter, 1, 1, dt, seed, N, 0, lo, hi)
    L = ref["L"]
    assert L.min() == 1 and L.max() == 4
    wave0 = L[:4]
    assert np.any((wave0 == 1).any(axis=0) & (wave0 >= 2).any(axis=0))
    assert np.any(L % 2 == 0) and np.any(L % 2 == 1)
    eng = _engine(D, niter, 1, 1, dt, seed, lo=lo, hi=hi)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


@gpu
def test_rows_longest_trajectories():
    """L in 4000..4095, the top of the range the host routes here: long paired-step loops with rows
    finishing at different counts, and L^2 close to the 24 bits the tally's multiply takes."""
    D, niter, dt, seed, lo, hi = 100, 3, 0.1, 0xFA_0000, 4000, 4096
    ref = _reference(D, niter, 1, 1, dt, seed, N, 0, lo, hi)
    assert ref["L"].min() >= 4000 and len(set(ref["L"][:4, 0])) > 1
    assert ref["L_sq"] > N * niter * 4000 ** 2 and int(ref["L"].max()) ** 2 < 1 << 24
    eng = _engine(D, niter, 1, 1, dt, seed, lo=lo, hi=hi)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)


# ---- tallies and the sample window
@gpu
def test_rows_total_steps_through_the_sampler():
    """HMC_sampler on the four-chain kernel: N_total_steps (Q13: L x D per step, from the L^2 tally)
    and the acceptance figures equal the oracle's."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    D, niter, wu, dt, seed = 100, 24, 3, 0.1, 0xFB_0000
    ref = _reference(D, niter, wu, 1, dt, seed)
    h = HMC_sampler(D, None, None, Nchain=N, Niter=niter, sampler_type="Random", L_low=L_LOW, L_high=L_HIGH, dt=dt,
                    warm_up_num=wu, target=MVNTarget(np.zeros(D), np.eye(D)), rng="philox", seed=seed,
                    fp_mode="fast")
    h.gen_sample(_q_start(D), verbose=False)
    _assert_rows(h.engine)
    assert h.N_total_steps == ref["N_total_steps"] == N * (1 + 2 * niter) + D * ref["L_sq"]
    assert h.n_leapfrog == ref["n_leapfrog"]
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.accept_R == ref["accept_R"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)


def _accepts(ref, q_start):
    """(N, niter) booleans of a thin = 1, warm_up = 1 reference run: iteration i moved the chain (a
    rejected iteration stores the row before it again, bit for bit)."""
    qc = ref["q_chain"]
    return np.any(qc != np.concatenate([q_start[:, None, :], qc[:, :-1]], axis=1), axis=2)


@functools.lru_cache(maxsize=None)
def _oob_dt(D, niter, seed, i_oob):
    """The first step size of the ladder at which the reference loop rejects, but not always, in the
    iterations before i_oob.  The decisions do not depend on warm_up or thin, so they are read from
    the replay of the same loop on the same draws with warm_up = 1, which stores every iteration."""
    for dt in (0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.2):
        rej = ~_accepts(_reference(D, niter, 1, 1, dt, seed), _q_start(D))[:, :i_oob - 1]
        if 0 < rej.sum() < rej.size:
            return dt, int(rej.sum())
    raise AssertionError("no step size of the ladder rejects before i_oob")


@gpu
def test_rows_out_of_range_rejections():
    """warm_up > L_chain * thin: a rejection at i < warm_up - L_chain * thin writes q_chain row
    (i - warm_up) // thin < -L_chain in the reference (samplers.py:471), an IndexError.  The kernel
    tallies those rejections, and HMC_sampler raises the reference's error from the tally."""
    from hmc_amd import _lib as H
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    D, niter, wu, seed = 100, 20, 16, 0xFC_0000
    L_chain = O.chain_len(niter, wu, 1)
    i_oob = wu - L_chain
    assert L_chain == 5 and i_oob == 11
    dt, n_oob = _oob_dt(D, niter, seed, i_oob)
    p0, P = wave_momenta(seed, N, D, niter)
    L, lnu = host_L_lnu(seed, np.arange(N, dtype=np.uint64), niter, L_LOW, L_HIGH)
    with pytest.raises(IndexError):
        O.gen_sample_random(_core(D, dt, L_HIGH), _q_start(D), N, niter, wu, 1, L_LOW, L_HIGH,
                            O.ReplayDraws(p0, P, L, lnu))
    eng = _engine(D, niter, wu, 1, dt, seed)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    c = eng.read_counters()
    assert int(c[H.CNT_OOB_REJECT]) == n_oob
    assert int(c[H.CNT_LEAPFROG]) == int(L.sum()) and int(c[H.CNT_LEAPFROG_SQ]) == int((L.astype(np.int64) ** 2).sum())
    h = HMC_sampler(D, None, None, Nchain=N, Niter=niter, sampler_type="Random", L_low=L_LOW, L_high=L_HIGH, dt=dt,
                    warm_up_num=wu, target=MVNTarget(np.zeros(D), np.eye(D)), rng="philox", seed=seed,
                    fp_mode="fast")
    assert H.random_layout(D, L_LOW, L_HIGH, dt=dt) == (4, 16, 4, 0)
    assert H.random_leapfrog_form(D, L_LOW, L_HIGH, dt) == 1
    with pytest.raises(IndexError):
        h.gen_sample(_q_start(D), verbose=False)


@gpu
def test_rows_window_from_a_later_row():
    """A circular window of 8 rows that starts at chain row 6 of 10 (qc_row0): rows 6..9 land in
    slots 6, 7, 0, 1 and equal the oracle's; slots 2..5, where rows 2..5 would have gone, keep the
    sentinel the window was filled with."""
    D, niter, wu, thin, dt, seed, R, row0 = 100, 24, 6, 2, 0.1, 0xFD_0000, 8, 6
    ref = _reference(D, niter, wu, thin, dt, seed)
    eng = _engine(D, niter, wu, thin, dt, seed, store_chain=False)
    _assert_rows(eng)
    sentinel = -12345.0
    win = torch.full((N, R, D), sentinel, dtype=torch.float64, device=eng.device)
    eng.set_chain_window(win, row0)
    _run(eng, _q_start(D), [1, 10, niter + 1])
    _check_counts(eng, ref)
    rows = ref["q_chain"].shape[1]
    assert rows == 10
    w = win.cpu().numpy()
    for r in range(row0, rows):
        np.testing.assert_allclose(w[:, r % R], ref["q_chain"][:, r], rtol=1e-9, atol=1e-9)
    untouched = sorted(set(range(R)) - {r % R for r in range(row0, rows)})
    assert untouched == [2, 3, 4, 5]
    assert np.all(w[:, untouched] == sentinel)
    np.testing.assert_allclose(eng.q.cpu().numpy(), ref["q_chain"][:, -1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)
