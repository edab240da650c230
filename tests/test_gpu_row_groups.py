"""Four chains per wavefront (hmc_rows.hip, 97 <= D <= 112): `k_rows_iters<7>` pinned to the oracle
on host-regenerated Philox draws, to the wave-per-chain kernel inside one library, and to itself
under sharding.

Every case runs N = 6 chains with L in 5..20: wave 0 is full (chains 0..3, one per 16-lane row) and
wave 1 is half empty (chains 4, 5).  The draws are regenerated on the host (tests/philox_host.py,
as tests/test_gpu_philox_parity.py does) and replayed through oracle/hmc_oracle.py.
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


def _q_start(D):
    return np.random.RandomState(1000 + D).standard_normal((N, D)) * np.sqrt(2.0)


@functools.lru_cache(maxsize=None)
def _reference(D, niter, wu, thin, dt, seed):
    """The oracle's run of chains 0..N-1 on the host-regenerated draws (computed once per case)."""
    p0, P = wave_momenta(seed, N, D, niter)
    L, lnu = host_L_lnu(seed, np.arange(N, dtype=np.uint64), niter, L_LOW, L_HIGH)
    ref = O.gen_sample_random(O.HMCCore(O.MVNTarget(np.zeros(D), np.eye(D)), dt), _q_start(D), N, niter, wu, thin,
                              L_LOW, L_HIGH, O.ReplayDraws(p0, P, L, lnu))
    ref["L_sum"] = int(L.sum())
    return ref


def _engine(D, niter, wu, thin, dt, seed, n=N, chain_offset=0, **kw):
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    return RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), n, niter, wu, thin, L_LOW, L_HIGH, dt, rng="philox",
                        seed=seed, fp_mode="fast", chain_offset=chain_offset, **kw)


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
