"""Four chains per wavefront (hmc_rows.hip), the parts its trimmed sampling loop moved:

  * the split Philox block (a per-block table of the pair-only products, keyed by the high word of
    the block's first chain id) and the wave that falls back to the whole block because one of its
    rows lies across a 2^32 boundary of the global chain id;
  * the L and L^2 tallies and the wave's longest trajectory, now taken from the 16-iteration draw
    block, under launches cut at iterations that are no multiple of 16;
  * the paired row reduction, which leaves the energy in lane 15 and the Metropolis test in lane 7 of
    a row, and the in-place parking of E and dE.

Helpers, references and tolerances are those of tests/test_gpu_row_groups.py: q to 1e-9, E to 1e-10
relative, dE to 1e-10 of the largest |E|, counts exact."""
import numpy as np
import pytest
import torch

from test_gpu_row_groups import (L_HIGH, L_LOW, _accepts, _assert_rows, _check_chain, _check_counts, _engine,
                                 _q_start, _reference, _run)

gpu = pytest.mark.gpu


def _state(eng):
    return (eng.q.clone(), eng.q_chain.clone(), eng.E_chain.clone(), eng.dE_chain.clone(), eng.read_counters())


def _check_dE(eng, ref):
    np.testing.assert_allclose(eng.dE_chain.cpu().numpy(), ref["dE_chain"], rtol=0,
                               atol=1e-10 * np.abs(ref["E_chain"]).max())


# ---- a 2^32 boundary of the global chain id inside a wave
STRADDLE = dict(D=100, niter=20, dt=0.1, seed=0xE0_0000, n=10, off=(1 << 32) - 5)


def _straddle_run(lo, hi):
    s = STRADDLE
    eng = _engine(s["D"], s["niter"], 1, 1, s["dt"], s["seed"], n=hi - lo, chain_offset=s["off"] + lo)
    _assert_rows(eng)
    _run(eng, _q_start(s["D"], s["n"])[lo:hi], [1, s["niter"] + 1])
    return eng


@gpu
def test_rows_wave_across_a_32_bit_chain_boundary():
    """Ten chains at global ids 2^32 - 5 .. 2^32 + 4: wave 0 lies below the boundary (the table's
    high word), wave 1 holds rows 2^32 - 1 | 2^32, 2^32 + 1, 2^32 + 2 and must draw with the whole
    block, wave 2 lies above.  Every chain against the oracle on host-regenerated draws."""
    s = STRADDLE
    ids = s["off"] + np.arange(s["n"])
    assert (ids[4] >> 32, ids[5] >> 32) == (0, 1) and ids[3] >> 32 == 0 and ids[8] >> 32 == 1
    ref = _reference(s["D"], s["niter"], 1, 1, s["dt"], s["seed"], s["n"], s["off"])
    eng = _straddle_run(0, s["n"])
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    _check_dE(eng, ref)


@gpu
def test_rows_boundary_shards_bitwise():
    """The same ten chains as two launches' shards of five: chain 2^32 - 1 is then the only row of a
    wave that takes the table, and chains 2^32 .. start a block whose table has the other high word.
    Everything bitwise equal to the single launch."""
    s = STRADDLE
    whole = _state(_straddle_run(0, s["n"]))
    a, b = _state(_straddle_run(0, 5)), _state(_straddle_run(5, s["n"]))
    for k in range(4):
        assert torch.equal(torch.cat([a[k], b[k]]), whole[k]), k
    assert np.array_equal(a[4] + b[4], whole[4])


# ---- launches cut inside a 16-iteration draw block
@gpu
@pytest.mark.parametrize("D", [97, 112])
def test_rows_ragged_launch_cuts(D):
    """npairs 49 and 56 (the table's extremes), 35 iterations as launches [1, 8), [8, 24), [24, 36):
    no cut is a multiple of 16, so every launch tallies part of a draw block and flushes its parked
    E and dE partially.  Against the oracle, and bitwise equal to the single launch [1, 36)."""
    niter, dt, seed = 35, 0.1, 0xE1_0000 + D
    ref = _reference(D, niter, 1, 1, dt, seed)
    out = []
    for cuts in ([1, 8, 24, 36], [1, 36]):
        eng = _engine(D, niter, 1, 1, dt, seed)
        _assert_rows(eng)
        _run(eng, _q_start(D), cuts)
        _check_counts(eng, ref)                      # accepts, sum L, sum L^2
        _check_chain(eng, ref)
        _check_dE(eng, ref)
        out.append(_state(eng))
    for k in range(4):
        assert torch.equal(out[0][k], out[1][k]), k
    assert np.array_equal(out[0][4], out[1][4])


# ---- the decision lanes
@gpu
def test_rows_decisions_per_chain():
    """dt = 1.2: rejections in every chain, and rows of wave 0 that accept beside rows that reject in
    one iteration (asserted on the reference).  The decision of every chain and iteration equals the
    reference's, a rejected iteration stores the row before it bit for bit, and the counts are exact."""
    D, n, niter, dt, seed = 100, 6, 40, 1.2, 0xE2_0000
    ref = _reference(D, niter, 1, 1, dt, seed, n)
    qs = _q_start(D, n)
    acc_ref = _accepts(ref, qs)
    rej_ref = ~acc_ref
    assert rej_ref.any(axis=1).all()                                       # every chain rejects at least once
    assert np.any(rej_ref[:4].any(axis=0) & acc_ref[:4].any(axis=0))      # mixed decisions in wave 0
    assert np.array_equal(acc_ref.sum(axis=1), ref["accept"])
    eng = _engine(D, niter, 1, 1, dt, seed, n=n)
    _assert_rows(eng)
    _run(eng, qs, [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    qc = eng.q_chain.cpu().numpy()
    prev = np.concatenate([qs[:, None, :], qc[:, :-1]], axis=1)
    same = np.all(qc == prev, axis=2)                                       # the row before, bit for bit
    assert np.array_equal(same, rej_ref)
    assert np.array_equal((~same).sum(axis=1), ref["accept"])              # accept counts per chain
    assert L_LOW == 5 and L_HIGH == 20
