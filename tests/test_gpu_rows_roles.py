"""The four-chain kernel's two state sets (hmc_rows.hip): an iteration integrates from the set that
holds the state into the other one, the next iteration swaps the roles, and a loop that ends after an
odd number of iterations copies the state back once.  What can go wrong is tied to the parity of an
iteration inside its loop: launch cuts and a warm-up boundary at odd counts, rejections in either
role, a thinned run whose sampling loop is odd, and the state a launch leaves behind.  Helpers,
draws (host-regenerated Philox) and tolerances are those of tests/test_gpu_row_groups.py: q to 1e-9,
E to 1e-10 relative, counts exact.  The last test pins the table-driven normals (whose log table
and series now carry the radius's factor -2) to a fixture recorded with the library before that
change."""
import os

import numpy as np
import pytest
import torch

from test_gpu_row_groups import (_assert_rows, _check_chain, _check_counts, _engine, _q_start, _reference,
                                 _rejections, _run)

pytestmark = pytest.mark.gpu

PAR_N, PAR_ITERS = 10, 35          # three waves, the last with two rows


def _outputs(eng):
    return (eng.q.clone(), eng.q_chain.clone(), eng.E_chain.clone(), eng.dE_chain.clone(), eng.E_prev.clone(),
            eng.read_counters())


def _assert_bitwise(a, b):
    for k in range(5):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a[5], b[5])


def _parity_run(D, wu, cuts, seed):
    ref = _reference(D, PAR_ITERS, wu, 1, 0.1, seed, PAR_N)
    eng = _engine(D, PAR_ITERS, wu, 1, 0.1, seed, n=PAR_N)
    _assert_rows(eng)
    _run(eng, _q_start(D, PAR_N), cuts)
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    np.testing.assert_allclose(eng.dE_chain.cpu().numpy(), ref["dE_chain"], rtol=0,
                               atol=1e-10 * np.abs(ref["E_chain"]).max())
    return _outputs(eng)


def test_role_parity_under_cuts():
    """D = 100, 35 iterations: one launch (17 trips and an unpaired iteration), and launches of 1, 3
    and 31 iterations (each odd: every launch ends with the copy back, and an iteration's role differs
    from the one it has in the single launch from the second launch on)."""
    seed = 0xA1_0000
    whole = _parity_run(100, 1, [1, 36], seed)
    cut = _parity_run(100, 1, [1, 2, 5, 36], seed)
    _assert_bitwise(cut, whole)


def test_warmup_ends_after_an_odd_count_inside_a_launch():
    """warm_up = 4: the warm-up loop of the single launch runs iterations 1..3 (odd: copy back at the
    boundary), the sampling loop 32; cut at 3, the second launch has one warm-up iteration."""
    seed = 0xA2_0000
    whole = _parity_run(100, 4, [1, 36], seed)
    cut = _parity_run(100, 4, [1, 3, 36], seed)
    _assert_bitwise(cut, whole)


@pytest.mark.parametrize("D", [97, 112])
def test_role_parity_other_D(D):
    seed = 0xA3_0000 + D
    whole = _parity_run(D, 1, [1, 36], seed)
    cut = _parity_run(D, 1, [1, 2, 5, 36], seed)
    _assert_bitwise(cut, whole)


REJ_SEED = 0xA4_0000


def test_rejections_in_both_roles():
    """dt = 1.2, 6 chains, 41 iterations in one launch: iteration i runs in role (i - 1) % 2.  The
    reference's wave 0 (chains 0..3) rejects at even and at odd iterations and at two consecutive
    ones; the decisions are the reference's, and a rejected iteration stores the row before it bit
    for bit (the set the iteration started from was never written)."""
    D, niter, dt = 100, 41, 1.2
    ref = _reference(D, niter, 1, 1, dt, REJ_SEED)
    rej = _rejections(ref)                               # [:, k]: iteration k + 2
    its = np.arange(2, niter + 1)
    w0 = rej[:4].any(axis=0)
    assert np.any(w0 & (its % 2 == 0)) and np.any(w0 & (its % 2 == 1))
    assert np.any(rej[:4, 1:] & rej[:4, :-1])            # a chain of wave 0 rejects twice in a row
    assert 0 < rej.sum() < rej.size
    eng = _engine(D, niter, 1, 1, dt, REJ_SEED)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    qc = eng.q_chain.cpu().numpy()
    got = np.all(qc[:, 1:] == qc[:, :-1], axis=2)
    assert np.array_equal(got, rej)                      # the same decisions, restored bit for bit
    assert np.array_equal(eng.q.cpu().numpy(), qc[:, -1])


def test_thin2_odd_sampling_loop():
    """warm_up = 6, 24 iterations, thin = 2, one launch: five warm-up iterations and nineteen sampling
    ones (both loops end unpaired).  Rows and the final state against the oracle; the last iteration
    stores a row, so the state the launch leaves is that row bit for bit."""
    D, niter, wu, thin, dt, seed = 100, 24, 6, 2, 0.1, 0xA5_0000
    assert (wu - 1) % 2 == 1 and (niter - wu + 1) % 2 == 1 and (niter - wu) % thin == 0
    ref = _reference(D, niter, wu, thin, dt, seed)
    eng = _engine(D, niter, wu, thin, dt, seed)
    _assert_rows(eng)
    _run(eng, _q_start(D), [1, niter + 1])
    _check_counts(eng, ref)
    _check_chain(eng, ref)
    assert ref["q_chain"].shape[1] == 10
    assert torch.equal(eng.q, eng.q_chain[:, -1])


def test_table_normals_equal_parent_fixture():
    """hmc_rng_normals against tests/golden/bm_parent_normals.npz, recorded on an MI355X with the
    library before the -2 moved into the log table: 64 chains from global id 2^32 - 32 (both sides of
    the 2^32 boundary), 56 pairs, iterations 0 and 12345.  Equal, not close."""
    from hmc_amd import _lib as H
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "bm_parent_normals.npz"))
    seed, chain0, npairs = int(fx["seed"]), int(fx["chain0"]), int(fx["npairs"])
    assert (chain0, npairs, list(fx["iterations"])) == (2 ** 32 - 32, 56, [0, 12345])
    for it in fx["iterations"]:
        want = fx["z_it%d" % it]
        assert want.shape == (64, 2 * npairs)
        out = torch.empty(want.shape, dtype=torch.float64, device="cuda")
        H.check(H.lib().hmc_rng_normals(seed, chain0, 64, int(it), npairs, out.data_ptr(), None), "hmc_rng_normals")
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), int(it)
