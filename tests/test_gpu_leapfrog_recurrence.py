"""The FAST wave kernels' three-term leapfrog u[n+1] = (2 - dt^2) u[n] - u[n-1] (hmc_wave.hip, TT).

Host model: tests/leapfrog_model.py restates the kernel's operation order in NumPy (`three_term`)
and integrates the reference's kick-drift-kick in long double on the same tape.  The tolerance of
"GPU against the restatement" is derived inside each test: 20 x the deviation the restatement
itself shows against the long-double run on the test's own inputs, required to come out below
1e-11 absolute (a ratio to the reference, never to the code under test).  The project's FAST
contract against the oracle (q 1e-9, E 1e-10 relative, identical decisions) is asserted as well.
The last tests run Philox schedules just inside and just outside the host's bound on the trajectory
length against the oracle, after checking on the CPU that the oracle and the
restatement are themselves within 1e-10 of the long-double run on those draws.
"""
import ctypes

import numpy as np
import pytest
import torch

import leapfrog_model as M
from oracle import hmc_oracle as O
from philox_host import host_L_lnu, table_normals, wave_momenta
from test_gpu_philox_parity import UnitCore, UnitMVN

pytestmark = pytest.mark.gpu

DT = 0.1
# every L of the tape: no interior step (1), both parities of L - 1, the longest trajectory
L_TAPE = np.array([[1, 2, 3, 4, 19, 1, 2, 3], [19, 4, 3, 2, 1, 19, 4, 3], [2, 19, 1, 3, 4, 4, 19, 1]], dtype=np.int32)


def _tape(D, N, Niter, seed, Ls=None, lnu=None):
    rs = np.random.RandomState(seed)
    q_start = rs.standard_normal((N, D)) * np.sqrt(2.0)
    p0, P = rs.standard_normal((N, D)), rs.standard_normal((N, Niter, D))
    if Ls is None:
        Ls = L_TAPE[:N, :Niter]
    if lnu is None:
        lnu = np.log(rs.random_sample((N, Niter)))
    return q_start, p0, P, np.ascontiguousarray(Ls, dtype=np.int32), lnu


def _form(eng):
    from hmc_amd import _lib as H
    return H.lib().hmc_random_leapfrog_form(ctypes.byref(eng.T), ctypes.byref(eng.K),
                                            ctypes.byref(eng.schedule(1, eng.n_iter + 1)))


def _gpu_replay(D, tape, dt=DT, L_low=1, L_high=20, n_save=0):
    """One launch of the replay kernel, warm-up 1, thin 1: row i - 1 holds iteration i."""
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    q_start, p0, P, Ls, lnu = tape
    N, Niter = Ls.shape
    eng = RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), N, Niter, 1, 1, L_low, L_high, dt, rng="replay",
                       fp_mode="fast", n_save=n_save)
    eng.set_replay(p0, P, Ls, lnu)
    eng.init(q_start)
    eng.run(1, Niter + 1)
    torch.cuda.synchronize()
    return eng


def _decisions(q_start, q_chain):
    """accept[m, i-1]: iteration i moved chain m (a rejected iteration stores the previous row)."""
    prev = np.concatenate([q_start[:, None, :], q_chain[:, :-1, :]], axis=1)
    return np.any(q_chain != prev, axis=2)


def _models(D, tape, dt=DT):
    """The restatement and the long-double run on the tape, and the derived tolerances."""
    q_start, p0, P, Ls, lnu = tape
    logc = D * np.log(2 * np.pi)
    rest = M.run_chains(q_start, P, Ls, lnu, dt, logc, "three_term")
    ld = M.run_chains(q_start, P, Ls, lnu, dt, logc, "long_double")
    assert np.array_equal(rest["accept"], ld["accept"])
    dev_q = float(np.max(np.abs(rest["q_chain"] - ld["q_chain"])))
    dev_E = float(np.max(np.abs(rest["E_chain"] - ld["E_chain"])))
    tol_q, tol_E = 20 * dev_q, 20 * dev_E
    print(f"D={D}: restatement vs long double: q {dev_q:.3e}, E {dev_E:.3e}; tolerances {tol_q:.3e}, {tol_E:.3e}")
    assert 0 < tol_q < 1e-11 and 0 < tol_E < 1e-11, (tol_q, tol_E)
    return rest, ld, tol_q, tol_E


def _oracle(D, tape, dt, L_low, L_high):
    q_start, p0, P, Ls, lnu = tape
    N, Niter = Ls.shape
    return O.gen_sample_random(UnitCore(UnitMVN(D), dt), q_start, N, Niter, 1, 1, L_low, L_high,
                               O.ReplayDraws(p0, P, Ls, lnu))


# K = 1 with an even D (66: the smallest even D of the wave kernel's range; 100: the headline), then
# the smallest D that selects K = 2, 4, 8, 16 (choose_layout: the first K with 64 K >= ceil(D/2))
@pytest.mark.parametrize("D", [66, 100, 129, 257, 513, 1025])
def test_replay_parity_smallest_shapes(D):
    from hmc_amd import _lib as H
    tape = _tape(D, 3, 8, 100 + D)
    rest, ld, tol_q, tol_E = _models(D, tape)
    eng = _gpu_replay(D, tape)
    assert _form(eng) == 1
    q_chain, E_chain = eng.q_chain.cpu().numpy(), eng.E_chain.cpu().numpy()
    c = eng.read_counters()
    ref = _oracle(D, tape, DT, 1, 20)
    acc = _decisions(tape[0], q_chain)
    dq, dE = np.max(np.abs(q_chain - rest["q_chain"])), np.max(np.abs(E_chain - rest["E_chain"]))
    print(f"D={D}: GPU vs restatement: q {dq:.3e}, E {dE:.3e}")
    assert np.array_equal(acc, rest["accept"])
    assert np.array_equal(acc, _decisions(tape[0], ref["q_chain"]))
    assert int(c[H.CNT_ACCEPT]) == ref["accept_count"] == int(rest["accept"].sum())
    assert int(c[H.CNT_ACCEPT_WU]) == ref["accept_count_warm_up"] == 0
    assert int(c[H.CNT_LEAPFROG]) == ref["n_leapfrog"] == int(tape[3].sum())
    assert dq <= tol_q and dE <= tol_E
    np.testing.assert_allclose(q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(E_chain, ref["E_chain"], rtol=1e-10)
    np.testing.assert_allclose(np.float64(rest["q_chain"]), ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(np.float64(rest["E_chain"]), ref["E_chain"], rtol=1e-10)


@pytest.mark.parametrize("D", [66, 65])
def test_philox_production_instance(D):
    """The assertions of test_wave_production_kernel_vs_oracle[fast] on the three-term instances:
    even D and the ODD ring instance, 64 chains x 6 iterations, L in {1..4}."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import MVNTarget
    N, Niter, wu, seed, lo, hi = 64, 6, 2, 0x5EED_0002 + D, 1, 5
    q_start = np.random.RandomState(7).standard_normal((N, D)) * np.sqrt(2.0)
    h = HMC_sampler(D, None, None, Nchain=N, Niter=Niter, sampler_type="Random", L_low=lo, L_high=hi, dt=DT,
                    warm_up_num=wu, target=MVNTarget(np.zeros(D), np.eye(D)), rng="philox", seed=seed,
                    fp_mode="fast")
    h.gen_sample(q_start, verbose=False)
    p0, P = wave_momenta(seed, N, D, Niter, normals=table_normals)
    L, lnu = host_L_lnu(seed, np.arange(N, dtype=np.uint64), Niter, lo, hi)
    assert L.min() == 1 and L.max() == 4
    ref = O.gen_sample_random(O.HMCCore(O.MVNTarget(np.zeros(D), np.eye(D)), DT), q_start, N, Niter, wu, 1, lo, hi,
                              O.ReplayDraws(p0, P, L, lnu))
    assert h._acc == ref["accept_count"] and h._acc_wu == ref["accept_count_warm_up"]
    assert h.accept_R == ref["accept_R"] and h.accept_R_warm_up == ref["accept_R_warm_up"]
    assert h.n_leapfrog == ref["n_leapfrog"] == int(L.sum())
    assert h.N_total_steps == ref["N_total_steps"]
    np.testing.assert_allclose(h.q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(h.E_chain[:, :, 0], ref["E_chain"], rtol=1e-10)


def test_capture_shows_every_step():
    """Chain 0's captured trajectory has L + 1 points per iteration, each the restatement's u[l]."""
    D, N, n_save = 100, 2, 5
    tape = _tape(D, N, 8, 7)
    rest, ld, tol_q, _ = _models(D, tape)
    dev = max(float(np.max(np.abs(a - b))) for a, b in zip(rest["traj0"], ld["traj0"]))
    tol = 20 * dev
    assert 0 < tol < 1e-11
    eng = _gpu_replay(D, tape, n_save=n_save)
    assert _form(eng) == 1
    traj, tlen = eng.traj.cpu().numpy(), eng.traj_len.cpu().numpy()
    dec = eng.decision.cpu().numpy()
    for i in range(n_save):
        L = int(tape[3][0, i])
        assert tlen[i] == L + 1
        want = rest["traj0"][i][:, :2]
        assert want.shape == (L + 1, 2)
        err = np.max(np.abs(traj[i, :L + 1] - want))
        print(f"iteration {i + 1}: L={L}, capture vs restatement {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol
        assert dec[i] == int(rest["accept"][0, i])


def test_rejected_moves_restore_q():
    """log u = 0 rejects every iteration whose energy rises: the row stored after a rejected
    iteration is the previous row bit for bit, for odd and for even L - 1."""
    D, N, Niter = 100, 3, 8
    tape = _tape(D, N, Niter, 11, lnu=np.zeros((N, Niter)))
    rest = M.run_chains(tape[0], tape[2], tape[3], tape[4], DT, D * np.log(2 * np.pi), "three_term")
    rej = ~rest["accept"]
    parity = (tape[3] - 1) & 1
    assert (rej & (parity == 0)).any() and (rej & (parity == 1)).any() and rest["accept"].any()
    eng = _gpu_replay(D, tape)
    assert _form(eng) == 1
    q_chain = eng.q_chain.cpu().numpy()
    prev = np.concatenate([tape[0][:, None, :], q_chain[:, :-1, :]], axis=1)
    assert np.array_equal(_decisions(tape[0], q_chain), rest["accept"])
    for m, i in zip(*np.nonzero(rej)):
        assert np.array_equal(q_chain[m, i], prev[m, i]), (m, i)


@pytest.mark.parametrize("dt", [5e-4, 2.0])
def test_fallback_two_fma_instance(dt):
    """Below the lower bound on dt (1e-3) and at the stability limit dt >= 2 the
    host launches the two-FMA instance, and the run keeps the FAST contract against the oracle."""
    D, N, Niter, lo, hi = 66, 2, 8, 1, 5
    rs = np.random.RandomState(5)
    tape = _tape(D, N, Niter, 13, Ls=rs.randint(lo, hi, size=(N, Niter)))
    eng = _gpu_replay(D, tape, dt=dt, L_low=lo, L_high=hi)
    assert _form(eng) == 0
    ref = _oracle(D, tape, dt, lo, hi)
    q_chain = eng.q_chain.cpu().numpy()
    assert np.array_equal(_decisions(tape[0], q_chain), _decisions(tape[0], ref["q_chain"]))
    np.testing.assert_allclose(q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)


# ---- the bound on the trajectory length: L_high m <= 2e5 dt (1 - dt^2 / 4), m = 2
# from dt^2 = 2 on.  (dt, L_low, the largest L_high inside the rule, iterations); L_high + 1 is the
# schedule just outside.  Short trajectories at the lower bound on dt, thousands of steps on the
# small-dt side, and thousands of steps near the stability limit, where the oracle in float64 is
# itself still within 1e-10 of the long-double run (it is not at dt = 1.9999).
EDGES = {"dt=1e-3": (1e-3, 190, 199, 8), "dt=1e-2": (1e-2, 1990, 1999, 3), "dt=1.99": (1.99, 1975, 1985, 3)}
EDGE_N = 6


def _edge_start(D, dt):
    """Start points on the scale of the leapfrog orbit, 1 / sqrt(1 - dt^2 / 4) (10 at dt = 1.99: from
    the target's own scale every proposal there is rejected and no long trajectory is ever kept)."""
    scale = max(np.sqrt(2.0), 1.0 / np.sqrt(1.0 - 0.25 * dt * dt))
    return np.random.RandomState(1000 + D).standard_normal((EDGE_N, D)) * scale


def _edge_run(D, dt, lo, hi, niter, seed):
    """One Philox run of 6 chains against the oracle on the host-regenerated draws, with the two
    figures that make the reference side safe printed and asserted first: the float64 oracle and
    the restatement of the three-term recurrence against the long-double run on these draws."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    p0, P = wave_momenta(seed, EDGE_N, D, niter)
    L, lnu = host_L_lnu(seed, np.arange(EDGE_N, dtype=np.uint64), niter, lo, hi)
    q_start = _edge_start(D, dt)
    ref = O.gen_sample_random(UnitCore(UnitMVN(D), dt), q_start, EDGE_N, niter, 1, 1, lo, hi,
                              O.ReplayDraws(p0, P, L, lnu))
    logc = D * np.log(2 * np.pi)
    ld = M.run_chains(q_start, P, L, lnu, dt, logc, "long_double")
    rest = M.run_chains(q_start, P, L, lnu, dt, logc, "three_term")
    dev_oracle = float(np.max(np.abs(ref["q_chain"] - ld["q_chain"])))
    dev_rest = float(np.max(np.abs(rest["q_chain"] - ld["q_chain"])))
    form = H.random_leapfrog_form(D, lo, hi, dt)
    print(f"D={D} dt={dt} L in [{lo}, {hi}): form {form}; against long double: oracle q {dev_oracle:.3e}, "
          f"restatement q {dev_rest:.3e}; {int(ld['accept'].sum())} of {ld['accept'].size} accepted")
    assert dev_oracle <= 1e-10
    assert np.array_equal(_decisions(q_start, ref["q_chain"]), ld["accept"])
    if form == 1:
        assert dev_rest <= 1e-10 and np.array_equal(rest["accept"], ld["accept"])
    eng = RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), EDGE_N, niter, 1, 1, lo, hi, dt, rng="philox", seed=seed,
                       fp_mode="fast")
    assert _form(eng) == form
    eng.init(q_start)
    eng.run(1, niter + 1)
    torch.cuda.synchronize()
    c = eng.read_counters()
    assert int(c[H.CNT_ACCEPT]) == ref["accept_count"] == int(ld["accept"].sum())
    assert int(c[H.CNT_LEAPFROG]) == ref["n_leapfrog"] == int(L.sum())
    assert int(c[H.CNT_LEAPFROG_SQ]) == int((L.astype(np.int64) ** 2).sum())
    q_chain = eng.q_chain.cpu().numpy()
    print(f"D={D}: GPU vs oracle: q {np.max(np.abs(q_chain - ref['q_chain'])):.3e}")
    np.testing.assert_allclose(q_chain, ref["q_chain"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eng.E_chain.cpu().numpy(), ref["E_chain"], rtol=1e-10)
    return form, ld["accept"]


@pytest.mark.parametrize("side", ["inside", "outside"])
@pytest.mark.parametrize("D", [100, 66])
@pytest.mark.parametrize("edge", list(EDGES))
def test_three_term_rule_edges(edge, D, side):
    """Just inside the rule the three-term instance runs (at D = 100 the four-chain kernel, at
    D = 66 the wave kernel's), just outside the two-FMA instance; both keep the FAST contract
    against the oracle."""
    from hmc_amd import _lib as H
    dt, lo, hi, niter = EDGES[edge]
    inside = side == "inside"
    hi += 0 if inside else 1
    assert H.random_leapfrog_form(D, lo, hi, dt) == (1 if inside else 0)
    assert H.random_layout(D, lo, hi, dt=dt) == ((4, 16, 4, 0) if inside and D == 100 else (1, 64, 1, 1))
    form, accept = _edge_run(D, dt, lo, hi, niter, 0xE0_0000 + D)
    assert form == (1 if inside else 0)
    assert accept.any()           # some long trajectory is kept: q rows that are not the start point


def test_three_term_long_rows_equal_wave_kernel():
    """Thousands of steps, inside the rule: the four-chain kernel and the wave-per-chain kernel
    (taken with chain-0 capture requested) run the same FMAs per coordinate, so q and the q rows are
    bitwise equal; E differs by the order of the energy sums."""
    from hmc_amd import _lib as H
    from hmc_amd.engine import RandomEngine
    from hmc_amd.target import MVNTarget
    D, seed = 100, 0xE3_0000
    dt, lo, hi, niter = EDGES["dt=1e-2"]
    assert H.random_layout(D, lo, hi, dt=dt) == (4, 16, 4, 0) and H.random_leapfrog_form(D, lo, hi, dt) == 1
    q_start = _edge_start(D, dt)
    out = []
    for n_save in (2, 0):
        eng = RandomEngine(MVNTarget(np.zeros(D), np.eye(D)), EDGE_N, niter, 1, 1, lo, hi, dt, rng="philox",
                           seed=seed, fp_mode="fast", n_save=n_save)
        assert _form(eng) == 1
        eng.init(q_start)
        eng.run(1, 3)
        eng.run(3, niter + 1)
        torch.cuda.synchronize()
        out.append((eng.q.clone(), eng.q_chain.clone(), eng.E_chain.clone(), eng.read_counters()))
    (qw, qcw, Ew, cw), (qr, qcr, Er, cr) = out
    assert torch.equal(qw, qr) and torch.equal(qcw, qcr)
    assert not torch.equal(qcr[:, 0], torch.as_tensor(q_start, device=qcr.device))
    torch.testing.assert_close(Er, Ew, rtol=1e-12, atol=0)
    for k in (H.CNT_ACCEPT, H.CNT_ACCEPT_WU, H.CNT_LEAPFROG, H.CNT_LEAPFROG_SQ):
        assert cw[k] == cr[k]
