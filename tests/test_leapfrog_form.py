"""Host-side choice of the leapfrog form (no GPU): hmc_random_leapfrog_form answers what
hmc_random_iters would launch (hmc_route.cpp::leapfrog_three_term)."""
import ctypes


def test_form_query_follows_the_bounds(monkeypatch):
    """hmc_random_leapfrog_form (host only, L in 5..20): three-term inside [1e-3, 2), two-FMA outside,
    in EXACT mode, for a general diagonal target and for the lane-group kernels (D <= 64)."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    L = H.lib()

    def form(D, dt, fp=H.HMC_MODE_FAST, prec=None):
        T = H.Target(D, H.HMC_TARGET_DIAG, None, prec, 0.0)
        K = H.Kinetic(None, None, None, dt, None, None, None)
        S = H.Schedule(4, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, fp, 10, 0, 0)
        return L.hmc_random_leapfrog_form(ctypes.byref(T), ctypes.byref(K), ctypes.byref(S))

    assert [form(100, dt) for dt in (0.1, 1e-3, 1.99, 9.9e-4, 2.0, 0.0)] == [1, 1, 1, 0, 0, 0]
    assert form(1000, 0.1) == 1 and form(2048, 0.1) == 1
    assert form(100, 0.1, fp=H.HMC_MODE_EXACT) == 0
    assert form(100, 0.1, prec=1) == 0          # any non-NULL diagonal: the general kernels
    assert form(64, 0.1) == 0 and form(4096, 0.1) == 0


GRID_DT = (1e-3, 1.5e-3, 3e-3, 1e-2, 0.1, 1, 1.9, 1.99, 1.999, 1.9999)
GRID_L_HIGH = (20, 128, 1024, 4096)
# what the rule L_high m <= 2e5 dt (1 - dt^2 / 4) (m = 2 from dt^2 = 2 on) answers over the grid, one
# row per dt: pinned, so that a change of the constants shows up here and is measured again
GRID_FORM = ((1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 1), (1, 1, 1, 1),
             (1, 1, 1, 0), (1, 1, 0, 0), (0, 0, 0, 0))


def test_three_term_routing_against_the_model(monkeypatch):
    """Wherever the host answers "three-term" over dt x L_high, the restatement of the kernels'
    recurrence (leapfrog_model.three_term) stays within 1e-10 of the long-double kick-drift-kick over
    a trajectory of L_high - 1 steps (unit-normal q and p, D = 100, max over every step and
    coordinate): a tenth of FAST mode's 1e-9 on q, which leaves room for about ten accepted
    iterations of accumulated drift and the kernels' sum order.  The reference is the long-double
    run, never the GPU.  The headline and bench schedules (dt = 0.1, L in 5..20) keep the
    three-term form, and D = 100 its four-chains-per-wave layout."""
    import leapfrog_model as M
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    answers, worst_in = [], 0.0
    for dt in GRID_DT:
        row = []
        for L_high in GRID_L_HIGH:
            f = H.random_leapfrog_form(100, max(1, L_high - 16), L_high, dt)
            dev = float(M.trajectory_deviation(dt, L_high - 1, D=100, seed=20)[-1])
            print(f"dt={dt:<7g} L_high={L_high:<5d} form={f} restatement vs long double: {dev:.3e}")
            # D = 100 takes the four-chain kernel exactly where the form is the three-term one; the
            # wave kernels of other shapes follow the same answer
            assert H.random_layout(100, max(1, L_high - 16), L_high, dt=dt) == ((4, 16, 4, 0) if f else (1, 64, 1, 1))
            assert H.random_leapfrog_form(66, max(1, L_high - 16), L_high, dt) == f
            assert H.random_leapfrog_form(1000, max(1, L_high - 16), L_high, dt) == f
            if f:
                worst_in = max(worst_in, dev)
                assert dev <= 1e-10, (dt, L_high, dev)
            row.append(f)
        answers.append(tuple(row))
    print(f"largest deviation inside the rule: {worst_in:.3e}")
    assert tuple(answers) == GRID_FORM
    # the flagship schedules: bench.py runs L in 5..20 at dt = 0.1 for the headline (D = 100), c2
    # (D = 100) and c4 (D = 1000)
    assert H.random_leapfrog_form(100, 5, 20, 0.1) == 1 and H.random_leapfrog_form(1000, 5, 20, 0.1) == 1
    assert H.random_layout(100, 5, 20) == (4, 16, 4, 0) == H.random_layout(100, 5, 20, dt=0.1)
    assert H.random_layout(1000, 5, 20) == (8, 64, 1, 1) == H.random_layout(1000, 5, 20, dt=0.1)
