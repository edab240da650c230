"""LogisticTarget (hmc_amd/target.py) on the host: V / dVdq against an independent restatement, the
hmc_logistic struct mirror, and the argument validation of the four hmc_logit_* entries, which runs
before any device access.  No GPU."""
import ctypes

import numpy as np
import pytest
from scipy.special import expit


def _logistic(n, D, seed, prior="vector"):
    from hmc_amd.target import LogisticTarget
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((n, D))
    beta = rs.standard_normal(D)
    y = (rs.random_sample(n) < expit(X @ beta)).astype(float)
    pv = rs.uniform(0.5, 2.0, D) if prior == "vector" else 1.7
    return LogisticTarget(X, y, pv), rs


def _restated(t, q):
    """V and dV/dq of one row from scipy's expit and np.logaddexp."""
    z = t.X @ q
    V = np.sum(np.logaddexp(0.0, z) - t.y * z) + 0.5 * np.sum(q * q / t.prior_var)
    return V, t.X.T @ (expit(z) - t.y) + q / t.prior_var


@pytest.mark.parametrize("n,D,prior", [(1, 1, "scalar"), (20, 2, "vector"), (100, 37, "vector"), (250, 64, "scalar")])
def test_V_and_gradient_match_restatement(n, D, prior):
    t, rs = _logistic(n, D, 100 + D, prior)
    assert (t.n, t.D) == (n, D) and t.diagonal is True
    assert np.array_equal(t.q0, np.zeros(D))
    q = 0.5 * rs.standard_normal((9, D))
    for row in q:
        V, g = _restated(t, row)
        np.testing.assert_allclose(t.V(row), V, rtol=1e-12)
        np.testing.assert_allclose(t.dVdq(row), g, rtol=1e-12, atol=1e-13)
    # batched rows equal single rows, for any leading shape (to the rounding of the n- and D-term
    # sums, whose order the BLAS picks by shape: the bound of the restatement above)
    Vb, gb = t.V(q), t.dVdq(q)
    assert Vb.shape == (9,) and gb.shape == (9, D)
    np.testing.assert_allclose(Vb, [t.V(r) for r in q], rtol=1e-12)
    np.testing.assert_allclose(gb, [t.dVdq(r) for r in q], rtol=1e-12, atol=1e-13)
    q3 = q[:8].reshape(2, 4, D)
    assert t.V(q3).shape == (2, 4) and t.dVdq(q3).shape == (2, 4, D)
    np.testing.assert_allclose(t.V(q3).ravel(), Vb[:8], rtol=1e-12)
    np.testing.assert_allclose(t.dVdq(q3).reshape(8, D), gb[:8], rtol=1e-12, atol=1e-13)


def test_far_points_stay_finite():
    t, _ = _logistic(50, 6, 3)
    for s in (1.0, -1.0):
        q = s * 1e3 * np.ones(6)
        assert np.isfinite(t.V(q)) and np.all(np.isfinite(t.dVdq(q)))
        V, g = _restated(t, q)
        np.testing.assert_allclose(t.V(q), V, rtol=1e-12)
        np.testing.assert_allclose(t.dVdq(q), g, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,D", [(20, 2), (60, 17)])
def test_gradient_against_central_differences(n, D):
    """|fd - g_d| <= h^2/6 |V'''_d| + (n + D) eps |V| / h with |V'''_d| <= sum_j |X_jd|^3 / (6 sqrt 3)
    (|sigma''| <= 1 / (6 sqrt 3); the quadratic prior has no third derivative)."""
    t, rs = _logistic(n, D, 7 + D)
    h, eps = 1e-5, np.finfo(float).eps
    third = np.sum(np.abs(t.X) ** 3, axis=0) / (6 * np.sqrt(3))
    for q in 0.5 * rs.standard_normal((4, D)):
        g = t.dVdq(q)
        tol = h * h / 6 * third + (n + D) * eps * abs(t.V(q)) / h
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            fd = (t.V(q + e) - t.V(q - e)) / (2 * h)
            assert abs(fd - g[d]) <= tol[d], (d, fd, g[d], tol[d])
        assert tol.max() < 1e-4                                   # the bound is a meaningful one


def test_constructor_assertions():
    from hmc_amd.target import LogisticTarget
    X, y = np.ones((4, 3)), np.array([0.0, 1.0, 1.0, 0.0])
    LogisticTarget(X, y)
    LogisticTarget(X, y.astype(int), prior_var=[1.0, 2.0, 3.0])
    LogisticTarget(X, y > 0.5, prior_var=2.0)
    for bad_y in (np.array([0.0, 1.0, 2.0, 0.0]), np.array([0.0, 0.5, 1.0, 0.0]), np.array([0.0, 1.0, -1.0, 0.0]),
                  np.array([0.0, 1.0, np.nan, 0.0]), y[:3], y[:, None]):
        with pytest.raises(AssertionError):
            LogisticTarget(X, bad_y)
    for bad_X in (np.ones(4), np.ones((0, 3)), np.ones((4, 0)), np.ones((4, 3, 1))):
        with pytest.raises(AssertionError):
            LogisticTarget(bad_X, y[:bad_X.shape[0]] if bad_X.ndim else y)
    for bad_pv in (0.0, -1.0, [1.0, 1.0], [1.0, 0.0, 1.0], np.ones((3, 1))):
        with pytest.raises(AssertionError):
            LogisticTarget(X, y, prior_var=bad_pv)


def test_logistic_struct_layout():
    from hmc_amd import _lib as H
    assert ctypes.sizeof(H.Logistic) == 40
    assert [(n, getattr(H.Logistic, n).offset) for n, _ in H.Logistic._fields_] == \
        [("D", 0), ("n", 4), ("ldx", 8), ("X", 16), ("y", 24), ("prior_prec", 32)]
    assert (H.LOGIT_MAX_D, H.LOGIT_MAX_N) == (128, 1 << 20)


def test_logit_entries_validate_before_any_launch(monkeypatch):
    """HMC_EINVAL for null arrays, D < 1, n < 1, ldx < D; HMC_ENOTSUP for D > 128, n > 2^20 and a full
    cov_p (minv_full, p_chol_t or kick): on the host, with fake device pointers that nothing reads."""
    from hmc_amd import _lib as H
    monkeypatch.setattr(H, "_lib", None)     # argtypes bound to this module's structure classes
    L = H.lib()
    P = 0x7000_0000
    K = H.Kinetic(None, None, None, 0.1, None, None, None)
    S = H.Schedule(4, 0, 10, 0, 1, 11, 5, 20, 1, 11, H.HMC_RNG_PHILOX, H.HMC_MODE_FAST, 10, 0, 0)
    st = H.State(P, P)

    def calls(M, Kin):
        return [L.hmc_logit_chain_init(M, Kin, S, None, P, st, None),
                L.hmc_logit_random_iters(M, Kin, S, None, st, None),
                L.hmc_logit_leapfrog(M, Kin, 4, P, P + 64, P + 128, P + 192, None),
                L.hmc_logit_energy(M, Kin, 4, P, P, P, None)]

    def logit(D=3, n=5, ldx=None, X=P, y=P, prec=P):
        return H.Logistic(D, n, D if ldx is None else ldx, X, y, prec)

    for bad in (logit(D=0), logit(n=0), logit(D=-1), logit(n=-3), logit(ldx=2), logit(X=None), logit(y=None),
                logit(prec=None)):
        assert calls(bad, K) == [H.HMC_EINVAL] * 4
        assert L.hmc_last_error()
    for bad in (logit(D=129), logit(n=(1 << 20) + 1)):
        assert calls(bad, K) == [H.HMC_ENOTSUP] * 4
    for i in (4, 5, 6):                       # minv_full, p_chol_t, kick
        args = [None, None, None, 0.1, None, None, None]
        args[i] = P
        assert calls(logit(), H.Kinetic(*args)) == [H.HMC_ENOTSUP] * 4
    assert b"cov_p" in L.hmc_last_error()
    # the limits themselves pass this check: a wrong L_chain is then the schedule's HMC_EINVAL
    S.L_chain = 7
    assert L.hmc_logit_random_iters(logit(D=128, n=1 << 20, ldx=200), K, S, None, st, None) == H.HMC_EINVAL
    assert b"L_chain" in L.hmc_last_error()
    assert L.hmc_logit_chain_init(logit(D=128, n=1 << 20), K, S, None, P, st, None) == H.HMC_EINVAL
    with pytest.raises(NotImplementedError):
        H.check(L.hmc_logit_energy(logit(D=129), K, 4, P, P, P, None), "x")
    with pytest.raises(AssertionError):
        H.check(L.hmc_logit_energy(logit(ldx=1), K, 4, P, P, P, None), "x")
    # a diagonal mass and a per-dimension dt are supported: an empty batch returns HMC_OK untouched
    S.L_chain, S.n_chains = 11, 0
    Kd = H.Kinetic(P, P, P, 0.0, None, None, None)
    assert L.hmc_logit_chain_init(logit(), Kd, S, None, None, st, None) == H.HMC_OK
    assert L.hmc_logit_random_iters(logit(), Kd, S, None, st, None) == H.HMC_OK
    assert L.hmc_logit_energy(logit(), Kd, 0, None, None, None, None) == H.HMC_OK
    assert L.hmc_logit_leapfrog(logit(), Kd, 0, None, None, None, None, None) == \
        H.HMC_EINVAL   # outputs alias inputs (all NULL), as hmc_leapfrog


def test_sampler_refuses_unsupported_logistic_setups():
    """NUTS, a full cov_p, D > 128 and n > 2^20 raise NotImplementedError in the constructor, before
    anything touches a device."""
    from hmc_amd.samplers import HMC_sampler
    from hmc_amd.target import LogisticTarget
    t, _ = _logistic(12, 4, 1)
    kw = dict(Nchain=2, Niter=10, dt=0.1, device="cpu")
    with pytest.raises(NotImplementedError):
        HMC_sampler(4, None, None, sampler_type="NUTS", d_max=5, target=t, **kw)
    cov_p = np.eye(4)
    cov_p[0, 1] = cov_p[1, 0] = 0.2
    with pytest.raises(NotImplementedError):
        HMC_sampler(4, None, None, sampler_type="Random", L_low=5, L_high=20, cov_p=cov_p, target=t, **kw)
    wide = LogisticTarget(np.zeros((2, 129)), np.array([0.0, 1.0]))
    with pytest.raises(NotImplementedError):
        HMC_sampler(129, None, None, sampler_type="Random", L_low=5, L_high=20, target=wide, **kw)
    n = (1 << 20) + 1
    tall = LogisticTarget(np.zeros((n, 1)), np.zeros(n))
    with pytest.raises(NotImplementedError):
        HMC_sampler(1, None, None, sampler_type="Random", L_low=5, L_high=20, target=tall, **kw)
    h = HMC_sampler(4, None, None, sampler_type="Random", L_low=5, L_high=20, cov_p=np.diag([0.9, 1.0, 1.1, 1.0]),
                    target=t, **kw)
    q = np.arange(4.0)
    assert h.V(q) == t.V(q) and np.array_equal(h.dVdq(q), t.dVdq(q))
